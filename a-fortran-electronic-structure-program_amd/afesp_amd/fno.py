"""Frozen natural orbitals, host side (numpy; importable without a GPU).

The virtual-virtual block D of the MP2 one-particle density comes from the engine (Engine.mp2_vv_density / ump2_vv_density).  Everything
after it is v x v linear algebra and lives here (and, statement for statement, in host/els_host.f90):

  1. D = U diag(occ) U^T, occupations in descending order;
  2. the cut: a count, or every occupation >= occ_tol; a cut that would fall between occupations that agree to a relative 1e-8 is moved
     up until the whole degenerate set is kept (the subspace of a split set is arbitrary, and so would the energy be);
  3. the kept block is re-canonicalised -- U_k^T diag(e_virt) U_k is diagonalised, which gives the new levels and a rotation -- and so
     is the discarded block, so that the coefficient matrix stays square and orthonormal and the Fock matrix is diagonal within the
     occupied, the kept and the discarded block (not between the last two: the window cuts that coupling off);
  4. C' = [occupied ; kept ; discarded] (MO x AO rows), levels' likewise.

A second transform with C' and the orbital window (nfc, v - n_keep) then leave the unchanged solvers a canonical problem in the truncated
virtual space.  Delta MP2 = E(MP2, all virtuals) - E(MP2, kept virtuals) is the customary correction for what the cut lost."""
from __future__ import annotations

import numpy as np

DEGENERATE_RTOL = 1e-8


def occupations(d_vv):
    """-> (occupations descending, eigenvectors as columns in that order) of the symmetric v x v density block"""
    w, U = np.linalg.eigh(np.asarray(d_vv, dtype=np.float64))
    order = np.argsort(-w, kind="stable")
    return w[order], U[:, order]


def _same(x, y):
    return abs(x - y) <= DEGENERATE_RTOL * max(abs(x), abs(y))


def widen_cut(occ, n_keep):
    """The smallest count >= n_keep that does not split a set of occupations agreeing to a relative 1e-8."""
    n_keep, v = int(n_keep), len(occ)
    while 0 < n_keep < v and _same(occ[n_keep - 1], occ[n_keep]):
        n_keep += 1
    return n_keep


def choose_cut(occ, n_keep=None, occ_tol=0.0, report=print):
    """The number of natural virtuals kept: `n_keep` of them, or every occupation >= occ_tol; widened over a degenerate set.  Exactly
    one of the two is given; the count must leave at least one virtual and not exceed their number."""
    v = len(occ)
    if (n_keep is None or n_keep < 0) == (not occ_tol or occ_tol <= 0.0):
        raise ValueError("give either the number of natural virtuals kept or an occupation threshold")
    asked = int(n_keep) if (n_keep is not None and n_keep >= 0) else int(np.count_nonzero(np.asarray(occ) >= occ_tol))
    if asked < 1 or asked > v:
        raise ValueError(f"the cut keeps {asked} of {v} natural virtuals: it must keep at least one and at most all of them")
    kept = widen_cut(occ, asked)
    if report is not None:
        note = "" if kept == asked else f" (asked for {asked}: degenerate occupations are kept together)"
        report(f"Number of natural virtuals kept: {kept}{note}")
    return kept


def rotate_block(coeff_virt, levels_virt, U):
    """The orbitals U^T C_virt made canonical among themselves -> (rows of C', their levels ascending)"""
    if U.shape[1] == 0:
        return np.zeros((0, coeff_virt.shape[1])), np.zeros(0)
    fock = U.T @ (np.asarray(levels_virt)[:, None] * U)
    e, R = np.linalg.eigh(0.5 * (fock + fock.T))
    return (U @ R).T @ coeff_virt, e


def rotated_orbitals(coeff, levels, nocc, U, n_keep):
    """C' = [occupied ; kept natural virtuals ; discarded ones], each virtual block canonical within itself, and levels'."""
    coeff, levels = np.asarray(coeff, dtype=np.float64), np.asarray(levels, dtype=np.float64)
    ck, ek = rotate_block(coeff[nocc:], levels[nocc:], U[:, :n_keep])
    cd, ed = rotate_block(coeff[nocc:], levels[nocc:], U[:, n_keep:])
    return np.vstack([coeff[:nocc], ck, cd]), np.concatenate([levels[:nocc], ek, ed])


def natural_virtuals(d_vv, coeff, levels, nocc, n_keep=None, occ_tol=0.0, report=print):
    """One spin (or the closed shell): -> (count kept, occupations descending, C' (MO x AO), levels')."""
    occ, U = occupations(d_vv)
    kept = choose_cut(occ, n_keep, occ_tol, report)
    c2, e2 = rotated_orbitals(coeff, levels, nocc, U, kept)
    return kept, occ, c2, e2


def natural_virtuals_uhf(d_a, d_b, coeff_a, coeff_b, levels_a, levels_b, nalpha, nbeta, n_keep=None, occ_tol=0.0, report=print):
    """Both spins of an open shell.  The orbital window drops the same number of highest orbitals for both spins, so one number serves
    both: n_keep counts the natural virtuals kept in the smaller of the two virtual spaces, n_drop = min(va, vb) - n_keep is dropped from
    either spin.  A threshold takes the larger of the two spins' counts (the smaller n_drop); the degenerate-set rule holds for both.
    -> (n_keep, (occ_a, occ_b), C'_a, C'_b, levels'_a, levels'_b)"""
    (oa, Ua), (ob, Ub) = occupations(d_a), occupations(d_b)
    va, vb = len(oa), len(ob)
    vmin = min(va, vb)
    if (n_keep is None or n_keep < 0) == (not occ_tol or occ_tol <= 0.0):
        raise ValueError("give either the number of natural virtuals kept or an occupation threshold")
    if n_keep is not None and n_keep >= 0:
        asked = int(n_keep)
    else:
        drop = min(va - int(np.count_nonzero(oa >= occ_tol)), vb - int(np.count_nonzero(ob >= occ_tol)))
        asked = vmin - drop
    if asked < 1 or asked > vmin:
        raise ValueError(f"the cut keeps {asked} of {vmin} natural virtuals: it must keep at least one and at most all of them")
    drop = vmin - asked
    while True:   # (a set widened in one spin moves the other spin's cut as well)
        new = min(va - widen_cut(oa, va - drop), vb - widen_cut(ob, vb - drop))
        if new == drop:
            break
        drop = new
    kept = vmin - drop
    if report is not None:
        note = "" if kept == asked else f" (asked for {asked}: degenerate occupations are kept together)"
        report(f"Number of natural virtuals kept: {kept}{note}")
    ca, ea = rotated_orbitals(coeff_a, levels_a, nalpha, Ua, va - drop)
    cb, eb = rotated_orbitals(coeff_b, levels_b, nbeta, Ub, vb - drop)
    return kept, (oa, ob), ca, cb, ea, eb
