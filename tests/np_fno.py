"""Numpy restatement of frozen natural orbitals, written from the definitions and independent of afesp_amd/fno.py: the virtual-virtual
block of the MP2 one-particle density (closed and open shell) from full n^4 MO integral arrays, the natural virtuals with the kept and
the discarded block re-canonicalised, and the degenerate-cut rule.  Test infrastructure only.

Closed shell, t(i,j,a,b) = (ia|jb) / (e_i + e_j - e_a - e_b), i, j over the active occupied orbitals:
    D(a,b) = sum_ijc [2 t(i,j,a,c) - t(i,j,c,a)] t(i,j,b,c)
Open shell, t_ss(i,j,a,b) = [(ia|jb) - (ib|ja)] / D, t_ab(i,J,a,B) = (ia|JB) / D:
    D_a(a,b) = 1/2 sum_{ijc} t_aa(ijac) t_aa(ijbc) + sum_{iJC} t_ab(iJaC) t_ab(iJbC),   D_b the mirror image."""
from __future__ import annotations

import numpy as np

import np_ucc


def _amps(g, ea, eb, lo, oa, ob):
    """(ia|jb) / D for i in [lo, oa) of the first spin, j in [lo, ob) of the second; g full (first pair: first spin), or 8-fold packed
    (one spin; only the slice is gathered: a full n^4 array at n = 100 would not fit) -> (t[i, j, a, b], (ia|jb)[i, j, a, b])"""
    n = len(ea)
    if g.ndim == 1:
        i, j, a, b = np.meshgrid(np.arange(lo, oa), np.arange(lo, ob), np.arange(oa, n), np.arange(ob, n), indexing="ij")
        x = g[np_ucc.tri(np_ucc.tri(a, i), np_ucc.tri(b, j))]
    else:
        x = g[lo:oa, oa:, lo:ob, ob:].transpose(0, 2, 1, 3)
    d = ea[lo:oa, None, None, None] + eb[None, lo:ob, None, None] - ea[None, None, oa:, None] - eb[None, None, None, ob:]
    return x / d, x


def vv_density(n, nocc, nfc, eri_mo_packed, levels):
    """-> (D[v, v], frozen-core E(MP2)) of a closed shell from the 8-fold packed MO integrals"""
    e = np.asarray(levels, dtype=np.float64)
    t, x = _amps(np.asarray(eri_mo_packed), e, e, nfc, nocc, nocc)
    tt = 2.0 * t - t.transpose(0, 1, 3, 2)
    return np.einsum("ijac,ijbc->ab", tt, t, optimize=True), float(np.sum(x * tt))


def uvv_density(aa, ab, bb, ea, eb, na, nb, nfc):
    """-> (D_alpha, D_beta, frozen-core E(UMP2)) from the full arrays of np_ucc.mo_blocks (ab: alpha pair first)"""
    ea, eb = np.asarray(ea, dtype=np.float64), np.asarray(eb, dtype=np.float64)
    out, e2 = [], 0.0
    for g, e, o in ((aa, ea, na), (bb, eb, nb)):
        t, x = _amps(g, e, e, nfc, o, o)
        t = t - t.transpose(0, 1, 3, 2)
        out.append(0.5 * np.einsum("ijac,ijbc->ab", t, t, optimize=True))
        e2 += 0.25 * float(np.sum((x - x.transpose(0, 1, 3, 2)) * t))
    t, x = _amps(ab, ea, eb, nfc, na, nb)                     # t[i, J, a, B]
    e2 += float(np.sum(x * t))
    return out[0] + np.einsum("iJaC,iJbC->ab", t, t, optimize=True), out[1] + np.einsum("iJaB,iJaC->BC", t, t, optimize=True), e2


def widened(occ, n_keep):
    """The count kept when `n_keep` is asked for: every occupation that agrees with the last kept one to a relative 1e-8 stays as well."""
    occ = np.asarray(occ)
    last = occ[n_keep - 1]
    more = [k for k in range(n_keep, len(occ)) if abs(occ[k] - last) <= 1e-8 * max(abs(occ[k]), abs(last))]
    return more[-1] + 1 if more else n_keep


def natural_orbitals(d_vv, coeff, levels, nocc, n_keep):
    """-> (occupations descending, C', levels'): eigenvectors of D taken from -D so that they come out in descending order; each block
    of natural virtuals is made canonical by diagonalising the virtual Fock matrix (diagonal in the canonical basis) projected on it."""
    coeff, levels = np.asarray(coeff), np.asarray(levels)
    w, U = np.linalg.eigh(-np.asarray(d_vv))
    fv = np.diag(levels[nocc:])
    rows, lev = [coeff[:nocc]], [levels[:nocc]]
    for blk in (U[:, :n_keep], U[:, n_keep:]):
        if blk.shape[1] == 0:
            continue
        e, R = np.linalg.eigh(blk.T @ fv @ blk)
        rows.append(R.T @ blk.T @ coeff[nocc:])
        lev.append(e)
    return -w, np.vstack(rows), np.concatenate(lev)


def best_cut(occ, lo=0.5, hi=0.8):
    """The count between lo v and hi v behind which the occupations drop by the largest ratio: never inside a degenerate pair"""
    occ = np.asarray(occ)
    v = len(occ)
    cands = [k for k in range(1, v) if lo * v <= k <= hi * v]
    return max(cands, key=lambda k: occ[k - 1] / max(occ[k], 1e-300))
