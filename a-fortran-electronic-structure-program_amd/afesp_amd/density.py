"""The Lambda solve of a spin-orbital CCSD state and what follows from its unrelaxed one-particle density: the spin blocks, natural
occupation numbers and one-electron expectation values (host code; the device calls are Engine.so_lambda_* / so_density).

Spin-orbital orders of the engine's states (include/afesp.h): the RHF-fed state (Engine.init_cc_spinorb) is interleaved -- spin orbital
2 P + spin over the spatial orbitals P in level order; the UHF- and Fock-fed states (init_cc_uspinorb, uso_init_fock) are block-ordered --
occupied alpha, occupied beta, virtual alpha, virtual beta."""
from __future__ import annotations

import numpy as np

from .capi import AfespError


def so_lambda_solve(eng, maxiter=100, e_tol=1e-8, l_tol=1e-8, diis_nerr=8):
    """Lambda of the state's current amplitudes: init, then Jacobi steps with DIIS -> (iterations, pseudo energies incl. the start
    line, un-rooted rms).  Raises AfespError if maxiter steps do not converge."""
    eng.so_lambda_init(diis_nerr)
    e, r, _ = eng.so_lambda_energy(e_tol, l_tol)
    en, rm = [e], [r]
    for it in range(1, maxiter + 1):
        e, r, conv = eng.so_lambda_iterate(e_tol, l_tol)
        en.append(e)
        rm.append(r)
        if conv:
            return it, np.array(en), np.array(rm)
        eng.so_lambda_diis()
    raise AfespError(f"the Lambda equations did not converge in {maxiter} iterations")


def so_lambda_t_correction(eng, t_begin=0, t_end=None, maxiter=100, e_tol=1e-8, l_tol=1e-8, diis_nerr=8):
    """Lambda-CCSD(T) beside (T) for the triples [t_begin, t_end) of the engine's list (default: all) -> (e_lt, e_t).  A live Lambda state
    of the current amplitudes is used as it stands (the caller converged it, or set it); without one the Lambda equations are solved
    first (so_lambda_solve with the given limits)."""
    try:
        e_lt = eng.so_lambda_t(t_begin, t_end)
    except AfespError as err:
        if not str(err).startswith("status 21:"):   # (AFESP_LAMBDA_STALE: no Lambda state, or t1 / t2 changed since its init)
            raise
        so_lambda_solve(eng, maxiter, e_tol, l_tol, diis_nerr)
        e_lt = eng.so_lambda_t(t_begin, t_end)
    return e_lt, eng.do_ccsd_t_spinorb(t_begin, t_end)


def so_spin_order(nbasis, nalpha, nbeta, interleaved):
    """(spatial orbital, spin) of every spin orbital of a state, in its own order"""
    n = int(nbasis)
    if interleaved:
        if nalpha != nbeta:
            raise ValueError("the interleaved (RHF-fed) order has nalpha == nbeta")
        x = np.arange(2 * n)
        return x // 2, x % 2
    orb = np.concatenate([np.arange(nalpha), np.arange(nbeta), np.arange(nalpha, n), np.arange(nbeta, n)])
    spin = np.concatenate([np.zeros(nalpha, int), np.ones(nbeta, int), np.zeros(n - nalpha, int), np.ones(n - nbeta, int)])
    return orb, spin


def spatial_blocks(d, nbasis, nalpha, nbeta, interleaved):
    """The alpha and the beta n x n one-particle density matrices, reference determinant included, from the engine's correlation density d
    over the spin orbitals."""
    n = int(nbasis)
    d = np.asarray(d, dtype=np.float64)
    if d.shape != (2 * n, 2 * n):
        raise ValueError("the density is (2 nbasis) x (2 nbasis)")
    orb, spin = so_spin_order(n, nalpha, nbeta, interleaved)
    full = d + np.diag((np.arange(2 * n) < nalpha + nbeta).astype(np.float64))
    out = []
    for s in (0, 1):
        idx = np.where(spin == s)[0]
        m = np.zeros((n, n))
        m[np.ix_(orb[idx], orb[idx])] = full[np.ix_(idx, idx)]
        out.append(m)
    return out[0], out[1]


def natural_occupations(da, db, beta_in_alpha=None):
    """Spin-summed natural occupation numbers, descending.  da and db are matrices in the alpha and in the beta orbitals: where the two
    sets differ (UHF, semicanonical ROHF orbitals) beta_in_alpha[b, a] = <beta orbital b | alpha orbital a> (C_b S C_a^T, or u_b u_a^T for
    two rotations u[new, old] of one orthonormal set) brings db into the alpha orbitals first; None: one set of orbitals."""
    da, db = np.asarray(da, dtype=np.float64), np.asarray(db, dtype=np.float64)
    if beta_in_alpha is not None:
        m = np.asarray(beta_in_alpha, dtype=np.float64)
        db = m.T @ db @ m
    d = da + db
    return np.sort(np.linalg.eigvalsh(0.5 * (d + d.T)))[::-1]


def expectation(da, db, a_mo_alpha, a_mo_beta=None):
    """<A> of a one-electron operator given in the MO basis of each spin (the beta matrix defaults to the alpha one)"""
    a_mo_beta = a_mo_alpha if a_mo_beta is None else a_mo_beta
    return float(np.sum(da * np.asarray(a_mo_alpha)) + np.sum(db * np.asarray(a_mo_beta)))
