"""The Lambda solve of a spin-orbital CCSD state and what follows from its unrelaxed one-particle density: the spin blocks, natural
occupation numbers and one-electron expectation values (host code; the device calls are Engine.so_lambda_* / so_density), and from its
two-particle density (Engine.so_density2_*): the full two-particle density, <S^2> and the density-side energy; and the orbital-relaxed
one-particle density (Engine.so_zvector_solve / so_relaxed_density), which the same helpers take as they take the unrelaxed one.

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


def total_rdm2(d, gamma, nocc):
    """<a+_p a+_q a_s a_r> over the spin orbitals from the engine's correlation parts d (so_density) and gamma (so_density2_get("full")): the
    reference determinant's part, the one-particle parts and gamma.  An (o+v)^4 array: for small cases."""
    d, gamma = np.asarray(d, dtype=np.float64), np.asarray(gamma, dtype=np.float64)
    g0 = np.diag((np.arange(d.shape[0]) < nocc).astype(np.float64))
    ref = np.einsum("pr,qs->pqrs", g0, g0) - np.einsum("ps,qr->pqrs", g0, g0)
    one = (np.einsum("pr,qs->pqrs", d, g0) + np.einsum("qs,pr->pqrs", d, g0) - np.einsum("ps,qr->pqrs", d, g0)
           - np.einsum("qr,ps->pqrs", d, g0))
    return ref + one + gamma


def _spin_flip_overlap(nbasis, nalpha, nbeta, interleaved, beta_in_alpha):
    """(alpha spin orbitals, beta spin orbitals, S[beta spin orbital, alpha spin orbital])"""
    orb, spin = so_spin_order(nbasis, nalpha, nbeta, interleaved)
    ia, ib = np.where(spin == 0)[0], np.where(spin == 1)[0]
    m = np.eye(int(nbasis)) if beta_in_alpha is None else np.asarray(beta_in_alpha, dtype=np.float64)
    return ia, ib, m[np.ix_(orb[ib], orb[ia])]


def _spin_flip_pair(x, y, ia, ib, s):
    """sum over p, r beta and q, s alpha of (x_pr y_qs - x_ps y_qr) S_ps S_rq"""
    return float(np.trace(x[np.ix_(ib, ib)] @ s @ y[np.ix_(ia, ia)] @ s.T) - np.sum(x[np.ix_(ib, ia)] * s) * np.sum(y[np.ix_(ia, ib)] * s.T))


def s_squared_reference(nbasis, nalpha, nbeta, interleaved, beta_in_alpha=None):
    """<S^2> of the reference determinant of a state: N/2 + Ms^2 - sum over occupied alpha a and beta b of <b|a>^2"""
    ia, ib, s = _spin_flip_overlap(nbasis, nalpha, nbeta, interleaved, beta_in_alpha)
    g0 = np.diag((np.arange(2 * int(nbasis)) < nalpha + nbeta).astype(np.float64))
    ms = 0.5 * (nalpha - nbeta)
    return 0.5 * (nalpha + nbeta) + ms * ms - _spin_flip_pair(g0, g0, ia, ib, s)


def s_squared(eng, nbasis, nalpha, nbeta, interleaved, beta_in_alpha=None):
    """<S^2> = N/2 + Ms^2 - sum_PQ Gtot[P beta, Q alpha, Q beta, P alpha] of the engine's CCSD state (unrelaxed; needs a live Lambda state and
    so_density2_build for the current t and lambda).  The correlation part goes through Engine.so_density2_expect with the spin-flip
    overlaps as the two matrices, the reference and one-particle parts are one-body algebra here.  beta_in_alpha as natural_occupations
    takes it: <beta orbital b | alpha orbital a> where the two spins have different orbitals."""
    ia, ib, s = _spin_flip_overlap(nbasis, nalpha, nbeta, interleaved, beta_in_alpha)
    n2 = 2 * int(nbasis)
    d = eng.so_density()
    g0 = np.diag((np.arange(n2) < nalpha + nbeta).astype(np.float64))
    a = np.zeros((n2, n2))
    a[np.ix_(ib, ia)] = s
    # Gamma_pqrs S_ps S_rq = -Gamma_pqsr S_ps S_rq: A_pr B_qs with A the (beta, alpha) overlap and B its transpose
    corr = -eng.so_density2_expect(a, a.T)
    ms = 0.5 * (nalpha - nbeta)
    flips = _spin_flip_pair(g0, g0, ia, ib, s) + _spin_flip_pair(d, g0, ia, ib, s) + _spin_flip_pair(g0, d, ia, ib, s) + corr
    return 0.5 * (nalpha + nbeta) + ms * ms - flips


def so_relaxed_density_solve(eng, tol=1e-10, maxiter=100):
    """The orbital-relaxed correlation density of the engine's CCSD state: builds the two-particle density of the current
    t and lambda if there is no live build, solves the Z-vector equations on the device and -> (d_rel, z, iterations).  d_rel is laid out
    as Engine.so_density: spatial_blocks, natural_occupations and expectation take it as they take the unrelaxed matrix.  Needs a live
    (converged) Lambda state; a state made by uso_init_fock is refused (status 24), a solve that does not converge raises status 25."""
    try:
        z, it, _ = eng.so_zvector_solve(tol, maxiter)
    except AfespError as err:
        if not str(err).startswith("status 21:"):   # (AFESP_LAMBDA_STALE: no live build -- or no live Lambda state, which the build reports)
            raise
        eng.so_density2_build()
        z, it, _ = eng.so_zvector_solve(tol, maxiter)
    return eng.so_relaxed_density(), z, it


def energy_from_densities(eng):
    """The density-side correlation energy of the engine's state: -> (e, difference), e the eight numbers of Engine.so_density2_energy
    (sum f D, the six family contributions of 1/4 sum g Gamma, their sum) and difference = e[0] + e[7] - E(CCSD) at the state's current
    amplitudes: zero at converged t and lambda, where the discarded Lagrangian terms vanish."""
    e = eng.so_density2_energy()
    e_cc = eng.so_energy()[0]
    return e, float(e[0] + e[7] - e_cc)
