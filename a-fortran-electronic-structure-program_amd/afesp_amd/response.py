"""EOM-CCSD linear response of a spin-orbital CCSD state: the response function <<X;Y>>_omega and the polarisability alpha(omega) over
Engine.so_response_* (host code).

    (A - omega) R^X(omega) = -xi^X,     <<X;Y>>_omega = Phi[X, R^Y(omega)] + Phi[Y, R^X(-omega)],     alpha_XY(omega) = -<<X;Y>>_omega

This is the EOM-CC response function (Stanton and Bartlett), not the LR-CC one: the term quadratic in the perturbed amplitudes is absent
by definition, <<X;Y>>_omega = <<Y;X>>_-omega holds but alpha_XY(omega) != alpha_YX(omega) in general off omega = 0.  For two electrons it
is exact.  Real frequencies only; the orbitals do not relax."""
from __future__ import annotations

import numpy as np


def signed_frequencies(omegas):
    """the signed list the library solves for: +omega and -omega of every frequency, each value once, in order of first appearance"""
    out = []
    for w in np.atleast_1d(np.asarray(omegas, dtype=np.float64)):
        for s in (float(w), -float(w)):
            if not any(s == x for x in out):
                out.append(s + 0.0)                                          # (-0.0 + 0.0 = 0.0)
    return out


def default_max_space(nsys, nunique):
    """eight vectors per system, at least 2 nsys (what the library asks for), at most what it takes"""
    return min(4096, max(2 * nsys, min(int(nunique), 8 * nsys)))


def so_response_solve(eng, operators, omegas, tol=1e-8, max_space=None, maxiter=100):
    """<<X_a;X_b>>_omega of the engine's spin-orbital state at its converged amplitudes and Lambda, for the symmetric one-body operators
    `operators` [(o+v, o+v) each, over the state's spin orbitals in its order] and the real frequencies `omegas`.  A live, converged Lambda
    state is needed (density.so_lambda_solve).  All right-hand sides -- operators x (+omega, -omega) -- share one basis: every sigma build
    serves every system.
    -> (response [nfreq, nop, nop], info) -- info: iterations, nsigma, resnorm [signed frequencies, nop], omega_signed, max_space.
    Raises AfespError: status 26 when a frequency is at an excitation energy of the projected EOM matrix (a pole), status 27 when
    maxiter steps do not converge."""
    if maxiter < 1:
        raise ValueError("so_response_solve: maxiter must be at least 1")
    ops = np.asarray(operators, dtype=np.float64)
    om = np.atleast_1d(np.asarray(omegas, dtype=np.float64))
    signed = signed_frequencies(om)
    o, v = eng.so_o, eng.so_v
    nsys = len(signed) * (ops.shape[0] if ops.ndim == 3 else 1)
    ms = max_space if max_space is not None else default_max_space(nsys, o * v + (o * (o - 1) // 2) * (v * (v - 1) // 2))
    eng.so_response_init(ops, signed, ms)
    for it in range(1, maxiter + 1):
        res, nsigma, conv = eng.so_response_iterate(tol)
        if conv:
            break
    out = eng.so_response_function(om)                                       # (status 27 where maxiter steps were not enough)
    return out, dict(iterations=it, nsigma=nsigma, resnorm=res, omega_signed=np.array(signed), max_space=ms)


def mean_and_anisotropy(alpha):
    """isotropic mean tr(alpha) / 3 and the anisotropy sqrt(1/2 [(a_xx - a_yy)^2 + (a_yy - a_zz)^2 + (a_zz - a_xx)^2 + 6 (a_xy^2 + a_yz^2 +
    a_zx^2)]) of one 3 x 3 tensor, off-diagonal elements symmetrised"""
    a = 0.5 * (np.asarray(alpha) + np.asarray(alpha).T)
    iso = float(np.trace(a)) / 3.0
    an2 = 0.5 * ((a[0, 0] - a[1, 1]) ** 2 + (a[1, 1] - a[2, 2]) ** 2 + (a[2, 2] - a[0, 0]) ** 2) + 3.0 * (a[0, 1] ** 2 + a[1, 2] ** 2 + a[2, 0] ** 2)
    return iso, float(np.sqrt(an2))


def polarizability(eng, dipole_so, omegas, tol=1e-8, max_space=None, maxiter=100):
    """alpha(omega) = -<<mu;mu>>_omega.  dipole_so: the three Cartesian components of the dipole operator as symmetric matrices over the
    state's spin orbitals, in its order (afesp_amd.density.so_spin_order) -- the operator is the caller's, in the same molecular orbitals
    as the state, as for eom.oscillator_strengths.
    -> (alpha [nfreq, 3, 3], isotropic mean [nfreq], anisotropy [nfreq], info of so_response_solve)"""
    n = eng.so_o + eng.so_v
    dipole_so = [np.asarray(m, dtype=np.float64) for m in dipole_so]
    if len(dipole_so) != 3 or any(m.shape != (n, n) or not np.allclose(m, m.T, rtol=0.0, atol=1e-12 * max(1.0, np.max(np.abs(m))))
                                  for m in dipole_so):
        raise ValueError("polarizability: dipole_so is three symmetric matrices over the state's spin orbitals")
    rf, info = so_response_solve(eng, np.stack(dipole_so), omegas, tol=tol, max_space=max_space, maxiter=maxiter)
    alpha = -rf
    ma = [mean_and_anisotropy(a) for a in alpha]
    return alpha, np.array([x[0] for x in ma]), np.array([x[1] for x in ma]), info


def table(omegas, alpha, iso, aniso, info):
    """The lines the Fortran host prints for cc_polar: one 3 x 3 table per frequency with the mean and the anisotropy, then the sigma
    builds and the largest residual"""
    lines = []
    for f, w in enumerate(np.atleast_1d(omegas)):
        lines.append(f"  omega = {w:14.8f} Eh")
        for r, c in enumerate("xyz"):
            lines.append(f"    {c}  {alpha[f][r, 0]:18.10f}{alpha[f][r, 1]:18.10f}{alpha[f][r, 2]:18.10f}")
        lines.append(f"    mean {iso[f]:18.10f}   anisotropy {aniso[f]:18.10f}")
    lines.append(f"  response sigma builds: {info['nsigma']}   largest residual: {float(np.max(info['resnorm'])):11.3e}")
    return "\n".join(lines)
