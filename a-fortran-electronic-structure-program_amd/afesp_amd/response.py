"""EOM-CCSD linear response of a spin-orbital CCSD state: the response function <<X;Y>>_omega and the polarisability alpha(omega) over
Engine.so_response_* (host code).

    (A - omega) R^X(omega) = -xi^X,     <<X;Y>>_omega = Phi[X, R^Y(omega)] + Phi[Y, R^X(-omega)],     alpha_XY(omega) = -<<X;Y>>_omega

This is the EOM-CC response function (Stanton and Bartlett), not the LR-CC one: the term quadratic in the perturbed amplitudes is absent
by definition, <<X;Y>>_omega = <<Y;X>>_-omega holds but alpha_XY(omega) != alpha_YX(omega) in general off omega = 0.  For two electrons it
is exact.  The orbitals do not relax.  Complex frequencies z = omega + i gamma -- damped response inside the spectrum, the absorption
cross-section, alpha(i omega) and C6 -- are the *_complex functions further down."""
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


# ---------------------------------------------------------------------------------------------------------------- complex frequencies
# z = omega + i gamma: (A - z) R(z) = -xi with A and xi real, <<X;Y>>_z = Phi[X, R^Y(z)] + Phi[Y, R^X(-z)] -- the analytic
# continuation of the function above.  R(conj z) = conj R(z), so an imaginary z needs one solve (-z = conj z), any other z two.
LIGHT_SPEED = 137.035999084                                                  # c in atomic units
# Default of casimir_polder_grid: the smallest n at which the quadrature of the two-electron FCI alpha-bar(iu) (lowest gap 1.76 Eh) with
# u0 = 0.3 is within 1e-6 relative of the closed form (2.1e-7; tests/test_response_complex_cpu.py).  With three
# operators that is 57 systems: one response state (at most 64).
C6_NPTS = 19


def signed_complex_frequencies(zs):
    """the list the library solves for: every z, and -z where Re z != 0 (for an imaginary z, -z is its conjugate: nothing to add), each
    value once, in order of first appearance"""
    out = []
    for z in np.atleast_1d(np.asarray(zs, dtype=np.complex128)):
        z = complex(z.real + 0.0, z.imag + 0.0)
        for s in ((z,) if z.real == 0.0 else (z, complex(-z.real + 0.0, -z.imag + 0.0))):
            if not any(s == x for x in out):
                out.append(s)
    return out


def default_max_space_complex(nsys, nunique):
    """sixteen vectors per system (two per system and step), at least 4 nsys (what the library asks for), at most what it takes: the real
    basis cannot outgrow the unique amplitudes, and a step's 2 nsys pending vectors must fit beside it"""
    return min(4096, max(4 * nsys, min(int(nunique) + 2 * nsys, 16 * nsys)))


def so_response_solve_complex(eng, operators, zs, tol=1e-8, max_space=None, maxiter=100):
    """<<X_a;X_b>>_z at the complex frequencies `zs`, as so_response_solve: all systems -- operators x signed_complex_frequencies(zs) --
    share one real basis, every sigma build serves every system, a solution is two vectors.
    -> (response [nfreq, nop, nop] complex, info) -- info: iterations, nsigma, resnorm [signed frequencies, nop], z_signed, max_space.
    Raises AfespError: status 26 only where a z with Im z = 0 is at a pole, status 27 when maxiter steps do not converge."""
    if maxiter < 1:
        raise ValueError("so_response_solve_complex: maxiter must be at least 1")
    ops = np.asarray(operators, dtype=np.float64)
    z = np.atleast_1d(np.asarray(zs, dtype=np.complex128))
    signed = signed_complex_frequencies(z)
    o, v = eng.so_o, eng.so_v
    nsys = len(signed) * (ops.shape[0] if ops.ndim == 3 else 1)
    ms = max_space if max_space is not None else default_max_space_complex(nsys, o * v + (o * (o - 1) // 2) * (v * (v - 1) // 2))
    eng.so_response_init_complex(ops, signed, ms)
    for it in range(1, maxiter + 1):
        res, nsigma, conv = eng.so_response_iterate(tol)
        if conv:
            break
    out = eng.so_response_function_complex(z)                                # (status 27 where maxiter steps were not enough)
    return out, dict(iterations=it, nsigma=nsigma, resnorm=res, z_signed=np.array(signed), max_space=ms)


def polarizability_complex(eng, dipole_so, zs, tol=1e-8, max_space=None, maxiter=100):
    """alpha(z) = -<<mu;mu>>_z at complex frequencies; dipole_so as for polarizability.
    -> (alpha [nfreq, 3, 3] complex, isotropic mean tr(alpha) / 3 [nfreq] complex, info of so_response_solve_complex)"""
    n = eng.so_o + eng.so_v
    dipole_so = [np.asarray(m, dtype=np.float64) for m in dipole_so]
    if len(dipole_so) != 3 or any(m.shape != (n, n) or not np.allclose(m, m.T, rtol=0.0, atol=1e-12 * max(1.0, np.max(np.abs(m))))
                                  for m in dipole_so):
        raise ValueError("polarizability_complex: dipole_so is three symmetric matrices over the state's spin orbitals")
    rf, info = so_response_solve_complex(eng, np.stack(dipole_so), zs, tol=tol, max_space=max_space, maxiter=maxiter)
    alpha = -rf
    return alpha, np.trace(alpha, axis1=1, axis2=2) / 3.0, info


def absorption_cross_section(omegas, gamma, alpha):
    """sigma(omega) = 4 pi omega / c Im alpha-bar(omega + i gamma) in atomic units; alpha: the isotropic means [nfreq] (complex) or the
    tensors [nfreq, 3, 3] at omega + i gamma.  gamma enters through alpha alone; it is taken to say which damping the numbers belong to"""
    w = np.atleast_1d(np.asarray(omegas, dtype=np.float64))
    a = np.asarray(alpha, dtype=np.complex128)
    if not gamma > 0.0:
        raise ValueError("absorption_cross_section: gamma must be positive")
    iso = np.trace(a, axis1=1, axis2=2) / 3.0 if a.ndim == 3 else np.atleast_1d(a)
    if iso.shape != w.shape:
        raise ValueError("absorption_cross_section: one alpha per frequency")
    return 4.0 * np.pi * w / LIGHT_SPEED * iso.imag


def casimir_polder_grid(n=C6_NPTS, u0=0.3):
    """Gauss-Legendre nodes t_k in (-1, 1) mapped to u = u0 (1 + t) / (1 - t) on (0, inf), with the weights w_k 2 u0 / (1 - t_k)^2
    -> (u [n], weights [n])"""
    if n < 1 or not u0 > 0.0:
        raise ValueError("casimir_polder_grid: n >= 1 and u0 > 0")
    t, w = np.polynomial.legendre.leggauss(int(n))
    return u0 * (1.0 + t) / (1.0 - t), w * 2.0 * u0 / (1.0 - t) ** 2


def c6_coefficient(alpha_a, alpha_b, weights):
    """C6^AB = (3 / pi) int_0^inf alpha-bar_A(iu) alpha-bar_B(iu) du on the grid of casimir_polder_grid: alpha_a, alpha_b are the isotropic
    means at i u_k (their imaginary parts, zero up to the solver's tolerance, are dropped)"""
    a, b, w = (np.asarray(x) for x in (alpha_a, alpha_b, weights))
    if not a.shape == b.shape == w.shape:
        raise ValueError("c6_coefficient: one alpha of each monomer per grid point")
    return float(3.0 / np.pi * np.sum(w * a.real * b.real))


def table_complex(omegas, gamma, alpha, info):
    """The lines the Fortran host prints for cc_polar with polar_gamma > 0: per frequency the real and the imaginary 3 x 3 table, Re and Im of
    the mean and the absorption cross-section, then the sigma builds and the largest residual"""
    w = np.atleast_1d(omegas)
    iso = np.trace(np.asarray(alpha), axis1=1, axis2=2) / 3.0
    sig = absorption_cross_section(w, gamma, iso)
    lines = []
    for f in range(len(w)):
        lines.append(f"  omega = {w[f]:14.8f} Eh   gamma = {gamma:14.8f} Eh")
        for part, name in ((alpha[f].real, "Re"), (alpha[f].imag, "Im")):
            for r, c in enumerate("xyz"):
                lines.append(f"    {name} {c}  {part[r, 0]:18.10f}{part[r, 1]:18.10f}{part[r, 2]:18.10f}")
        lines.append(f"    Re mean {iso[f].real:18.10f}   Im mean {iso[f].imag:18.10f}   sigma {sig[f]:18.10f}")
    lines.append(f"  response sigma builds: {info['nsigma']}   largest residual: {float(np.max(info['resnorm'])):11.3e}")
    return "\n".join(lines)


def table_c6(u, weights, iso, info, u0=0.3):
    """The lines the Fortran host prints for polar_c6_npts > 0: the grid, alpha-bar(i u_k) and the homo-dimer C6"""
    lines = [f"  Casimir-Polder grid: {len(u)} points, u0 = {u0:10.6f}"]
    for k in range(len(u)):
        lines.append(f"    point{k + 1:3d}   u {u[k]:18.10f}   weight {weights[k]:18.10f}   mean(iu) {np.real(iso[k]):18.10f}")
    lines.append(f"  C6 (homo-dimer) = {c6_coefficient(iso, iso, weights):18.10f}")
    lines.append(f"  C6 response sigma builds: {info['nsigma']}   largest residual: {float(np.max(info['resnorm'])):11.3e}")
    return "\n".join(lines)


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
