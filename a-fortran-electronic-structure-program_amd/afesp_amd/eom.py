"""EOM-EE-CCSD excitation energies of a spin-orbital CCSD state: the Davidson driver over Engine.so_eom_* and the labelling of a root
(host code).

The spin-orbital space holds every Ms component: a triplet appears threefold (Ms = 0 and the two spin-flip components Ms = +-1), a singlet
once.  The driver reports the degeneracies and filters nothing."""
from __future__ import annotations

import numpy as np

from .capi import AfespError
from .density import so_spin_order

HARTREE_EV = 27.211386245988
FLAG_CONVERGED, FLAG_COMPLEX = 1, 2


def default_max_space(nroots, nunique):
    """eight vectors per root, at least 2 nroots (what the library asks for)"""
    return max(2 * nroots, min(int(nunique), 8 * nroots))


def so_eom_solve(eng, nroots, tol=1e-8, max_space=None, maxiter=100, guesses=None):
    """The nroots lowest EOM-EE-CCSD excitation energies of the engine's spin-orbital state at its current (converged) amplitudes.
    A live Lambda state is needed for its H-bar elements (eng.so_lambda_init, or density.so_lambda_solve); Lambda need not be converged.
    guesses: [(r1, r2)] instead of the unit vectors on the smallest orbital-energy differences.
    -> (omega [nroots], [(x1, x2)] with <x, x> = 1, info) -- info: iterations, nsigma, resnorm, flags, r1_norm2 (sum x1^2 per root: the
    singles weight), complex (roots whose projected value had an imaginary part), degeneracy (roots within 1e-6 Eh of each one).
    Raises AfespError if maxiter steps do not converge."""
    if maxiter < 1:
        raise ValueError("so_eom_solve: maxiter must be at least 1")
    o, v = eng.so_o, eng.so_v
    nunique = o * v + (o * (o - 1) // 2) * (v * (v - 1) // 2)
    if max_space is None:
        max_space = default_max_space(nroots, nunique)
    eng.so_eom_init(nroots, max_space)
    if guesses is None:
        eng.so_eom_guess()
    else:
        for k, (r1, r2) in enumerate(guesses):
            eng.so_eom_set_guess(k, r1, r2)
    for it in range(1, maxiter + 1):
        omega, res, flags, nsigma, conv = eng.so_eom_iterate(tol)
        if conv:
            vectors = [eng.so_eom_vector(k) for k in range(nroots)]
            info = dict(iterations=it, nsigma=nsigma, resnorm=res, flags=flags, max_space=max_space,
                        r1_norm2=np.array([float(np.sum(x1 * x1)) for x1, _ in vectors]),
                        complex=[k for k in range(nroots) if flags[k] & FLAG_COMPLEX],
                        degeneracy=np.array([int(np.sum(np.abs(omega - w) < 1e-6)) for w in omega]))
            return omega, vectors, info
    raise AfespError(f"the EOM-CCSD Davidson iteration did not converge in {maxiter} steps (residuals {res})")


def label_root(x1, x2, nbasis, nalpha, nbeta, interleaved):
    """The dominant amplitude of a root and its spin change: -> dict(kind "single" / "double", occ, virt (spatial orbital indices),
    spins_occ, spins_virt (0 alpha, 1 beta), delta_ms, weight).  delta_ms = Ms(excited) - Ms(reference): 0 for spin-conserving
    amplitudes, +-1 for the spin-flip components of a triplet."""
    orb, spin = so_spin_order(nbasis, nalpha, nbeta, interleaved)
    o = nalpha + nbeta
    x1, x2 = np.asarray(x1), np.asarray(x2)
    ms = lambda s: 0.5 - s
    i1 = np.unravel_index(np.argmax(np.abs(x1)), x1.shape)
    i2 = np.unravel_index(np.argmax(np.abs(x2)), x2.shape) if x2.size else None
    if i2 is None or abs(x1[i1]) >= abs(x2[i2]):
        i, a = int(i1[0]), int(i1[1]) + o
        return dict(kind="single", occ=(int(orb[i]),), virt=(int(orb[a]),), spins_occ=(int(spin[i]),), spins_virt=(int(spin[a]),),
                    delta_ms=float(ms(spin[a]) - ms(spin[i])), weight=float(x1[i1] ** 2))
    i, j, a, b = int(i2[0]), int(i2[1]), int(i2[2]) + o, int(i2[3]) + o
    return dict(kind="double", occ=(int(orb[i]), int(orb[j])), virt=(int(orb[a]), int(orb[b])), spins_occ=(int(spin[i]), int(spin[j])),
                spins_virt=(int(spin[a]), int(spin[b])), delta_ms=float(ms(spin[a]) + ms(spin[b]) - ms(spin[i]) - ms(spin[j])),
                weight=float(x2[i2] ** 2))


def table(omega, info):
    """The lines the Fortran host prints: root, omega in Eh and eV, |r1|^2, residual, sigma builds"""
    lines = ["  root        omega / Eh        omega / eV     |r1|^2     residual"]
    for k, w in enumerate(omega):
        lines.append(f"  {k + 1:4d}  {w:16.10f}  {w * HARTREE_EV:16.8f}  {info['r1_norm2'][k]:9.6f}  {info['resnorm'][k]:11.3e}")
    lines.append(f"  sigma builds: {info['nsigma']}")
    return "\n".join(lines)
