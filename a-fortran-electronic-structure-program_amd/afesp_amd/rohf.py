"""Restricted open-shell (ROHF) references on the dense spin-orbital solver: semicanonical orbitals and the driver that strings the
engine's calls together.  No ROHF SCF: the orbitals come from a restricted FCIDUMP (MS2 >= 0, no UHF flag) or from the
caller.

A restricted open-shell determinant has two spin Fock operators F_a, F_b over ONE set of orbitals; neither is diagonal.  ROHF-MBPT(2) and
ROHF-CCSD(T) (Watts, Gauss, Bartlett, J. Chem. Phys. 98, 8718 (1993)) are defined in the semicanonical orbitals that diagonalise the
occupied-occupied and the virtual-virtual block of each spin separately; f_ia stays and enters the equations."""
from __future__ import annotations

import dataclasses

import numpy as np

from .capi import AfespError


def _block_rotation(f, o):
    """u[new, old] that diagonalises f[:o, :o] and f[o:, o:] (rising levels; each new orbital's largest component is positive)."""
    n = f.shape[0]
    u = np.zeros((n, n))
    for lo, hi in ((0, o), (o, n)):
        if hi > lo:
            _, vec = np.linalg.eigh(0.5 * (f[lo:hi, lo:hi] + f[lo:hi, lo:hi].T))
            big = np.argmax(np.abs(vec), axis=0)
            vec = vec * np.where(vec[big, np.arange(hi - lo)] < 0.0, -1.0, 1.0)[None, :]
            u[lo:hi, lo:hi] = vec.T
    return u


def semicanonical(fock_a, fock_b, nalpha, nbeta):
    """-> (u_a, u_b, fock_a', fock_b'): u_s[new orbital, old orbital] diagonalises the occupied and the virtual block of fock_s; fock_s' =
    u_s fock_s u_s^T, symmetric to the bit, with those two blocks diagonal to the bit (what the rotation leaves there is rounding)."""
    out = []
    for f, o in ((np.asarray(fock_a, dtype=np.float64), int(nalpha)), (np.asarray(fock_b, dtype=np.float64), int(nbeta))):
        n = f.shape[0]
        u = _block_rotation(f, o)
        g = u @ f @ u.T
        g = 0.5 * (g + g.T)
        for lo, hi in ((0, o), (o, n)):
            d = np.diag(g)[lo:hi].copy()
            g[lo:hi, lo:hi] = np.diag(d)
        out.append((u, g))
    return out[0][0], out[1][0], out[0][1], out[1][1]


@dataclasses.dataclass
class RohfCC:
    nbasis: int
    nalpha: int
    nbeta: int
    e_core: float
    e_ref: float                 # the determinant's energy as the file gives it (core energy included)
    fock_offdiag: tuple          # max |F|: occupied-occupied off-diagonal, virtual-virtual off-diagonal, occupied-virtual
    e_mp2: float                 # ROHF-MBPT(2)
    niter: int
    energies: np.ndarray         # the iteration table (first entry: the start amplitudes)
    rms: np.ndarray
    e_ccsd: float
    e_t: float | None


def rohf_cc(engine, path, maxiter=50, e_tol=1e-6, t_tol=1e-7, triples=True, diis_nerr=8) -> RohfCC:
    """ROHF-MBPT(2), ROHF-CCSD and (with triples) ROHF-CCSD(T) of a restricted FCIDUMP: reader -> semicanonical orbitals -> rotation of the
    resident integrals -> the spin-orbital solver with the full Fock matrix -> (T).  Raises AfespError where CCSD does not converge."""
    rec = engine.read_fcidump_rohf(path)
    n, na, nb = rec.norb, rec.nalpha, rec.nbeta
    u_a, u_b, f_a, f_b = semicanonical(rec.fock_a, rec.fock_b, na, nb)
    engine.mo_rotate_uhf(n, u_a, u_b)
    e_mp2 = engine.uso_init_fock(n, na, nb, f_a, f_b, diis_nerr)
    nit, en, rm = engine.do_ccsd_spinorb(maxiter, e_tol, t_tol)
    if nit < 0:   # no CCSD energy to report, and no amplitudes (T) could be evaluated on
        raise AfespError(f"status 1: rohf_cc: ROHF-CCSD did not converge within {maxiter} iterations (last energy {en[-1]:.12f})")
    e_t = engine.do_ccsd_t_spinorb() if triples else None
    return RohfCC(n, na, nb, rec.e_core, rec.e_ref, rec.fock_offdiag3, e_mp2, nit, en, rm, float(en[-1]), e_t)
