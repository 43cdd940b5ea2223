"""Unrestricted Hartree-Fock, host side (numpy), in the style of rhf.py: the same start (core Hamiltonian, or the guess_in.dat
Fock matrix for both spins), the same orthogonaliser, energy and convergence tests, and DIIS on the concatenated error vectors
F_s D_s S - S D_s F_s of the two spins with one set of coefficients.  The reference has no UHF (src/main.F90:48-52 runs its
spin-orbital methods on doubled RHF orbitals); this produces the canonical UHF orbitals the open-shell path starts from.

Densities follow rhf.py: D_s = C_s,occ^T C_s,occ (C: MO x AO), so that with D_a = D_b = D every step is the RHF one.  Nothing
mixes the two spins: a symmetric start at multiplicity 1 stays on the RHF solution.
"""
from __future__ import annotations

import dataclasses
from typing import Callable

import numpy as np

from .inputs import Integrals, SystemIn
from .rhf import unpack_eri


@dataclasses.dataclass
class UHFResult:
    converged: bool
    e_hf: float                 # electronic energy (no nuclear repulsion)
    coeff_a: np.ndarray         # (MO, AO)
    coeff_b: np.ndarray
    levels_a: np.ndarray
    levels_b: np.ndarray
    fock_a: np.ndarray
    fock_b: np.ndarray
    s2: float                   # <S^2> of the UHF determinant
    iters: list


def numpy_fock_builder(ints: Integrals) -> Callable:
    """F_s = H + J[D_a + D_b] - K[D_s] from the unpacked AO integrals (the host counterpart of Engine.build_fock_uhf)."""
    V = unpack_eri(ints.nbasis, ints.eri)
    H = ints.core_hamil

    def build(da, db):
        J = np.einsum("ijkl,kl->ij", V, da + db)
        return H + J - np.einsum("ikjl,kl->ij", V, da), H + J - np.einsum("ikjl,kl->ij", V, db)
    return build


def spin_contamination(coeff_a, coeff_b, S, na, nb) -> float:
    """<S^2> = Sz (Sz + 1) + n_b - sum_ij |<i_a|j_b>|^2 over the occupied orbitals."""
    sz = 0.5 * (na - nb)
    ov = coeff_a[:na] @ S @ coeff_b[:nb].T
    return float(sz * (sz + 1.0) + nb - np.sum(ov * ov))


def do_uhf(sysin: SystemIn, ints: Integrals, nalpha: int, nbeta: int, scf_guess: np.ndarray | None = None,
           fock_builder: Callable | None = None) -> UHFResult:
    n = ints.nbasis
    S, H = ints.ovlp, ints.core_hamil
    build = fock_builder or numpy_fock_builder(ints)
    s, U = np.linalg.eigh(S)
    X = U @ np.diag(1.0 / np.sqrt(s)) @ U.T
    start = scf_guess if (sysin.scf_read_guess and scf_guess is not None) else H
    fa, fb = start.copy(), start.copy()
    nerr = sysin.scf_diis_n_errmat
    use_diis = nerr >= 2
    dF = np.zeros((nerr, 2, n, n)) if use_diis else None
    dE = np.zeros((nerr, 2, n, n)) if use_diis else None
    d_iter = d_active = 0
    energy = 0.0
    da_old, db_old = np.zeros((n, n)), np.zeros((n, n))
    iters = []
    for it in range(1, sysin.scf_maxiter + 1):
        wa, Aa = np.linalg.eigh(X.T @ fa @ X)
        wb, Ab = np.linalg.eigh(X.T @ fb @ X)
        Ca, Cb = (X @ Aa).T, (X @ Ab).T
        da, db = Ca[:nalpha].T @ Ca[:nalpha], Cb[:nbeta].T @ Cb[:nbeta]
        energy_old, energy = energy, float(0.5 * (np.sum(da * (H + fa)) + np.sum(db * (H + fb))))
        # (the mean of the two spins' squared changes: the RHF measure when D_a = D_b)
        rms = float(np.sqrt(0.5 * (np.sum((da - da_old) ** 2) + np.sum((db - db_old) ** 2))))
        da_old, db_old = da, db
        iters.append((it, energy, energy - energy_old, rms))
        if rms < sysin.scf_d_tol and abs(energy - energy_old) < sysin.scf_e_tol:
            return UHFResult(True, energy, Ca, Cb, wa, wb, fa, fb, spin_contamination(Ca, Cb, S, nalpha, nbeta), iters)
        fa, fb = build(da, db)
        if use_diis:
            d_iter += 1
            if d_iter > nerr:
                d_iter -= nerr
            if d_active < nerr:
                d_active += 1
            dF[d_iter - 1] = (fa, fb)
            dE[d_iter - 1] = (fa @ da @ S - S @ da @ fa, fb @ db @ S - S @ db @ fb)
            m = d_active
            if m > 1:
                B = np.zeros((m + 1, m + 1))
                B[:m, :m] = np.einsum("isab,jsab->ij", dE[:m], dE[:m])
                B[m, :m] = B[:m, m] = -1.0
                rhs = np.zeros(m + 1)
                rhs[m] = -1.0
                c = np.linalg.solve(B, rhs)
                fa = np.einsum("i,iab->ab", c[:m], dF[:m, 0])
                fb = np.einsum("i,iab->ab", c[:m], dF[:m, 1])
    return UHFResult(False, energy, Ca, Cb, wa, wb, fa, fb, spin_contamination(Ca, Cb, S, nalpha, nbeta), iters)
