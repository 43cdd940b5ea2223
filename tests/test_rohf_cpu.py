"""CPU checks of the restricted open-shell path: the numpy restatement (np_rocc) against np_ucc, FCI and its own invariances,
afesp_amd.rohf.semicanonical against the restatement's, and what the built library exports."""
import ctypes
import dataclasses

import numpy as np
import pytest

import molecules
import np_rocc
import np_ucc
from afesp_amd import capi, fcidump, inputs, rohf, uhf


@pytest.fixture(scope="module")
def water():
    si, ints, res, _ = molecules.load("h2o-cc-pvdz")
    return si, ints, res


@pytest.fixture(scope="module")
def cation(water):
    """H2O+ (5, 4), canonical UHF orbitals: blocks, the converged restatement of np_ucc and its (T)"""
    si, ints, _ = water
    si = dataclasses.replace(si, charge=1, multiplicity=2, scf_maxiter=200, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_read_guess=False)
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    u = uhf.do_uhf(si, ints, na, nb)
    assert u.converged and (na, nb) == (5, 4)
    aa, ab, bb = np_ucc.mo_blocks(n, u.coeff_a, u.coeff_b, ints.eri)
    cc = np_ucc.UCC(*np_ucc.so_integrals(aa, ab, bb, u.levels_a, u.levels_b, na, nb))
    it, e = cc.solve(60, 1e-11, 1e-11)
    return dict(n=n, na=na, nb=nb, u=u, blocks=(aa, ab, bb), e=e, e_t=cc.triples())


def test_diagonal_fock_reproduces_np_ucc_iteration_by_iteration(cation):
    c, u = cation, cation["u"]
    aa, ab, bb = c["blocks"]
    ref = np_ucc.UCC(*np_ucc.so_integrals(aa, ab, bb, u.levels_a, u.levels_b, c["na"], c["nb"]))
    cc = np_rocc.rocc_from_blocks(aa, ab, bb, np.diag(u.levels_a), np.diag(u.levels_b), c["na"], c["nb"])
    assert abs(cc.e_mp2() - np_ucc.ump2(aa, ab, bb, u.levels_a, u.levels_b, c["na"], c["nb"])) < 1e-13
    a, b = cc.energy_step(), ref.energy_step()
    assert abs(a[0] - b[0]) < 1e-13 and abs(a[1] - b[1]) < 1e-13
    for it in range(4):
        cc.iterate()
        ref.iterate()
        a, b = cc.energy_step(), ref.energy_step()
        assert abs(a[0] - b[0]) < 1e-13 and abs(a[1] - b[1]) < 1e-13, it
    assert abs(cc.triples() - ref.triples()) < 1e-13


def test_two_electron_triplet_with_f_ov_is_fci(water):
    si, ints, _ = water
    si = dataclasses.replace(si, charge=8, multiplicity=3, scf_maxiter=200, scf_e_tol=1e-12, scf_d_tol=1e-10)
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    assert (na, nb) == (2, 0)
    u = uhf.do_uhf(si, ints, na, nb)
    C = np_rocc.triplet_rotation(n, 0.05) @ u.coeff_a      # angle 0.05: see np_rocc.triplet_rotation
    aa, ab, bb = np_ucc.mo_blocks(n, C, C, ints.eri)
    h = C @ ints.core_hamil @ C.T
    fa, fb = np_rocc.fock_ro(h, aa, na, nb)
    assert np.max(np.abs(fa[:na, na:])) > 1.0             # f_ov is no small perturbation here
    cc = np_rocc.rocc_from_blocks(aa, ab, bb, fa, fb, na, nb)
    it, e = cc.solve(60, 1e-11, 1e-11)                    # (raises beyond 60 iterations)
    assert it <= 20
    assert abs(np_rocc.e_ref_elec(h, fa, fb, na, nb) + e - np_ucc.fci_two_electron(n, aa, ab, h, h, True)) < 1e-9


def test_ccsd_is_invariant_and_semicanonical_orbitals_give_back_the_canonical_results(cation, water):
    _, ints, _ = water
    c, u, n, na, nb = cation, cation["u"], cation["n"], cation["na"], cation["nb"]
    ra, rb = np_rocc.invariance_rotations(n, na, nb)       # seed 7, size 1e-3: see np_rocc.invariance_rotations
    fa, fb = ra @ np.diag(u.levels_a) @ ra.T, rb @ np.diag(u.levels_b) @ rb.T
    cc = np_rocc.rocc_from_blocks(*np_ucc.mo_blocks(n, ra @ u.coeff_a, rb @ u.coeff_b, ints.eri), fa, fb, na, nb)
    assert np.max(np.abs(cc.f_oo)) > 1e-2 and np.max(np.abs(cc.f_vv)) > 1e-3
    it, e = cc.solve(60, 1e-11, 1e-11, diis=20)
    assert abs(e - c["e"]) < 1e-9
    ua, ub, ga, gb = np_rocc.semicanonical(fa, fb, na, nb)
    assert np.max(np.abs(np.diag(ga) - u.levels_a)) < 1e-9 and np.max(np.abs(np.diag(gb) - u.levels_b)) < 1e-9
    sc = np_rocc.rocc_from_blocks(*np_ucc.mo_blocks(n, ua @ ra @ u.coeff_a, ub @ rb @ u.coeff_b, ints.eri), ga, gb, na, nb)
    it, e = sc.solve(60, 1e-11, 1e-11)
    assert abs(e - c["e"]) < 1e-9 and abs(sc.triples() - c["e_t"]) < 1e-9
    # the package's semicanonical is the restatement's
    pa, pb, qa, qb = rohf.semicanonical(fa, fb, na, nb)
    for x, y in ((pa, ua), (pb, ub), (qa, ga), (qb, gb)):
        assert np.max(np.abs(x - y)) < 1e-13
    assert np.array_equal(qa, qa.T) and not np.any(qa[:na, :na] - np.diag(np.diag(qa)[:na]))


def test_library_exports_and_declarations():
    names = ("afesp_mo_fock_ro", "afesp_read_fcidump_rohf", "afesp_mo_rotate_uhf", "afesp_ccsd_uso_init_fock")
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in names:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS
        assert getattr(capi.load_library(), s).argtypes is not None, s
    for m in ("mo_fock_ro", "read_fcidump_rohf", "mo_rotate_uhf", "uso_init_fock"):
        assert callable(getattr(capi.Engine, m))


def test_scan_reports_a_restricted_doublet(tmp_path):
    rng = np.random.default_rng(3)
    n = 4
    h = rng.standard_normal((n, n))
    path = tmp_path / "doublet.fcidump"
    nl = fcidump.write(path, h + h.T, rng.standard_normal(inputs.neri(n)), 3, 1, 0.25)
    hd = capi.scan_fcidump(path)
    assert (hd.norb, hd.nelec, hd.ms2, hd.uhf, hd.nlines) == (n, 3, 1, False, nl)
    rec = fcidump.read(path)
    assert rec.ms2 == 1 and not rec.uhf and rec.ecore == 0.25 and np.array_equal(rec.h, h + h.T)
