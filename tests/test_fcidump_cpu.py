"""The FCIDUMP reader and its numpy checks (afesp_amd/fcidump.py), and the numpy restatement of the frozen-core operator the GPU tests
rest on (np_fcidump.py).  No GPU."""
import dataclasses

import numpy as np
import pytest

import molecules
import np_fcidump
import np_ucc
import np_window
import orc
from afesp_amd import fcidump, inputs, rhf, uhf


def _sym(rng, n):
    a = rng.standard_normal((n, n))
    return 0.5 * (a + a.T)


def test_closed_shell_dump_written_by_hand_round_trips(tmp_path):
    n, rng = 4, np.random.default_rng(5)
    eri, h = rng.standard_normal(inputs.neri(n)), _sym(rng, n)
    eri[[3, 17]] = 0.0                                    # exact zeros are not written and read back as zeros
    path = tmp_path / "FCIDUMP"
    path.write_text(np_fcidump.dump_text(n, 4, 0, eri, h, -1.25))
    rec = fcidump.read(path)
    assert (rec.norb, rec.nelec, rec.ms2, rec.uhf) == (n, 4, 0, False)
    assert rec.nlines == inputs.neri(n) - 2 + n * (n + 1) // 2 + 1
    # 16 significant digits are written: one unit in the 16th at most
    assert np.max(np.abs(rec.eri - eri)) < 1e-15 * np.max(np.abs(eri)) * 10 and np.array_equal(rec.eri == 0.0, eri == 0.0)
    assert np.max(np.abs(rec.h - h)) < 1e-14 and np.array_equal(rec.h, rec.h.T) and rec.ecore == -1.25
    assert rec.h_a is None and rec.eri_ab is None


def test_open_shell_dump_written_by_hand_round_trips(tmp_path):
    n, na, nb, rng = 3, 2, 1, np.random.default_rng(6)
    aa, bb = rng.standard_normal(inputs.neri(n)), rng.standard_normal(inputs.neri(n))
    ab = rng.standard_normal((inputs.npair(n), inputs.npair(n)))
    ha, hb = _sym(rng, n), _sym(rng, n)
    path = tmp_path / "FCIDUMP"
    text = np_fcidump.udump_text(n, na, nb, aa, ab, bb, ha, hb, 0.5)
    path.write_text(text)
    assert "UHF=.TRUE." in text.split("&END")[0] and "NORB=6,NELEC=3,MS2=1," in text
    rec = fcidump.read(path)
    assert (rec.norb, rec.nelec, rec.ms2, rec.uhf, rec.nspatial, rec.nalpha, rec.nbeta) == (6, 3, 1, True, 3, 2, 1)
    for got, ref in ((rec.eri_aa, aa), (rec.eri_bb, bb), (rec.eri_ab, ab), (rec.h_a, ha), (rec.h_b, hb)):
        assert got.shape == ref.shape and np.max(np.abs(got - ref)) < 1e-14
    assert rec.ecore == 0.5 and rec.h is None and rec.eri is None
    # spatial orbital p is spin orbital 2p - 1 (alpha) / 2p (beta): the first alpha-beta line is (1 1 | 2 2)
    body = text.split("&END\n")[1].splitlines()
    first_ab = body[2 * inputs.neri(n)].split()
    assert first_ab[1:] == ["1", "1", "2", "2"] and float(first_ab[0]) == pytest.approx(ab[0, 0], rel=1e-15)
    # a spin-forbidden integral is refused
    path.write_text(text.replace(body[0], np_fcidump.line(1.0, 1, 2, 1, 1).rstrip("\n"), 1))
    with pytest.raises(ValueError, match="spin-forbidden"):
        fcidump.read(path)


def test_core_operator_restatement_equals_the_brute_force_sum():
    """np_fcidump.core_operator / ucore_operator (index arithmetic on the packed arrays) against loops over the unpacked four-index
    arrays: n = 6, nfc = 2, nfv = 1.  Sums of <= 3 nfc products of O(1) numbers: 1e-13."""
    n, nfc, nfv, rng = 6, 2, 1, np.random.default_rng(7)
    hi = n - nfv
    packed, h = rng.standard_normal(inputs.neri(n)), _sym(rng, n)
    g = rhf.unpack_eri(n, packed)
    ref_h, ref_e = np.zeros((hi - nfc, hi - nfc)), 0.0
    for p in range(nfc, hi):
        for q in range(nfc, hi):
            ref_h[p - nfc, q - nfc] = h[p, q] + sum(2.0 * g[p, q, c, c] - g[p, c, q, c] for c in range(nfc))
    for c in range(nfc):
        ref_e += 2.0 * h[c, c] + sum(2.0 * g[c, c, d, d] - g[c, d, c, d] for d in range(nfc))
    got_h, got_e = np_fcidump.core_operator(n, nfc, nfv, h, packed)
    assert np.max(np.abs(got_h - ref_h)) < 1e-13 and abs(got_e - ref_e) < 1e-13
    h0, e0 = np_fcidump.core_operator(n, 0, nfv, h, packed)
    assert np.array_equal(h0, h[:hi, :hi]) and e0 == 0.0
    # open shell: three independent blocks
    bb, hb = rng.standard_normal(inputs.neri(n)), _sym(rng, n)
    ab = rng.standard_normal((inputs.npair(n), inputs.npair(n)))
    gb, gab = rhf.unpack_eri(n, bb), np_ucc.unpair_matrix(n, ab)
    ra, rb, re = np.zeros_like(ref_h), np.zeros_like(ref_h), 0.0
    for p in range(nfc, hi):
        for q in range(nfc, hi):
            ra[p - nfc, q - nfc] = h[p, q] + sum(g[p, q, c, c] - g[p, c, q, c] + gab[p, q, c, c] for c in range(nfc))
            rb[p - nfc, q - nfc] = hb[p, q] + sum(gb[p, q, c, c] - gb[p, c, q, c] + gab[c, c, p, q] for c in range(nfc))
    for c in range(nfc):
        re += h[c, c] + hb[c, c] + sum(0.5 * (g[c, c, d, d] - g[c, d, c, d]) + 0.5 * (gb[c, c, d, d] - gb[c, d, c, d]) + gab[c, c, d, d]
                                       for d in range(nfc))
    ga, gb_, ge = np_fcidump.ucore_operator(n, nfc, nfv, h, hb, packed, ab, bb)
    assert np.max(np.abs(ga - ra)) < 1e-13 and np.max(np.abs(gb_ - rb)) < 1e-13 and abs(ge - re) < 1e-13
    # equal blocks: the closed-shell operator
    pm = np_ucc.pair_matrix(g)
    ca, cb, ce = np_fcidump.ucore_operator(n, nfc, nfv, h, h, packed, pm, packed)
    assert np.max(np.abs(ca - got_h)) < 1e-13 and np.max(np.abs(cb - got_h)) < 1e-13 and abs(ce - got_e) < 1e-13


@pytest.fixture(scope="module")
def water():
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, scf_e_tol=1e-13, scf_d_tol=1e-11, scf_maxiter=300, scf_read_guess=False)
    res = rhf.do_rhf(si, ints)
    assert res.converged
    return si, ints, res


@pytest.mark.parametrize("nfc,nfv", [(1, 0), (0, 0), (1, 3)])
def test_a_frozen_core_dump_is_the_hamiltonian_of_the_scf(water, tmp_path, nfc, nfv):
    """H2O/cc-pVDZ through the oracle's transform, the numpy core operator, the window and the hand writer: the file's determinant energy
    is the SCF total energy, its Fock diagonal the orbital energies of the window, its MP2 energy the oracle's on the window."""
    _, ints, res = water
    n, o = ints.nbasis, ints.nel // 2
    mo = orc.ao2mo(n, res.canon_coeff, ints.eri)
    h_act, e_core = np_fcidump.core_operator(n, nfc, nfv, res.canon_coeff @ ints.core_hamil @ res.canon_coeff.T, mo)
    win, lev = np_window.window_packed(n, nfc, nfv, mo), np_window.window_levels(n, nfc, nfv, res.canon_levels)
    path = tmp_path / "FCIDUMP"
    path.write_text(np_fcidump.dump_text(n - nfc - nfv, ints.nel - 2 * nfc, 0, win, h_act, e_core + ints.e_nuc))
    rec = fcidump.read(path)
    gap = abs(fcidump.hf_energy(rec) - (res.e_hf + ints.e_nuc))
    print(f"nfc={nfc} nfv={nfv}: E(HF) gap {gap:.2e}, levels {np.max(np.abs(fcidump.fock_diagonal(rec) - lev)):.2e}")
    assert gap < 1e-9
    assert np.max(np.abs(fcidump.fock_diagonal(rec) - lev)) < 1e-9
    assert abs(fcidump.mp2_energy(rec) - orc.mp2_energy(n - nfc - nfv, o - nfc, win, lev)) < 1e-10


def test_an_open_shell_dump_is_the_hamiltonian_of_the_uhf(tmp_path):
    """H2O+ (doublet), nfc = 1, nfv = 2, all in numpy: E(UHF), both spins' levels and E(UMP2) from the file"""
    nfc, nfv = 1, 2
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, charge=1, multiplicity=2, scf_maxiter=300, scf_e_tol=1e-13, scf_d_tol=1e-11, scf_read_guess=False)
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    u = uhf.do_uhf(si, ints, na, nb)
    assert u.converged
    faa, fab, fbb = np_ucc.mo_blocks(n, u.coeff_a, u.coeff_b, ints.eri)
    ha, hb, e_core = np_fcidump.ucore_operator(n, nfc, nfv, u.coeff_a @ ints.core_hamil @ u.coeff_a.T, u.coeff_b @ ints.core_hamil @ u.coeff_b.T,
                                               np_ucc.pack8(faa), np_ucc.pair_matrix(fab), np_ucc.pack8(fbb))
    waa, wab, wbb = (np_window.window_full(nfc, nfv, x) for x in (faa, fab, fbb))
    la, lb = u.levels_a[nfc:n - nfv], u.levels_b[nfc:n - nfv]
    path = tmp_path / "FCIDUMP"
    path.write_text(np_fcidump.udump_text(n - nfc - nfv, na - nfc, nb - nfc, np_ucc.pack8(waa), np_ucc.pair_matrix(wab), np_ucc.pack8(wbb), ha, hb,
                                          e_core + ints.e_nuc))
    rec = fcidump.read(path)
    fa, fb = fcidump.fock_diagonal(rec)
    assert abs(fcidump.hf_energy(rec) - (u.e_hf + ints.e_nuc)) < 1e-9
    assert np.max(np.abs(fa - la)) < 1e-9 and np.max(np.abs(fb - lb)) < 1e-9
    assert abs(fcidump.mp2_energy(rec) - np_ucc.ump2(waa, wab, wbb, la, lb, na - nfc, nb - nfc)) < 1e-10


def test_the_new_namelist_key_is_read_and_excludes_the_old_dump(tmp_path):
    base = open(molecules.GOLDEN + "/h2o-cc-pvdz/els.in").read()
    (tmp_path / "a.in").write_text(base.rstrip()[:-1] + "fcidump_active = .true.,\n/\n")
    assert inputs.read_els_in(str(tmp_path / "a.in")).fcidump_active is True
    assert inputs.read_els_in(molecules.GOLDEN + "/h2o-cc-pvdz/els.in").fcidump_active is False
    (tmp_path / "b.in").write_text(base.replace("write_fcidump = .false.", "write_fcidump = .true.").rstrip()[:-1] + "fcidump_active = .true.,\n/\n")
    with pytest.raises(ValueError, match="both write FCIDUMP"):
        inputs.read_els_in(str(tmp_path / "b.in"))


def test_the_four_calls_are_bound_everywhere():
    import os
    from afesp_amd import capi
    names = ["afesp_core_operator", "afesp_ucore_operator", "afesp_write_fcidump_active", "afesp_write_fcidump_uactive"]
    root = os.path.dirname(os.path.dirname(molecules.GOLDEN))
    header = open(os.path.join(root, "include", "afesp.h")).read()
    f90 = open(os.path.join(root, "a-fortran-electronic-structure-program_amd", "host", "afesp_capi.f90")).read()
    for name in names:
        assert name in capi.EXPORTS and f"int {name}(" in header and f"bind(C, name='{name}')" in f90
