"""The active space as a standard FCIDUMP on the GPU: afesp_core_operator / afesp_ucore_operator against the numpy restatement
(np_fcidump.py), the files of afesp_write_fcidump_active / _uactive read back as Hamiltonians (afesp_amd/fcidump.py), the stream
compaction against numpy's selection, and the refusals."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import molecules
import np_fcidump
from afesp_amd import capi, fcidump, inputs, rhf, uhf
from test_gpu_frozen import _random_system, _v_oovv

pytestmark = pytest.mark.gpu
TIGHT = dict(scf_e_tol=1e-13, scf_d_tol=1e-11, scf_maxiter=300, scf_read_guess=False)


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _sym(rng, n):
    a = rng.standard_normal((n, n))
    return 0.5 * (a + a.T)


@pytest.mark.parametrize("n,nfc,nfv", [(24, 1, 0), (28, 2, 3), (28, 0, 5), (100, 3, 5)])
def test_core_operator_matches_numpy(eng, n, nfc, nfv):
    """h_act and e_core against np_fcidump.core_operator on the packed array the transform itself returned: 1e-11 of the largest element
    (a sum of <= 3 nfc products in a fixed order); h_act symmetric to the bit.  n = 100: the array the LDS-DMA transform wrote."""
    o = nfc + 3
    eri, c, e = _random_system(n, o, 17 * n + nfc)
    h_ao = _sym(np.random.default_rng(n + nfv), n)
    before = eng.launch_counts()
    _, full = eng.do_mp2_spatial(n, o, c, e, eri)
    after = eng.launch_counts()
    if n == 100:
        assert after["tgemm"] + after["tgemm_mixed"] > before["tgemm"] + before["tgemm_mixed"], (before, after)
    h_act, e_core = eng.core_operator(n, nfc, nfv, c, h_ao)
    ref_h, ref_e = np_fcidump.core_operator(n, nfc, nfv, c @ h_ao @ c.T, full)
    scale = np.max(np.abs(ref_h))
    print(f"n={n} nfc={nfc} nfv={nfv}: h_act {np.max(np.abs(h_act - ref_h)) / scale:.2e} e_core {abs(e_core - ref_e) / scale:.2e} of {scale:.3f}")
    assert h_act.shape == ref_h.shape and np.array_equal(h_act, h_act.T)
    assert np.max(np.abs(h_act - ref_h)) < 1e-11 * scale and abs(e_core - ref_e) < 1e-11 * scale
    if nfc == 0:
        assert e_core == 0.0
    if n < 100:   # nothing resident was written: the transform's array is still what ccsd_init reads
        eng.ccsd_init(o, n - o, e, None, 4)
        assert np.array_equal(eng.tensor("v_oovv"), _v_oovv(o, n - o, full))


def test_open_shell_core_operator_matches_numpy_and_the_closed_shell_limit(eng):
    n, na, nb, nfc, nfv = 20, 5, 3, 1, 2
    rng = np.random.default_rng(99)
    eri, ca, la = _random_system(n, na, 5)
    _, cb, lb = _random_system(n, nb, 6)
    h_ao = _sym(rng, n)
    _, aa, ab, bb = eng.do_ump2(n, na, nb, ca, cb, la, lb, eri)
    ha, hb, e_core = eng.ucore_operator(n, nfc, nfv, ca, cb, h_ao)
    ra, rb, re = np_fcidump.ucore_operator(n, nfc, nfv, ca @ h_ao @ ca.T, cb @ h_ao @ cb.T, aa, ab, bb)
    scale = max(np.max(np.abs(ra)), np.max(np.abs(rb)))
    print(f"open shell: h_a {np.max(np.abs(ha - ra)) / scale:.2e} h_b {np.max(np.abs(hb - rb)) / scale:.2e} e_core {abs(e_core - re) / scale:.2e}")
    assert np.array_equal(ha, ha.T) and np.array_equal(hb, hb.T)
    assert np.max(np.abs(ha - ra)) < 1e-11 * scale and np.max(np.abs(hb - rb)) < 1e-11 * scale and abs(e_core - re) < 1e-11 * scale
    # nalpha = nbeta with equal coefficients: both operators are the closed-shell one
    eng.do_ump2(n, na, na, ca, ca, la, la, eri, want_eri_mo=False)
    ua, ub, ue = eng.ucore_operator(n, nfc, nfv, ca, ca, h_ao)
    eng.do_mp2_spatial(n, na, ca, la, eri, want_eri_mo=False)
    h, e = eng.core_operator(n, nfc, nfv, ca, h_ao)
    print(f"closed-shell limit: {np.max(np.abs(ua - h)):.2e} {np.max(np.abs(ub - h)):.2e} {abs(ue - e):.2e}")
    assert np.max(np.abs(ua - h)) < 1e-12 and np.max(np.abs(ub - h)) < 1e-12 and abs(ue - e) < 1e-12


@pytest.fixture(scope="module")
def water():
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    res = rhf.do_rhf(dataclasses.replace(si, **TIGHT), ints)
    assert res.converged
    return ints, res


@pytest.mark.parametrize("nfc,windowed", [(1, True), (0, False)])
def test_closed_shell_dump_is_the_hamiltonian(eng, water, tmp_path, nfc, windowed):
    """H2O/cc-pVDZ: the file's determinant energy is the SCF total energy (1e-9: what the SCF convergence leaves), its Fock diagonal the
    levels of the window (1e-9), its MP2 energy the one the window call reported (1e-10).  Holds only if the core operator, the window,
    the writer and the numbering are all right."""
    ints, res = water
    n, o, lev = ints.nbasis, ints.nel // 2, res.canon_levels
    e_mp2, _ = eng.do_mp2_spatial(n, o, res.canon_coeff, lev, ints.eri, want_eri_mo=False)
    h_act, e_core = eng.core_operator(n, nfc, 0, res.canon_coeff, ints.core_hamil)
    if windowed:
        _, e_mp2 = eng.mo_window(n, o, nfc, 0, lev, want_eri=False)
    path = tmp_path / "FCIDUMP"
    nw = eng.write_fcidump_active(path, n - nfc, ints.nel - 2 * nfc, 0, h_act, e_core + ints.e_nuc, 0.0)
    rec = fcidump.read(path)
    gap = abs(fcidump.hf_energy(rec) - (res.e_hf + ints.e_nuc))
    print(f"nfc={nfc}: lines {nw}, E(HF) gap {gap:.2e}, levels {np.max(np.abs(fcidump.fock_diagonal(rec) - lev[nfc:])):.2e}, "
          f"E(MP2) {abs(fcidump.mp2_energy(rec) - e_mp2):.2e}")
    assert (rec.norb, rec.nelec, rec.ms2, rec.uhf, rec.nlines) == (n - nfc, ints.nel - 2 * nfc, 0, False, nw)
    assert gap < 1e-9
    assert np.max(np.abs(fcidump.fock_diagonal(rec) - lev[nfc:])) < 1e-9
    assert abs(fcidump.mp2_energy(rec) - e_mp2) < 1e-10


def test_open_shell_dump_is_the_hamiltonian(eng, tmp_path):
    """The doublet H2O+ of test_gpu_uhf.py with nfc = 1: E(UHF), both spins' levels, E(UMP2), and the order of the blocks in the file."""
    nfc = 1
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, charge=1, multiplicity=2, **TIGHT)
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    eng.set_eri(n, ints.eri)
    u = uhf.do_uhf(si, ints, na, nb, None, lambda da, db: eng.build_fock_uhf(n, da, db, ints.core_hamil))
    assert u.converged
    eng.do_ump2(n, na, nb, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, None, want_eri_mo=False)
    ha, hb, e_core = eng.ucore_operator(n, nfc, 0, u.coeff_a, u.coeff_b, ints.core_hamil)
    *_, e2 = eng.umo_window(n, na, nb, nfc, 0, u.levels_a, u.levels_b, want_eri=False)
    path = tmp_path / "FCIDUMP"
    nw = eng.write_fcidump_uactive(path, n - nfc, na - nfc, nb - nfc, ha, hb, e_core + ints.e_nuc, 0.0)
    rec = fcidump.read(path)
    fa, fb = fcidump.fock_diagonal(rec)
    gap = abs(fcidump.hf_energy(rec) - (u.e_hf + ints.e_nuc))
    print(f"H2O+: lines {nw}, E(UHF) gap {gap:.2e}, levels {np.max(np.abs(fa - u.levels_a[nfc:])):.2e} {np.max(np.abs(fb - u.levels_b[nfc:])):.2e}, "
          f"E(UMP2) {abs(fcidump.mp2_energy(rec) - e2):.2e}")
    assert (rec.norb, rec.nelec, rec.ms2, rec.uhf, rec.nlines) == (2 * (n - nfc), na + nb - 2 * nfc, na - nb, True, nw)
    assert gap < 1e-9
    assert np.max(np.abs(fa - u.levels_a[nfc:])) < 1e-9 and np.max(np.abs(fb - u.levels_b[nfc:])) < 1e-9
    assert abs(fcidump.mp2_energy(rec) - e2) < 1e-10
    # alpha-alpha, beta-beta, alpha-beta, h_alpha, h_beta, core energy -- in this order, no spin-forbidden line
    text = path.read_text()
    assert "UHF=.TRUE." in text.split("&END")[0]
    idx = np.array([ln.split()[1:] for ln in text.split("&END\n")[1].splitlines()], dtype=np.int64)
    odd = idx % 2 == 1
    two = idx[:, 2] > 0
    kind = np.where(two & odd[:, 0] & odd[:, 2], 0, np.where(two & ~odd[:, 0] & ~odd[:, 2], 1, np.where(two, 2, np.where(
        idx[:, 0] == 0, 5, np.where(odd[:, 0], 3, 4)))))
    assert np.all(np.diff(kind) >= 0) and set(kind) == {0, 1, 2, 3, 4, 5}
    assert np.all(odd[two, 0] == odd[two, 1]) and np.all(odd[two, 2] == odd[two, 3]) and np.all(odd[kind == 2, 0] & ~odd[kind == 2, 2])


def _resident(eng, n, packed):
    """any packed array resident as MO integrals: handed in through the window call with nothing frozen"""
    o = 3
    lev = np.concatenate([-2.0 - np.arange(o), 1.0 + np.arange(n - o)])
    eng.mo_window(n, o, 0, 0, lev, eri_mo=packed, want_eri=False)


@pytest.mark.parametrize("threshold", [0.05, 0.0])
def test_compaction_keeps_numpys_selection_in_canonical_order(eng, tmp_path, threshold):
    """n = 28 (82621 elements: 41 chunks of 2048, the last one partial): sigma = 0.05, so a threshold of 0.05 removes the 68 % inside one
    sigma; threshold 0 removes exactly the planted zeros.  The file equals the numpy selection byte for byte -- lines, order, count --
    and a second call writes the same bytes."""
    n, rng = 28, np.random.default_rng(28)
    packed = 0.05 * rng.standard_normal(inputs.neri(n))
    packed[rng.integers(0, packed.size, 500)] = 0.0
    packed[[0, 2047, 2048, packed.size - 1]] = [0.0, 0.3, -0.3, 0.7]
    h = _sym(rng, n)
    h[3, 1] = h[1, 3] = 0.0
    _resident(eng, n, packed)
    a, b = tmp_path / "a", tmp_path / "b"
    nw = eng.write_fcidump_active(a, n, 6, 0, h, -3.5, threshold)
    ref = np_fcidump.dump_text(n, 6, 0, packed, h, -3.5, threshold)
    kept = int(np.count_nonzero(np.abs(packed) > threshold))
    print(f"threshold {threshold}: {kept} of {packed.size} integrals kept, {nw} lines")
    assert (0.25 < kept / packed.size < 0.40) if threshold > 0 else (packed.size - 501 <= kept < packed.size)
    assert a.read_text() == ref
    assert nw == len(ref.split("&END\n")[1].splitlines()) == kept + int(np.count_nonzero(np.abs(np.tril(h)) > threshold)) + 1
    assert eng.write_fcidump_active(b, n, 6, 0, h, -3.5, threshold) == nw
    assert a.read_bytes() == b.read_bytes()


def test_compaction_at_three_digit_indices(eng, tmp_path):
    """n = 100 (1.3e7 elements, 6228 chunks: the grid-stride loop runs): every line splits into five fields and the largest index read
    back is 100; the lines are numpy's selection.  A threshold of four sigma keeps the file small."""
    n, rng = 100, np.random.default_rng(100)
    packed = 0.05 * rng.standard_normal(inputs.neri(n))
    packed[-1] = 1.0                                           # (100 100 | 100 100)
    h = np.zeros((n, n))
    h[n - 1, 0] = h[0, n - 1] = 0.5
    _resident(eng, n, packed)
    path = tmp_path / "FCIDUMP"
    nw = eng.write_fcidump_active(path, n, 6, 0, h, 0.0, 0.2)
    body = path.read_text().split("&END\n")[1].splitlines()
    fields = [ln.split() for ln in body]
    assert all(len(f) == 5 for f in fields) and nw == len(body)
    assert max(int(x) for f in fields for x in f[1:]) == 100
    assert body == np_fcidump.dump_text(n, 6, 0, packed, h, 0.0, 0.2).split("&END\n")[1].splitlines()
    rec = fcidump.read(path)
    assert rec.eri[-1] == 1.0 and rec.h[n - 1, 0] == 0.5 and np.count_nonzero(rec.eri) == nw - 2


def test_refusals_leave_the_resident_integrals_untouched(tmp_path):
    """Status 1 for a negative count, no active orbital, a NULL argument, nothing resident, a call after the window -- and afterwards
    ccsd_init(NULL) reads the same integrals as before."""
    from afesp_amd.capi import AfespError, Engine
    n, o, nfc = 24, 4, 1
    eri, c, lev = _random_system(n, o, 3)
    h_ao = _sym(np.random.default_rng(4), n)
    with Engine(0) as e:
        with pytest.raises(AfespError, match="status 1"):          # nothing resident
            e.core_operator(n, nfc, 0, c, h_ao)
        with pytest.raises(AfespError, match="status 1"):
            e.ucore_operator(n, nfc, 0, c, c, h_ao)
        with pytest.raises(AfespError, match="status 1"):
            e.write_fcidump_active(tmp_path / "x", n, 2 * o, 0, h_ao, 0.0, 0.0)
        with pytest.raises(AfespError, match="status 1"):
            e.write_fcidump_uactive(tmp_path / "x", n, o, o, h_ao, h_ao, 0.0, 0.0)
        e.do_mp2_spatial(n, o, c, lev, eri, want_eri_mo=False)
        e.ccsd_init(o, n - o, lev, None, 4)
        before = e.tensor("v_oovv")
        for bad in ((-1, 0), (0, -1), (n, 0), (0, n), (n - 3, 3), (n + 2, 0)):
            with pytest.raises(AfespError, match="status 1"):
                e.core_operator(n, bad[0], bad[1], c, h_ao)
        with pytest.raises(AfespError, match="status 1"):          # another basis size
            e.core_operator(n - 1, nfc, 0, c[:n - 1, :n - 1], h_ao[:n - 1, :n - 1])
        with pytest.raises(AfespError, match="status 1"):          # closed-shell integrals are not open-shell ones
            e.ucore_operator(n, nfc, 0, c, c, h_ao)
        with pytest.raises(AfespError, match="status 1"):          # a negative threshold
            e.write_fcidump_active(tmp_path / "x", n, 2 * o, 0, h_ao, 0.0, -1.0)
        out, ec, vp = np.zeros(n * n), C.c_double(), C.c_void_p
        good = [capi._f(c).ctypes.data_as(vp), capi._f(h_ao).ctypes.data_as(vp), out.ctypes.data_as(vp), C.cast(C.byref(ec), vp)]
        e.L.afesp_core_operator.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64, vp, vp, vp, vp]
        try:
            for k in range(4):                                     # each pointer NULL in turn
                args = list(good)
                args[k] = None
                assert e.L.afesp_core_operator(e.h, n, nfc, 0, *args) == 1
            assert e.L.afesp_core_operator(e.h, n, nfc, 0, *good) == 0
        finally:
            e.L.afesp_core_operator.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64, capi._dp, capi._dp, capi._dp, C.POINTER(C.c_double)]
        e.ccsd_init(o, n - o, lev, None, 4)
        assert np.array_equal(e.tensor("v_oovv"), before)
        h_act, _ = e.core_operator(n, nfc, 2, c, h_ao)             # a legal call still works ...
        assert h_act.shape == (n - 3, n - 3)
        e.mo_window(n, o, nfc, 2, lev, want_eri=False)
        with pytest.raises(AfespError, match="status 1"):          # ... and after the window the core orbitals are gone
            e.core_operator(n, nfc, 2, c, h_ao)
        assert e.write_fcidump_active(tmp_path / "ok", n - 3, 2 * (o - nfc), 0, h_act, 0.0, 1e-7) > 0
