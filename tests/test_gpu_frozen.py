"""Frozen core / frozen virtuals on the GPU: afesp_mo_window / afesp_umo_window (the gather of the active orbital window
[nfc, n - nfv) out of the resident MO integrals) and the unchanged solvers on its output, against the CPU oracle on the window that
np_window cuts in numpy.  Energies, (T) sums and amplitudes to 1e-10; the window itself is a copy and must be exactly equal."""
import dataclasses

import numpy as np
import pytest

import molecules
import np_ucc
import np_window
import orc
from afesp_amd import inputs, uhf

pytestmark = pytest.mark.gpu

WINDOWS = {"h2o-cc-pvdz": (1, 0), "n2-cc-pvdz": (2, 0), "f2-cc-pvdz": (2, 3)}


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _v_oovv(o, v, packed):
    """<ij|ab> = (ia|jb) of packed integrals over o + v orbitals, as afesp_ccsd_get_tensor("v_oovv") returns it"""
    i, j, a, b = np.meshgrid(np.arange(o), np.arange(o), o + np.arange(v), o + np.arange(v), indexing="ij")
    return packed[np_window.tri(np_window.tri(a, i), np_window.tri(b, j))]


def _random_system(n, o, seed):
    rng = np.random.default_rng(seed)
    eri = 0.05 * rng.standard_normal(inputs.neri(n))
    c = rng.standard_normal((n, n)) / np.sqrt(n)
    e = np.concatenate([-2.0 - rng.random(o), 1.0 + rng.random(n - o)])
    return eri, c, e


@pytest.mark.parametrize("n,nfc,nfv", [(24, 1, 0), (28, 2, 3), (28, 0, 5), (90, 4, 7), (100, 3, 5)])
def test_packed_window_is_an_exact_copy(eng, n, nfc, nfv):
    """The window handed back to the host and the resident copy (read through v_oovv after afesp_ccsd_init) equal np_window's element
    for element; E(MP2) of the call is the oracle's on the window.  n = 100: the source array was written by the LDS-DMA transform."""
    o = nfc + 3
    eri, c, e = _random_system(n, o, 31 * n + nfc)
    before = eng.launch_counts()
    _, full = eng.do_mp2_spatial(n, o, c, e, eri)
    after = eng.launch_counts()
    if n == 100:
        assert after["tgemm"] + after["tgemm_mixed"] > before["tgemm"] + before["tgemm_mixed"], (before, after)
    ref = np_window.window_packed(n, nfc, nfv, full)
    na, oa = n - nfc - nfv, o - nfc
    va, ew = na - oa, np_window.window_levels(n, nfc, nfv, e)
    act, e_mp2 = eng.mo_window(n, o, nfc, nfv, e)
    assert act.shape == ref.shape and np.array_equal(act, ref)
    ref_e = orc.mp2_energy(na, oa, ref, ew)
    print(f"window n={n} nfc={nfc} nfv={nfv}: E(MP2) {e_mp2:.14f} oracle {ref_e:.14f} diff {abs(e_mp2 - ref_e):.2e}")
    assert abs(e_mp2 - ref_e) < 1e-10
    eng.ccsd_init(oa, va, ew, None, 4)
    assert np.array_equal(eng.tensor("v_oovv"), _v_oovv(oa, va, ref))
    # ... and from integrals the host hands in
    act2, e2 = eng.mo_window(n, o, nfc, nfv, e, eri_mo=full)
    assert np.array_equal(act2, ref) and e2 == e_mp2
    eng.ccsd_init(oa, va, ew, None, 4)
    assert np.array_equal(eng.tensor("v_oovv"), _v_oovv(oa, va, ref))


@pytest.mark.parametrize("path", ["small", "large"])
@pytest.mark.parametrize("name", ["h2o-cc-pvdz", "n2-cc-pvdz", "f2-cc-pvdz"])
def test_frozen_core_ccsd_and_triples_match_the_oracle_on_the_window(eng, name, path, monkeypatch):
    """H2O (nfc = 1), N2 (nfc = 2), F2 (nfc = 2, nfv = 3): E(MP2), the whole CCSD iteration table, t1, t2 and the four (T) sums against
    OracleCC on the window of the oracle's own MO integrals -- down the launch-fused small-system path and down the large-system path
    (AFESP_SMALL_MAX=0).  N2 also the R- / CR- sums; the small path also three cost-balanced shards."""
    if path == "large":
        monkeypatch.setenv("AFESP_SMALL_MAX", "0")
        monkeypatch.setenv("AFESP_RING_TG_MIN", "1")
    nfc, nfv = WINDOWS[name]
    si, ints, res, _ = molecules.load(name)
    n, o = ints.nbasis, ints.nel // 2
    oa, va = o - nfc, n - o - nfv
    ew = np_window.window_levels(n, nfc, nfv, res.canon_levels)
    ref = np_window.window_packed(n, nfc, nfv, orc.ao2mo(n, res.canon_coeff, ints.eri))
    eng.do_mp2_spatial(n, o, res.canon_coeff, res.canon_levels, ints.eri, want_eri_mo=False)
    act, e_mp2 = eng.mo_window(n, o, nfc, nfv, res.canon_levels)
    assert np.max(np.abs(act - ref)) < 1e-11
    ref_mp2 = orc.mp2_energy(oa + va, oa, ref, ew)
    eng.ccsd_init(oa, va, ew, None, si.ccsd_diis_n_errmat)
    cc = orc.OracleCC(oa, va, ref, ew, si.ccsd_diis_n_errmat)
    nit, en, rm = eng.do_ccsd_spatial(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    onit, oen, orm = cc.solve(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    t1, t2 = eng.amplitudes()
    out, tref = eng.do_ccsd_t_spatial(), cc.triples(ew)
    print(f"{name} {path}: E(MP2) {e_mp2:.12f} ({abs(e_mp2 - ref_mp2):.1e}) iterations {nit}/{onit} E(CCSD) {en[nit]:.12f} "
          f"(table {np.max(np.abs(en[:nit + 1] - oen[:nit + 1])):.1e}, rms {np.max(np.abs(rm[:nit + 1] - orm[:nit + 1])):.1e}) "
          f"t1 {np.max(np.abs(t1 - cc.t1)):.1e} t2 {np.max(np.abs(t2 - cc.t2)):.1e} (T) {out} ({np.max(np.abs(out - tref)):.1e})")
    assert abs(e_mp2 - ref_mp2) < 1e-10
    assert nit == onit > 0
    assert np.max(np.abs(en[:nit + 1] - oen[:nit + 1])) < 1e-10 and np.max(np.abs(rm[:nit + 1] - orm[:nit + 1])) < 1e-10
    assert np.max(np.abs(t1 - cc.t1)) < 1e-10 and np.max(np.abs(t2 - cc.t2)) < 1e-10
    assert np.max(np.abs(out - tref)) < 1e-10
    if path == "small":
        nt = eng.ntriples()
        bounds = eng.shard_bounds(3)
        assert nt == oa * (oa + 1) * (oa + 2) // 6 and bounds[0] == 0 and bounds[-1] == nt and len(bounds) == 4
        parts = sum(eng.do_ccsd_t_spatial(b0, b1) for b0, b1 in zip(bounds[:-1], bounds[1:]))
        assert np.max(np.abs(parts - out)) < 1e-12
    if name == "n2-cc-pvdz":
        eng.build_cr_intermediates()
        cr = eng.do_ccsd_t_spatial_cr()
        cc.cr_intermediates()
        cref = cc.triples_cr(ew)
        print(f"{name} {path}: CR sums {cr} ({np.max(np.abs(cr - cref)):.1e})")
        assert np.max(np.abs(cr - cref)) < 1e-10
        ec = en[nit]
        for num, den in ((1, 3), (4, 2), (5, 3)):        # R-CCSD(T), CR-CCSD[T], CR-CCSD(T)
            assert abs((ec + cr[num] / cr[den]) - (oen[onit] + cref[num] / cref[den])) < 1e-10


def test_decoupled_orbitals_full_run_equals_windowed_run_on_the_device(eng):
    """The invariant of test_frozen_cpu on the GPU: with every integral that touches orbital 0 or n - 1 zeroed, the full run and the
    run on the window [1, n - 1) give the same MP2, CCSD and (T) numbers, and both are the oracle's."""
    o, v = 4, 7
    n, e, eri = molecules.synthetic_system(o, v, scale=0.05)
    eri = np_window.decouple(n, eri, [0, n - 1])
    cc = orc.OracleCC(o, v, eri, e, 8)
    onit, oen, _ = cc.solve(50, 1e-9, 1e-9)
    tref = cc.triples(e)
    eng.ccsd_init(o, v, e, eri, 8)
    nit, en, _ = eng.do_ccsd_spatial(50, 1e-9, 1e-9)
    full_t = eng.do_ccsd_t_spatial()
    assert nit == onit and np.max(np.abs(en[:nit + 1] - oen[:nit + 1])) < 1e-10 and np.max(np.abs(full_t - tref)) < 1e-10
    act, e_mp2 = eng.mo_window(n, o, 1, 1, e, eri_mo=eri)
    ew = np_window.window_levels(n, 1, 1, e)
    assert np.array_equal(act, np_window.window_packed(n, 1, 1, eri))
    assert abs(e_mp2 - orc.mp2_energy(n, o, eri, e)) < 1e-10
    eng.ccsd_init(o - 1, v - 1, ew, None, 8)
    wnit, wen, _ = eng.do_ccsd_spatial(50, 1e-9, 1e-9)
    win_t = eng.do_ccsd_t_spatial()
    assert wnit == onit and np.max(np.abs(wen[:nit + 1] - oen[:nit + 1])) < 1e-10 and np.max(np.abs(win_t - tref)) < 1e-10
    assert np.max(np.abs(wen[:nit + 1] - en[:nit + 1])) < 1e-10 and np.max(np.abs(win_t - full_t)) < 1e-10


@pytest.mark.parametrize("name", ["h2o-cc-pvdz", "f2-cc-pvdz"])
def test_frozen_core_spin_orbital_path_matches_the_oracle(eng, name):
    """afesp_ccsd_so_init(n_act, nel - 2 nfc, NULL, levels + nfc) after the window against OracleSO on the same window: every
    iteration energy and E(T)."""
    nfc, nfv = WINDOWS[name]
    si, ints, res, _ = molecules.load(name)
    n, o = ints.nbasis, ints.nel // 2
    na, nel = n - nfc - nfv, ints.nel - 2 * nfc
    ew = np_window.window_levels(n, nfc, nfv, res.canon_levels)
    ref = np_window.window_packed(n, nfc, nfv, orc.ao2mo(n, res.canon_coeff, ints.eri))
    eng.do_mp2_spatial(n, o, res.canon_coeff, res.canon_levels, ints.eri, want_eri_mo=False)
    eng.mo_window(n, o, nfc, nfv, res.canon_levels, want_eri=False)
    eng.init_cc_spinorb(na, nel, ew, None, si.ccsd_diis_n_errmat)
    nit, en, rm = eng.do_ccsd_spinorb(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    so = orc.OracleSO(na, nel, ref, ew, si.ccsd_diis_n_errmat)
    onit, oen, orm = so.solve(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    e_t = eng.do_ccsd_t_spinorb()
    print(f"{name} spin-orbital: iterations {nit}/{onit} table {np.max(np.abs(en[:nit + 1] - oen[:nit + 1])):.1e} "
          f"E(T) {e_t:.12f} ({abs(e_t - so.triples()):.1e})")
    assert nit == onit > 0
    assert np.max(np.abs(en[:nit + 1] - oen[:nit + 1])) < 1e-10 and np.max(np.abs(rm[:nit + 1] - orm[:nit + 1])) < 1e-10
    assert abs(e_t - so.triples()) < 1e-10


def _cation(eng, name):
    si, ints, _, _ = molecules.load(name)
    si = dataclasses.replace(si, charge=1, multiplicity=2, scf_maxiter=200, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_read_guess=False)
    na, nb = inputs.spin_counts(si, ints.nel, ints.nbasis)
    eng.set_eri(ints.nbasis, ints.eri)
    u = uhf.do_uhf(si, ints, na, nb, None, lambda da, db: eng.build_fock_uhf(ints.nbasis, da, db, ints.core_hamil))
    assert u.converged
    return ints, na, nb, u


def test_doublet_cation_frozen_core_uccsd_and_triples_match_numpy(eng):
    """H2O+ (doublet) with nfc = 1, nfv = 2.  The three blocks afesp_umo_window returns are the window of the blocks afesp_ao2mo_ump2
    returned, element for element (a copy), and the sliced np_ucc.mo_blocks to the rounding of the two transforms (numpy's and the
    GPU's sum in different orders: 1e-12 of the largest integral, as test_gpu_uhf.py holds the full blocks).  Frozen-core UMP2, the
    converged UCCSD energy and (T) against np_ucc.UCC on the sliced integrals, which converges for this window in 48 iterations."""
    nfc, nfv = 1, 2
    ints, na, nb, u = _cation(eng, "h2o-cc-pvdz")
    n = ints.nbasis
    nact, la, lb = n - nfc - nfv, u.levels_a[nfc:n - nfv], u.levels_b[nfc:n - nfv]
    _, faa, fab, fbb = eng.do_ump2(n, na, nb, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, None)
    aa, ab, bb, e2 = eng.umo_window(n, na, nb, nfc, nfv, u.levels_a, u.levels_b)
    assert np.array_equal(aa, np_window.window_packed(n, nfc, nfv, faa)) and np.array_equal(bb, np_window.window_packed(n, nfc, nfv, fbb))
    assert np.array_equal(ab, np_window.window_pair_matrix(n, nfc, nfv, fab))
    raa, rab, rbb = (np_window.window_full(nfc, nfv, x) for x in np_ucc.mo_blocks(n, u.coeff_a, u.coeff_b, ints.eri))
    scale = np.max(np.abs(raa))
    assert np.max(np.abs(aa - np_ucc.pack8(raa))) < 1e-12 * scale and np.max(np.abs(bb - np_ucc.pack8(rbb))) < 1e-12 * scale
    assert np.max(np.abs(ab - np_ucc.pair_matrix(rab))) < 1e-12 * scale
    ref2 = np_ucc.ump2(raa, rab, rbb, la, lb, na - nfc, nb - nfc)
    cc = np_ucc.UCC(*np_ucc.so_integrals(raa, rab, rbb, la, lb, na - nfc, nb - nfc))
    eng.init_cc_uspinorb(nact, na - nfc, nb - nfc, la, lb, 8)
    assert np.max(np.abs(eng.so_tensor("oovv") - cc.oovv)) < 1e-12
    nit, en, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    _, ec = cc.solve(300, 1e-12, 1e-12)
    eng.so_set_amplitudes(cc.t1, cc.t2)
    e_t = eng.do_ccsd_t_spinorb()
    print(f"H2O+ nfc=1 nfv=2: E(UMP2) {e2:.12f} ({abs(e2 - ref2):.1e}) E(UCCSD) {en[nit]:.12f} ({abs(en[nit] - ec):.1e}) "
          f"E(T) {e_t:.12f} ({abs(e_t - cc.triples()):.1e})")
    assert abs(e2 - ref2) < 1e-10 and abs(en[0] - e2) < 1e-10
    assert nit > 0 and abs(en[nit] - ec) < 1e-10
    assert abs(e_t - cc.triples()) < 1e-10
    assert eng.so_ntriples() == (na + nb - 2 * nfc) * (na + nb - 2 * nfc - 1) * (na + nb - 2 * nfc - 2) // 6


@pytest.mark.parametrize("name", ["n2-cc-pvdz", "f2-cc-pvdz"])
def test_frozen_closed_shell_limit_equals_the_rhf_fed_spin_orbital_path(eng, name):
    """RHF orbitals for both spins through afesp_umo_window against the RHF-fed spin-orbital state on afesp_mo_window's output (F_mi in
    the published order, as in test_gpu_uhf.py): the same iterations and the same (T)."""
    nfc, nfv = WINDOWS[name]
    si, ints, res, _ = molecules.load(name)
    n, o = ints.nbasis, ints.nel // 2
    na, ew = n - nfc - nfv, np_window.window_levels(n, nfc, nfv, res.canon_levels)
    eng.do_mp2_spatial(n, o, res.canon_coeff, res.canon_levels, ints.eri, want_eri_mo=False)
    _, e_mp2 = eng.mo_window(n, o, nfc, nfv, res.canon_levels, want_eri=False)
    eng.init_cc_spinorb(na, ints.nel - 2 * nfc, ew, None, 8, foo_as_published=True)
    nit, en, rm = eng.do_ccsd_spinorb(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    e_t = eng.do_ccsd_t_spinorb()
    eng.do_ump2(n, o, o, res.canon_coeff, res.canon_coeff, res.canon_levels, res.canon_levels, ints.eri, want_eri_mo=False)
    *_, e_ump2 = eng.umo_window(n, o, o, nfc, nfv, res.canon_levels, res.canon_levels, want_eri=False)
    assert abs(e_ump2 - e_mp2) < 1e-10
    eng.init_cc_uspinorb(na, o - nfc, o - nfc, ew, ew, 8)
    unit, uen, urm = eng.do_ccsd_spinorb(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    assert unit == nit > 0
    assert np.max(np.abs(uen - en)) < 1e-10 and np.max(np.abs(urm - rm)) < 1e-10
    assert abs(eng.do_ccsd_t_spinorb() - e_t) < 1e-10


def test_refused_windows_leave_the_engine_usable():
    """nfc = nocc, nfv = nvirt, a negative count, a NULL source with nothing resident and a second window: status 1 each, the resident
    integrals untouched -- a legal window and a solve on the same engine afterwards give the oracle's energy."""
    from afesp_amd.capi import AfespError, Engine
    name = "h2o-cc-pvdz"
    nfc, nfv = 1, 2
    si, ints, res, _ = molecules.load(name)
    n, o = ints.nbasis, ints.nel // 2
    v, lev = n - o, res.canon_levels
    ew = np_window.window_levels(n, nfc, nfv, lev)
    ref = np_window.window_packed(n, nfc, nfv, orc.ao2mo(n, res.canon_coeff, ints.eri))
    cc = orc.OracleCC(o - nfc, v - nfv, ref, ew, si.ccsd_diis_n_errmat)
    onit, oen, _ = cc.solve(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)

    def legal_window_and_solve(e):
        act, _ = e.mo_window(n, o, nfc, nfv, lev)
        assert np.max(np.abs(act - ref)) < 1e-11
        e.ccsd_init(o - nfc, v - nfv, ew, None, si.ccsd_diis_n_errmat)
        nit, en, _ = e.do_ccsd_spatial(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
        assert nit == onit and abs(en[nit] - oen[onit]) < 1e-10

    with Engine(0) as e:
        with pytest.raises(AfespError, match="status 1"):        # nothing resident
            e.mo_window(n, o, nfc, nfv, lev)
        for bad in ((o, 0), (0, v), (-1, 0), (0, -2), (o + 3, 0), (0, v + 1)):
            e.do_mp2_spatial(n, o, res.canon_coeff, lev, ints.eri, want_eri_mo=False)
            with pytest.raises(AfespError, match="status 1"):
                e.mo_window(n, o, bad[0], bad[1], lev)
            legal_window_and_solve(e)
            with pytest.raises(AfespError, match="status 1"):    # a second window on the windowed context
                e.mo_window(n, o, nfc, nfv, lev)
            with pytest.raises(AfespError, match="status 1"):
                e.mo_window(n, o, 0, 0, lev)
            assert np.max(np.abs(e.do_ccsd_t_spatial() - cc.triples(ew))) < 1e-10   # (the solved state is still there)
        # the open-shell call: nothing resident, bad counts, a second window
        with pytest.raises(AfespError, match="status 1"):
            e.umo_window(n, o, o, nfc, nfv, lev, lev)
        e.do_ump2(n, o, o - 1, res.canon_coeff, res.canon_coeff, lev, lev, ints.eri, want_eri_mo=False)
        for bad in ((o, 0), (-1, 0), (0, -1), (0, n), (0, n - o + 1)):   # (nfc = o: the beta count would be negative)
            with pytest.raises(AfespError, match="status 1"):
                e.umo_window(n, o, o - 1, bad[0], bad[1], lev, lev)
        e.umo_window(n, o, o - 1, o - 1, 0, lev, lev, want_eri=False)      # no active beta electron: legal, as afesp_ccsd_uso_init takes it
        with pytest.raises(AfespError, match="status 1"):
            e.umo_window(n, o, o - 1, nfc, nfv, lev, lev)


def test_window_of_the_whole_basis_changes_nothing():
    """nfc = nfv = 0: the array is bit-identical, E(MP2) and the CCSD energies equal those of a run without the call to 1e-12 (the same
    kernels on the same data)."""
    from afesp_amd.capi import Engine
    si, ints, res, _ = molecules.load("n2-cc-pvdz")
    n, o = ints.nbasis, ints.nel // 2
    v = n - o
    with Engine(0) as e:
        e_mp2, full = e.do_mp2_spatial(n, o, res.canon_coeff, res.canon_levels, ints.eri)
        e.ccsd_init(o, v, res.canon_levels, None, si.ccsd_diis_n_errmat)
        nit, en, _ = e.do_ccsd_spatial(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    with Engine(0) as e:
        e.do_mp2_spatial(n, o, res.canon_coeff, res.canon_levels, ints.eri, want_eri_mo=False)
        act, w_mp2 = e.mo_window(n, o, 0, 0, res.canon_levels)
        assert np.array_equal(act, full)
        assert abs(w_mp2 - e_mp2) < 1e-12
        e.ccsd_init(o, v, res.canon_levels, None, si.ccsd_diis_n_errmat)
        wnit, wen, _ = e.do_ccsd_spatial(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
        assert wnit == nit and np.max(np.abs(wen[:nit + 1] - en[:nit + 1])) < 1e-12
        # the open-shell identity: the blocks and E(UMP2) as afesp_ao2mo_ump2 returned them
        e2, aa, ab, bb = e.do_ump2(n, o, o, res.canon_coeff, res.canon_coeff, res.canon_levels, res.canon_levels, ints.eri)
        waa, wab, wbb, we2 = e.umo_window(n, o, o, 0, 0, res.canon_levels, res.canon_levels)
        assert np.array_equal(waa, aa) and np.array_equal(wab, ab) and np.array_equal(wbb, bb) and abs(we2 - e2) < 1e-12
