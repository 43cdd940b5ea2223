"""GPU parity of the open-shell path: afesp_build_fock_uhf, afesp_ao2mo_ump2 and the UHF-fed spin-orbital CCSD / (T)
(afesp_ccsd_uso_init + the existing afesp_ccsd_so_* calls) against numpy (np_ucc) and against the RHF-fed path."""
import dataclasses

import numpy as np
import pytest

import molecules
import np_ucc
from afesp_amd import inputs, uhf
from afesp_amd.rhf import unpack_eri

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _random_ints(n, seed):
    rng = np.random.default_rng(seed)
    return 0.05 * rng.standard_normal(inputs.neri(n))


def _sym(rng, n):
    a = rng.standard_normal((n, n))
    return 0.1 * (a + a.T)


@pytest.mark.parametrize("n", [24, 90])
def test_fock_uhf_matches_numpy_and_equals_the_rhf_build_for_equal_densities(eng, n):
    rng = np.random.default_rng(n)
    eri = _random_ints(n, n)
    eng.set_eri(n, eri)
    H, da, db = _sym(rng, n), _sym(rng, n), _sym(rng, n)
    fa, fb = eng.build_fock_uhf(n, da, db, H)
    V = unpack_eri(n, eri)
    J = np.einsum("ijkl,kl->ij", V, da + db)
    ra, rb = H + J - np.einsum("ikjl,kl->ij", V, da), H + J - np.einsum("ikjl,kl->ij", V, db)
    assert np.max(np.abs(fa - ra)) < 1e-12 * np.max(np.abs(ra))
    assert np.max(np.abs(fb - rb)) < 1e-12 * np.max(np.abs(rb))
    f2a, f2b = eng.build_fock_uhf(n, da, da, H)
    f = eng.build_fock(n, da, H)
    assert np.array_equal(f2a, f) and np.array_equal(f2b, f)


@pytest.mark.parametrize("n,na,nb", [(24, 5, 3), (80, 7, 9)])
def test_ump2_blocks_and_energy_match_numpy(eng, n, na, nb):
    rng = np.random.default_rng(100 + n)
    eri = _random_ints(n, 7 + n)
    Ca, Cb = rng.standard_normal((n, n)) / np.sqrt(n), rng.standard_normal((n, n)) / np.sqrt(n)
    ea = np.sort(rng.uniform(-2, 2, n)); ea[na:] += 3.0
    eb = np.sort(rng.uniform(-2, 2, n)); eb[nb:] += 3.0
    e2, aa, ab, bb = eng.do_ump2(n, na, nb, Ca, Cb, ea, eb, eri)
    raa, rab, rbb = np_ucc.mo_blocks(n, Ca, Cb, eri)
    scale = np.max(np.abs(raa))
    assert np.max(np.abs(aa - np_ucc.pack8(raa))) < 1e-12 * scale
    assert np.max(np.abs(bb - np_ucc.pack8(rbb))) < 1e-12 * scale
    assert np.max(np.abs(ab - np_ucc.pair_matrix(rab))) < 1e-12 * scale
    ref = np_ucc.ump2(raa, rab, rbb, ea, eb, na, nb)
    assert abs(e2 - ref) < 1e-11 * abs(ref)


def test_ump2_closed_shell_limit_is_the_mp2_energy(eng):
    si, ints, res, _ = molecules.load("h2o-cc-pvdz")
    n, o = ints.nbasis, ints.nel // 2
    e2, *_ = eng.do_ump2(n, o, o, res.canon_coeff, res.canon_coeff, res.canon_levels, res.canon_levels, ints.eri, want_eri_mo=False)
    assert abs(e2 - molecules.SURVEY_GOLD["h2o-cc-pvdz"]["mp2_corr"]) < 1e-9


def _cation(eng, name):
    """doublet cation: UHF with the GPU Fock build -> (ints, na, nb, UHFResult)"""
    si, ints, _, _ = molecules.load(name)
    si = dataclasses.replace(si, charge=1, multiplicity=2, scf_maxiter=200, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_read_guess=False)
    na, nb = inputs.spin_counts(si, ints.nel, ints.nbasis)
    eng.set_eri(ints.nbasis, ints.eri)
    u = uhf.do_uhf(si, ints, na, nb, None, lambda da, db: eng.build_fock_uhf(ints.nbasis, da, db, ints.core_hamil))
    assert u.converged
    return ints, na, nb, u


def _gpu_named(eng):
    return {k: eng.so_tensor(k) for k in ("tau", "tau_tilde", "F_vv", "F_oo", "F_ov", "W_oooo", "W_ovvo", "W_vvvv")}


def _np_named(cc):
    """np_ucc's intermediates in the engine's storage (W_oooo(i,j,m,n) carrying the whole 1/2 tau <mn||ef> term, W_abef(e,f,a,b)
    none of it: the engine adds the two quarter terms of Eqs. 6-7 in one place)"""
    I = dict(cc.last)
    q = np.einsum("ijef,mnef->mnij", I["tau"], cc.oovv, optimize=True)
    I["W_oooo"] = (I["W_oooo"] + 0.25 * q).transpose(2, 3, 0, 1)
    I["W_vvvv"] = (I["W_vvvv"] - 0.25 * np.einsum("mnab,mnef->abef", I["tau"], cc.oovv, optimize=True)).transpose(2, 3, 0, 1)
    return I


@pytest.mark.parametrize("name", ["h2o-cc-pvdz", "f2-cc-pvdz"])
def test_doublet_cation_uccsd_and_triples_match_numpy(eng, name):
    ints, na, nb, u = _cation(eng, name)
    n = ints.nbasis
    e2, *_ = eng.do_ump2(n, na, nb, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, None, want_eri_mo=False)
    aa, ab, bb = np_ucc.mo_blocks(n, u.coeff_a, u.coeff_b, ints.eri)
    assert abs(e2 - np_ucc.ump2(aa, ab, bb, u.levels_a, u.levels_b, na, nb)) < 1e-10
    cc = np_ucc.UCC(*np_ucc.so_integrals(aa, ab, bb, u.levels_a, u.levels_b, na, nb))
    eng.init_cc_uspinorb(n, na, nb, u.levels_a, u.levels_b, 8)
    assert np.max(np.abs(eng.so_tensor("oovv") - cc.oovv)) < 1e-12
    # iteration by iteration (no DIIS on either side: the restatement's own DIIS is not the engine's)
    e, r, _ = eng.so_energy(1e-12, 1e-12)
    ne, nr = cc.energy_step()
    assert abs(e - ne) < 1e-10 and abs(r - nr) < 1e-10 and abs(e - e2) < 1e-10
    for it in range(6):
        e, r, _ = eng.so_iterate(1e-12, 1e-12)
        cc.iterate()
        ne, nr = cc.energy_step()
        assert abs(e - ne) < 1e-10 and abs(r - nr) < 1e-10, it
        if it == 1:
            gpu, ref = _gpu_named(eng), _np_named(cc)
            for k, v in gpu.items():
                assert np.max(np.abs(v - ref[k])) < 1e-10, k
    # converged: the engine's loop (its DIIS) against the restatement's fixed point
    eng.init_cc_uspinorb(n, na, nb, u.levels_a, u.levels_b, 8)
    nit, en, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    _, ec = cc.solve(300, 1e-12, 1e-12)
    assert abs(en[nit] - ec) < 1e-10
    t1, t2 = eng.so_amplitudes()
    assert np.max(np.abs(t1 - cc.t1)) < 1e-9 and np.max(np.abs(t2 - cc.t2)) < 1e-9
    eng.so_set_amplitudes(cc.t1, cc.t2)
    e_t = eng.do_ccsd_t_spinorb()
    assert abs(e_t - cc.triples()) < 1e-10
    nt = eng.so_ntriples()
    assert nt == (na + nb) * (na + nb - 1) * (na + nb - 2) // 6
    parts = [eng.do_ccsd_t_spinorb(a, b) for a, b in ((0, nt // 3), (nt // 3, nt // 2), (nt // 2, nt))]
    assert abs(sum(parts) - e_t) < 1e-12


@pytest.mark.parametrize("name", ["n2-cc-pvdz", "f2-cc-pvdz"])
def test_closed_shell_limit_equals_the_rhf_fed_spin_orbital_path(eng, name):
    """RHF orbitals for both spins through the new calls: at the input's tolerances the same iterations (DIIS is blind to the order
    of the spin orbitals) and the same (T) as the RHF-fed state with F_mi in the published order."""
    si, ints, res, _ = molecules.load(name)
    n, o = ints.nbasis, ints.nel // 2
    eng.do_mp2_spatial(n, o, res.canon_coeff, res.canon_levels, ints.eri, want_eri_mo=False)
    eng.init_cc_spinorb(n, ints.nel, res.canon_levels, None, 8, foo_as_published=True)
    nit, en, rm = eng.do_ccsd_spinorb(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    e_t = eng.do_ccsd_t_spinorb()
    eng.do_ump2(n, o, o, res.canon_coeff, res.canon_coeff, res.canon_levels, res.canon_levels, ints.eri, want_eri_mo=False)
    eng.init_cc_uspinorb(n, o, o, res.canon_levels, res.canon_levels, 8)
    unit, uen, urm = eng.do_ccsd_spinorb(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    assert unit == nit > 0
    assert np.max(np.abs(uen - en)) < 1e-10 and np.max(np.abs(urm - rm)) < 1e-10
    assert abs(eng.do_ccsd_t_spinorb() - e_t) < 1e-10


def test_two_electron_triplet_uccsd_is_fci(eng):
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, charge=8, multiplicity=3, scf_maxiter=200, scf_e_tol=1e-12, scf_d_tol=1e-10)
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    u = uhf.do_uhf(si, ints, na, nb)
    eng.do_ump2(n, na, nb, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, ints.eri, want_eri_mo=False)
    eng.init_cc_uspinorb(n, na, nb, u.levels_a, u.levels_b, 8)
    nit, en, _ = eng.do_ccsd_spinorb(200, 1e-12, 1e-12)
    assert nit > 0
    aa, ab, _ = np_ucc.mo_blocks(n, u.coeff_a, u.coeff_b, ints.eri)
    h = lambda C: C @ ints.core_hamil @ C.T
    assert abs(u.e_hf + en[nit] - np_ucc.fci_two_electron(n, aa, ab, h(u.coeff_a), h(u.coeff_b), True)) < 1e-10
    assert eng.so_ntriples() == 0 and eng.do_ccsd_t_spinorb() == 0.0


def _uhf_run(e, ints, na, nb, u):
    n = ints.nbasis
    e2, aa, ab, bb = e.do_ump2(n, na, nb, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, ints.eri)
    e.init_cc_uspinorb(n, na, nb, u.levels_a, u.levels_b, 8)
    nit, en, rm = e.do_ccsd_spinorb(60, 1e-9, 1e-9)
    return e2, aa, ab, bb, en, rm, e.do_ccsd_t_spinorb()


def test_uhf_and_rhf_states_do_not_see_each_other(eng):
    from afesp_amd.capi import Engine
    ints, na, nb, u = _cation(eng, "h2o-cc-pvdz")
    si, _, res, _ = molecules.load("h2o-cc-pvdz")
    n, nel = ints.nbasis, ints.nel
    with Engine(0) as fresh:
        ref_u = _uhf_run(fresh, ints, na, nb, u)
    with Engine(0) as fresh:
        e_mp2, _ = fresh.do_mp2_spatial(n, nel // 2, res.canon_coeff, res.canon_levels, ints.eri, want_eri_mo=False)
        fresh.init_cc_spinorb(n, nel, res.canon_levels, None, 8)
        ref_r = fresh.do_ccsd_spinorb(60, 1e-9, 1e-9)[1], fresh.do_ccsd_t_spinorb()
    with Engine(0) as one:
        got1 = _uhf_run(one, ints, na, nb, u)
        one.do_mp2_spatial(n, nel // 2, res.canon_coeff, res.canon_levels, ints.eri, want_eri_mo=False)
        one.init_cc_spinorb(n, nel, res.canon_levels, None, 8)
        got_r = one.do_ccsd_spinorb(60, 1e-9, 1e-9)[1], one.do_ccsd_t_spinorb()
        one.init_cc_spinorb(n, nel, res.canon_levels, None, 8)    # (the RHF MO integrals are still the RHF ones)
        assert np.max(np.abs(one.do_ccsd_spinorb(60, 1e-9, 1e-9)[1] - got_r[0])) < 1e-12
        got2 = _uhf_run(one, ints, na, nb, u)
    for a, b in ((got1, ref_u), (got2, ref_u)):
        assert all(np.max(np.abs(np.asarray(x) - np.asarray(y))) < 1e-12 for x, y in zip(a, b))
    assert np.max(np.abs(got_r[0] - ref_r[0])) < 1e-12 and abs(got_r[1] - ref_r[1]) < 1e-12
