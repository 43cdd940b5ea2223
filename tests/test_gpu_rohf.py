"""GPU parity of the restricted open-shell path: afesp_mo_fock_ro, afesp_read_fcidump_rohf, afesp_mo_rotate_uhf and the spin-orbital CCSD /
(T) with a full Fock matrix (afesp_ccsd_uso_init_fock + the existing afesp_ccsd_so_* calls) against numpy (np_rocc, np_ucc).

Tolerances: 1e-12 x scale for integral blocks and Fock matrices, 1e-10 for energies and intermediates at equal amplitudes,
1e-9 for converged amplitudes and for energies of two separately converged solves (e_tol = t_tol = 1e-11)."""
import dataclasses

import numpy as np
import pytest

import molecules
import np_rocc
import np_ucc
from afesp_amd import fcidump, inputs, rohf, uhf
from afesp_amd.capi import AfespError
from afesp_amd.rhf import unpack_eri

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def water():
    """H2O/cc-pVDZ in the neutral molecule's RHF orbitals: packed MO integrals, their full array, h_mo"""
    si, ints, res, _ = molecules.load("h2o-cc-pvdz")
    n = ints.nbasis
    C = res.canon_coeff
    full = np.einsum("pi,qj,rk,sl,ijkl->pqrs", C, C, C, C, unpack_eri(n, ints.eri), optimize=True)
    h = C @ ints.core_hamil @ C.T
    h = np.tril(h) + np.tril(h, -1).T                     # symmetric to the bit, as a file (one triangle) gives it back
    return dict(si=si, ints=ints, res=res, n=n, packed=np_ucc.pack8(full), full=full, h=h)


def _resident_packed(eng, n, nocc):
    """the packed MO array resident for n (a (0, 0) window leaves it where it is, bit for bit, and hands it out)"""
    return eng.mo_window(n, nocc, 0, 0, np.arange(n, dtype=np.float64))[0]


def _make_resident(eng, w):
    n = w["n"]
    eng.do_mp2_spatial(n, 5, np.eye(n), w["res"].canon_levels, w["packed"], want_eri_mo=False)


@pytest.mark.parametrize("na,nb", [(5, 4), (2, 0), (5, 5)])
def test_mo_fock_ro_matches_numpy(eng, water, tmp_path, na, nb):
    w, n = water, water["n"]
    path = tmp_path / "f.fcidump"
    fcidump.write(path, w["h"], w["packed"], na + nb, na - nb, 1.5)
    rec = eng.read_fcidump_rohf(path, want_eri=True)
    packed = rec.eri                                      # (what is resident: the file's 17 digits give the doubles back)
    assert np.array_equal(packed, w["packed"])
    fa, fb, e = eng.mo_fock_ro(n, na, nb, w["h"])
    ra, rb = np_rocc.fock_ro(w["h"], w["full"], na, nb)
    scale = np.max(np.abs(ra))
    assert np.max(np.abs(fa - ra)) < 1e-12 * scale and np.max(np.abs(fb - rb)) < 1e-12 * scale
    assert np.array_equal(fa, fa.T) and np.array_equal(fb, fb.T)
    assert abs(e - np_rocc.e_ref_elec(w["h"], ra, rb, na, nb)) < 1e-12 * abs(e)
    assert np.array_equal(rec.fock_a, fa) and np.array_equal(rec.fock_b, fb)
    assert abs(rec.e_ref - (1.5 + e)) < 1e-12 * abs(e)
    if na == nb:
        closed = eng.read_fcidump(path, canonical_tol=None)
        assert np.max(np.abs(fa - closed.fock)) < 1e-12 * scale and np.max(np.abs(fb - closed.fock)) < 1e-12 * scale
    for bad in ((n, 3, 4), (n, -1, -2), (n, n + 1, 0), (n + 1, na, nb)):     # nalpha < nbeta, negative, too many, nothing resident
        with pytest.raises(AfespError, match="status 1"):
            eng.mo_fock_ro(*bad, np.zeros((bad[0], bad[0])))


def test_reader_round_trip_and_refusals(eng, water, tmp_path):
    w, n = water, water["n"]
    good = tmp_path / "good.fcidump"
    fcidump.write(good, w["h"], w["packed"], 9, 1, -3.25)
    rec = eng.read_fcidump_rohf(good, want_eri=True)
    ra, rb = np_rocc.fock_ro(w["h"], w["full"], 5, 4)
    assert (rec.norb, rec.nalpha, rec.nbeta, rec.uhf) == (n, 5, 4, False)
    assert np.array_equal(rec.eri, w["packed"]) and np.array_equal(rec.h, w["h"])
    assert np.array_equal(_resident_packed(eng, n, 5), w["packed"])
    assert rec.e_core == -3.25
    assert abs(rec.e_ref - (-3.25 + np_rocc.e_ref_elec(w["h"], ra, rb, 5, 4))) < 1e-12 * abs(rec.e_ref)
    off = lambda f, o: (np.max(np.abs(f[:o, :o] - np.diag(np.diag(f)[:o]))), np.max(np.abs(f[o:, o:] - np.diag(np.diag(f)[o:]))),
                        np.max(np.abs(f[:o, o:])))
    ref3 = np.maximum(off(ra, 5), off(rb, 4))
    assert np.max(np.abs(np.array(rec.fock_offdiag3) - ref3)) < 1e-12 * np.max(np.abs(ra))
    text = good.read_text()
    bad = {
        "uhf": text.replace("MS2= 1,", "MS2= 1,UHF=.TRUE.,"),
        "ms2": text.replace("MS2= 1,", "MS2=-1,"),
        "nelec": text.replace("NELEC=  9", "NELEC= 11"),
        "dup": text + f"{w['packed'][0] + 1e-9:24.16E}   1   1   1   1\n",
    }
    assert all(v != text for v in bad.values())
    before = eng.mo_fock_ro(n, 5, 4, w["h"])
    for k, t in bad.items():
        p = tmp_path / f"{k}.fcidump"
        p.write_text(t)
        rc = eng.L.afesp_read_fcidump_rohf(eng.h, str(p).encode(), n, 5, 4, None, None, None, None, None, None, None, None)
        assert rc == 1, k
        assert np.array_equal(_resident_packed(eng, n, 5), w["packed"]), k
    after = eng.mo_fock_ro(n, 5, 4, w["h"])
    assert all(np.array_equal(a, b) for a, b in zip(before[:2], after[:2]))


def _orthogonal(rng, n):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return q


@pytest.mark.parametrize("n", [24, 80])
def test_mo_rotate_uhf_matches_numpy(eng, n):
    rng = np.random.default_rng(500 + n)
    src = 0.05 * rng.standard_normal(inputs.neri(n))
    lev = np.arange(n, dtype=np.float64)
    eng.do_mp2_spatial(n, 3, np.eye(n), lev, src, want_eri_mo=False)
    packed = _resident_packed(eng, n, 3)
    scale = np.max(np.abs(packed))
    assert np.max(np.abs(packed - src)) < 1e-12 * scale
    ua, ub = _orthogonal(rng, n), _orthogonal(rng, n)
    aa, ab, bb = eng.mo_rotate_uhf(n, ua, ub, want_eri=True)
    raa, rab, rbb = np_ucc.mo_blocks(n, ua, ub, packed)
    rs = np.max(np.abs(raa))
    assert np.max(np.abs(aa - np_ucc.pack8(raa))) < 1e-12 * rs
    assert np.max(np.abs(bb - np_ucc.pack8(rbb))) < 1e-12 * rs
    assert np.max(np.abs(ab - np_ucc.pair_matrix(rab))) < 1e-12 * rs
    assert np.array_equal(_resident_packed(eng, n, 3), packed)          # the source: bit for bit
    aa, ab, bb = eng.mo_rotate_uhf(n, np.eye(n), np.eye(n), want_eri=True)
    full = unpack_eri(n, packed)
    assert np.max(np.abs(aa - packed)) < 1e-14 and np.max(np.abs(bb - packed)) < 1e-14
    assert np.max(np.abs(ab - np_ucc.pair_matrix(full))) < 1e-14
    if n == 24:   # the window on the rotated blocks, as after afesp_ao2mo_ump2
        eng.mo_rotate_uhf(n, ua, ub)
        waa, wab, wbb, _ = eng.umo_window(n, 5, 4, 1, 2, lev, lev)
        sl = slice(1, n - 2)
        assert np.max(np.abs(waa - np_ucc.pack8(raa[sl, sl, sl, sl]))) < 1e-12 * rs
        assert np.max(np.abs(wbb - np_ucc.pack8(rbb[sl, sl, sl, sl]))) < 1e-12 * rs
        assert np.max(np.abs(wab - np_ucc.pair_matrix(rab[sl, sl, sl, sl]))) < 1e-12 * rs


def _cation_uhf(ints, si):
    si = dataclasses.replace(si, charge=1, multiplicity=2, scf_maxiter=200, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_read_guess=False)
    na, nb = inputs.spin_counts(si, ints.nel, ints.nbasis)
    u = uhf.do_uhf(si, ints, na, nb)
    assert u.converged
    return na, nb, u


def _table(eng, iters):
    rows = [eng.so_energy(1e-12, 1e-12)[:2]]
    for _ in range(iters):
        rows.append(eng.so_iterate(1e-12, 1e-12)[:2])
        eng.so_diis()
    return np.array(rows)


def test_diagonal_fock_state_equals_the_uhf_fed_state_and_leaves_it_untouched(eng, water):
    ints = water["ints"]
    n = water["n"]
    na, nb, u = _cation_uhf(ints, water["si"])
    eng.do_ump2(n, na, nb, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, ints.eri, want_eri_mo=False)
    eng.init_cc_uspinorb(n, na, nb, u.levels_a, u.levels_b, 8)
    c0 = eng.launch_counts()
    plain = _table(eng, 4)
    c1 = eng.launch_counts()
    t_plain = eng.do_ccsd_t_spinorb()
    e2 = eng.uso_init_fock(n, na, nb, np.diag(u.levels_a), np.diag(u.levels_b), 8)
    fock = _table(eng, 4)
    t_fock = eng.do_ccsd_t_spinorb()
    assert np.max(np.abs(fock - plain)) < 1e-13 and abs(t_fock - t_plain) < 1e-13
    assert abs(e2 - plain[0, 0]) < 1e-13
    for k in ("f_ov", "f_oo", "f_vv"):
        assert not np.any(eng.so_tensor(k))
    # a plain state created after the Fock state: the launches and the table of before
    eng.init_cc_uspinorb(n, na, nb, u.levels_a, u.levels_b, 8)
    c2 = eng.launch_counts()
    again = _table(eng, 4)
    c3 = eng.launch_counts()
    assert np.array_equal(again, plain)
    assert {k: c1[k] - c0[k] for k in c0} == {k: c3[k] - c2[k] for k in c0}
    with pytest.raises(AfespError, match="f_ov"):
        eng.so_tensor("f_ov")


@pytest.fixture(scope="module")
def cation_on_rhf(water):
    """H2O+ (5, 4) on the neutral molecule's RHF orbitals -- a genuine non-HF restricted determinant -- in semicanonical orbitals: numpy"""
    w, n = water, water["n"]
    fa, fb = np_rocc.fock_ro(w["h"], w["full"], 5, 4)
    ua, ub, ga, gb = np_rocc.semicanonical(fa, fb, 5, 4)
    aa, ab, bb = np_ucc.mo_blocks(n, ua, ub, w["packed"])
    cc = np_rocc.rocc_from_blocks(aa, ab, bb, ga, gb, 5, 4)
    return dict(fa=fa, fb=fb, ua=ua, ub=ub, ga=ga, gb=gb, cc=cc)


def test_cation_on_rhf_orbitals_matches_numpy(eng, water, cation_on_rhf):
    w, n, c = water, water["n"], cation_on_rhf
    cc = c["cc"]
    assert np.max(np.abs(cc.f_ov)) > 1e-3                # non-HF indeed
    _make_resident(eng, w)
    fa, fb, _ = eng.mo_fock_ro(n, 5, 4, w["h"])
    ua, ub, ga, gb = rohf.semicanonical(fa, fb, 5, 4)
    assert np.max(np.abs(ua - c["ua"])) < 1e-9 and np.max(np.abs(ub - c["ub"])) < 1e-9
    eng.mo_rotate_uhf(n, c["ua"], c["ub"])
    e2 = eng.uso_init_fock(n, 5, 4, c["ga"], c["gb"], 8)
    assert abs(e2 - cc.e_mp2()) < 1e-10
    assert np.max(np.abs(eng.so_tensor("f_ov") - cc.f_ov)) < 1e-14 and np.max(np.abs(eng.so_tensor("oovv") - cc.oovv)) < 1e-12
    e, r, _ = eng.so_energy(1e-12, 1e-12)
    ne, nr = cc.energy_step()
    print("start", e, ne, r, nr)
    assert abs(e - ne) < 1e-10 and abs(r - nr) < 1e-10
    for it in range(5):
        e, r, _ = eng.so_iterate(1e-12, 1e-12)
        cc.iterate()
        ne, nr = cc.energy_step()
        print(it, e, ne, r, nr)
        assert abs(e - ne) < 1e-10 and abs(r - nr) < 1e-10, it
        if it == 0:
            for k in ("F_vv", "F_oo", "F_ov", "W_ovvo"):
                d = np.max(np.abs(eng.so_tensor(k) - cc.last[k]))
                print(k, d)
                assert d < 1e-10, k
    eng.uso_init_fock(n, 5, 4, c["ga"], c["gb"], 8)
    nit, en, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    _, ec = cc.solve(300, 1e-11, 1e-11)
    print("converged", nit, en[nit], ec)
    assert abs(en[nit] - ec) < 1e-9
    t1, t2 = eng.so_amplitudes()
    assert np.max(np.abs(t1 - cc.t1)) < 1e-9 and np.max(np.abs(t2 - cc.t2)) < 1e-9
    eng.so_set_amplitudes(cc.t1, cc.t2)
    e_t = eng.do_ccsd_t_spinorb()
    ref_t = cc.triples()
    print("(T)", e_t, ref_t)
    assert abs(e_t - ref_t) < 1e-10
    nt = eng.so_ntriples()
    parts = [eng.do_ccsd_t_spinorb(a, b) for a, b in ((0, nt // 3), (nt // 3, nt // 2), (nt // 2, nt))]
    assert abs(sum(parts) - e_t) < 1e-12
    # (T) needs semicanonical orbitals: an occupied-occupied off-diagonal element of 1e-3 is refused
    g = c["ga"].copy()
    g[0, 1] = g[1, 0] = 1e-3
    eng.uso_init_fock(n, 5, 4, g, c["gb"], 8)
    assert eng.L.afesp_ccsd_so_t(eng.h, 0, nt, None) == 1


def test_rohf_cc_driver_on_the_file_matches_numpy(eng, water, cation_on_rhf, tmp_path):
    """afesp_amd.rohf.rohf_cc: reader (nalpha, nbeta from the header) -> semicanonical -> rotate -> solver -> (T), from a file"""
    w, c = water, cation_on_rhf
    ref = np_rocc.rocc_from_blocks(*np_ucc.mo_blocks(w["n"], c["ua"], c["ub"], w["packed"]), c["ga"], c["gb"], 5, 4)
    e_mp2 = ref.e_mp2()
    _, e_cc = ref.solve(300, 1e-11, 1e-11)
    path = tmp_path / "cation.fcidump"
    fcidump.write(path, w["h"], w["packed"], 9, 1, 9.25)
    out = rohf.rohf_cc(eng, path, 300, 1e-11, 1e-11)
    assert (out.nbasis, out.nalpha, out.nbeta, out.e_core) == (w["n"], 5, 4, 9.25) and out.niter > 0
    assert abs(out.e_ref - (9.25 + np_rocc.e_ref_elec(w["h"], c["fa"], c["fb"], 5, 4))) < 1e-10
    assert abs(out.e_mp2 - e_mp2) < 1e-10
    assert abs(out.e_ccsd - e_cc) < 1e-9 and out.e_ccsd == out.energies[out.niter]
    assert abs(out.e_t - ref.triples()) < 1e-9                   # (two separately converged sets of amplitudes)
    off = lambda f, o: (np.max(np.abs(f[:o, :o] - np.diag(np.diag(f)[:o]))), np.max(np.abs(f[o:, o:] - np.diag(np.diag(f)[o:]))),
                        np.max(np.abs(f[:o, o:])))
    assert np.max(np.abs(np.array(out.fock_offdiag) - np.maximum(off(c["fa"], 5), off(c["fb"], 4)))) < 1e-12 * np.max(np.abs(c["fa"]))
    with pytest.raises(AfespError, match="did not converge"):
        rohf.rohf_cc(eng, path, 2, 1e-11, 1e-11)


def test_two_electron_triplet_on_rotated_orbitals_is_fci(eng, water):
    """two electrons, both alpha, on UHF orbitals rotated by a small occupied-virtual rotation (f_ov != 0): CCSD is exact"""
    ints, n = water["ints"], water["n"]
    si = dataclasses.replace(water["si"], charge=8, multiplicity=3, scf_maxiter=200, scf_e_tol=1e-12, scf_d_tol=1e-10)
    na, nb = inputs.spin_counts(si, ints.nel, n)
    u = uhf.do_uhf(si, ints, na, nb)
    C = np_rocc.triplet_rotation(n, 0.05) @ u.coeff_a
    eng.do_mp2_spatial(n, 1, C, u.levels_a, ints.eri, want_eri_mo=False)
    h = C @ ints.core_hamil @ C.T
    fa, fb, e_ref = eng.mo_fock_ro(n, na, nb, h)
    assert np.max(np.abs(fa[:na, na:])) > 1e-2
    ua, ub, ga, gb = rohf.semicanonical(fa, fb, na, nb)
    eng.mo_rotate_uhf(n, ua, ub)
    eng.uso_init_fock(n, na, nb, ga, gb, 8)
    nit, en, _ = eng.do_ccsd_spinorb(200, 1e-11, 1e-11)
    assert nit > 0
    aa, ab, _ = np_ucc.mo_blocks(n, C, C, ints.eri)
    assert abs(e_ref + en[nit] - np_ucc.fci_two_electron(n, aa, ab, h, h, True)) < 1e-9
    assert eng.so_ntriples() == 0 and eng.do_ccsd_t_spinorb() == 0.0


def test_semicanonical_state_reproduces_the_canonical_uhf_results(eng, water):
    """H2O+ on canonical UHF orbitals, rotated within the occupied and the virtual space of each spin: after semicanonicalisation on the
    device path the levels, the CCSD energy and (T) are the canonical ones"""
    ints, n = water["ints"], water["n"]
    na, nb, u = _cation_uhf(ints, water["si"])
    eng.do_ump2(n, na, nb, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, ints.eri, want_eri_mo=False)
    eng.init_cc_uspinorb(n, na, nb, u.levels_a, u.levels_b, 8)
    nit, en, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    e_t = eng.do_ccsd_t_spinorb()
    Ra, Rb = np_rocc.invariance_rotations(n, na, nb)
    fa, fb = Ra @ np.diag(u.levels_a) @ Ra.T, Rb @ np.diag(u.levels_b) @ Rb.T
    # the device rotation: the packed MO array in the alpha orbitals is the source; the beta orbitals are M times the alpha ones
    eng.do_mp2_spatial(n, nb, u.coeff_a, u.levels_a, ints.eri, want_eri_mo=False)
    M = u.coeff_b @ ints.ovlp @ u.coeff_a.T
    assert np.max(np.abs(M @ M.T - np.eye(n))) < 1e-9
    eng.mo_rotate_uhf(n, Ra, Rb @ M)
    eng.uso_init_fock(n, na, nb, fa, fb, 8)
    rit, ren, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert rit > 0 and abs(ren[rit] - en[nit]) < 1e-9          # invariant under the rotation
    ua, ub, ga, gb = rohf.semicanonical(fa, fb, na, nb)
    assert np.max(np.abs(np.diag(ga) - u.levels_a)) < 1e-9 and np.max(np.abs(np.diag(gb) - u.levels_b)) < 1e-9
    eng.mo_rotate_uhf(n, ua @ Ra, ub @ Rb @ M)
    eng.uso_init_fock(n, na, nb, ga, gb, 8)
    sit, sen, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert sit > 0 and abs(sen[sit] - en[nit]) < 1e-9
    assert abs(eng.do_ccsd_t_spinorb() - e_t) < 1e-9
