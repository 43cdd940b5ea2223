"""The numpy reference of the EOM-IP / EOM-EA triples correction (np_eom_ipea_t.py) held to its definition, its limits, the condition of
the GPU test's reference values, the input key and the exports.  No GPU.

  (i)   the explicit forms the device follows against the ghost embedding on np_eom_t / np_lambda_t, per item and element by element, to
        1e-12 of the majorant at o, v = 3, 2 / 4, 3 / 5, 4 (IP) and 2, 3 / 3, 4 / 4, 5 (EA), with and without f_ov; the two majorants agree
  (ii)  every numerator of a triple of the enlarged system without the ghost orbital is exactly 0.0, on either side; the embedded
        numerators against the operator definition evaluated literally in the occupation-number basis (np_fockspace) at 8 spin orbitals
  (iii) bilinear in (L, R); invariant under L -> L / c, R -> c R; zero below the minimal extents; IP of a two-electron reference is zero
  (iv)  with the vectors the GPU test uses no item's value is cancelled away, and no denominator changes sign
  (v)   the min-gap diagnostic, the refusal of vectors that are not biorthonormal, the input key eom_ipea_triples
  (vi)  afesp_version() >= 8, the entry points are exported, declared and bound"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import np_eom_ipea_left as XL
import np_eom_ipea_t as Q
import np_fockspace as FS
import np_triples as T
from afesp_amd import capi, eom, inputs
from np_triples import LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EXE = os.path.join(ROOT, "a-fortran-electronic-structure-program_amd", "host", "els_amd")
IP, EA = Q.IP, Q.EA
SHAPES = {IP: [(3, 2), (4, 3), (5, 4)], EA: [(2, 3), (3, 4), (4, 5)]}


def _system(sector, o, v, seed, fock, scale=1.0):
    """random antisymmetric <pq||rs> with the symmetry of real orbitals, levels with a gap, a random f_ov on the Fock entry, t2 and a left
    and a right vector of the sector"""
    n = o + v
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, n, n, n))
    a = a - a.transpose(1, 0, 2, 3)
    a = a - a.transpose(0, 1, 3, 2)
    g = scale * 0.5 * (a + a.transpose(2, 3, 0, 1))
    lev = np.concatenate([-2.0 - rng.uniform(0, 1, o), 1.0 + rng.uniform(0, 1, v)])
    f_ov = rng.uniform(-0.5, 0.5, (o, v)) if fock else None
    _, t2 = T.random_so_amplitudes(o, v, seed + 1)
    return g, lev, f_ov, t2, Q.random_vectors(sector, o, v, seed + 2), Q.random_vectors(sector, o, v, seed + 3)


@pytest.mark.parametrize("fock", [False, True])
@pytest.mark.parametrize("sector,o,v", [(s, o, v) for s in (IP, EA) for o, v in SHAPES[s]])
def test_explicit_forms_against_the_embedding(sector, o, v, fock):
    """(i)  (integrals of scale 100, as the forms were first checked)"""
    g, lev, f_ov, t2, (l1, l2), (r1, r2) = _system(sector, o, v, 60 + 3 * o + v, fock, scale=100.0)
    omega = 0.4
    ve, Se, ee = Q.per_item_embedding(sector, g, lev, o, t2, omega, l1, l2, r1, r2, f_ov, elements=True)
    vx, Sx, ex = Q.per_item_explicit(sector, g, lev, o, t2, omega, l1, l2, r1, r2, f_ov, elements=True)
    assert len(ve) == len(vx) == Q.nitems(sector, o) == len(Q.items(sector, o)) > 0
    worst = 0.0
    for n in range(len(ve)):
        assert abs(vx[n] - ve[n]) <= LD(1e-12) * Se[n] and abs(Sx[n] - Se[n]) <= LD(1e-12) * Se[n], (n, vx[n], ve[n])
        assert ee[n].shape == ex[n].shape == ((v, v) if sector == IP else (v, v, v))
        assert np.all(np.abs(ex[n] - ee[n]) <= LD(1e-12) * Se[n])
        worst = max(worst, float(np.max(np.abs(ex[n] - ee[n])) / Se[n]))
    print("largest |explicit - embedding| / S, element by element", worst)
    assert np.all(np.abs(ve) > LD(1e-6) * Se)


@pytest.mark.parametrize("fock", [False, True])
@pytest.mark.parametrize("sector,o,v", [(IP, 4, 3), (EA, 3, 4)])
def test_triples_without_the_ghost_vanish_and_the_literal_operator_definition(sector, o, v, fock):
    """(ii)  8 spin orbitals with the ghost"""
    g, lev, f_ov, t2, (l1, l2), (r1, r2) = _system(sector, o, v, 80 + o, fock)
    num = Q.embedding_numerators(sector, g, lev, o, t2, l1, l2, r1, r2, f_ov)
    gg, levg, og, fo, ghost = Q.enlarged_system(sector, g, lev, o, f_ov)
    vg = len(levg) - og
    assert len(levg) == 8 and len(num) == len(T.so_order(og))
    fg = np.diag(levg)
    if fo is not None:
        fg[:og, og:], fg[og:, :og] = fo, fo.T
    T2 = XL.embed_plain(sector, o, v, np.zeros((o, v)), t2)[1]
    m, ell = FS.eom_t_numerators(fg, gg, og, T2, *XL.embed(sector, o, v, l1, l2), *XL.embed(sector, o, v, r1, r2))
    scale_m, scale_l = np.max(np.abs(m)), np.max(np.abs(ell))
    assert scale_m > 0.1 and scale_l > 0.1
    with_ghost = 0
    for (i, j, k), (pl, pm) in num.items():
        for a, b, c in itertools.combinations(range(vg), 3):
            has = (ghost - og in (a, b, c)) if sector == IP else (ghost in (i, j, k))
            if not has:
                assert pl[a, b, c] == 0.0 and pm[a, b, c] == 0.0, (i, j, k, a, b, c)
                assert m[i, j, k, a, b, c] == 0.0 and ell[i, j, k, a, b, c] == 0.0
            else:
                with_ghost += 1
                assert abs(pm[a, b, c] - m[i, j, k, a, b, c]) < 1e-12 * scale_m
                assert abs(pl[a, b, c] - ell[i, j, k, a, b, c]) < 1e-12 * scale_l
    # 3h2p: i<j<k, a<b beside the ghost; 3p2h: i<j beside the ghost, a<b<c
    assert with_ghost == (o * (o - 1) * (o - 2) // 6 * v * (v - 1) // 2 if sector == IP else o * (o - 1) // 2 * v * (v - 1) * (v - 2) // 6)
    # ... and the value per item is the sum over exactly those determinants
    omega = 0.3
    val, S = Q.per_item_embedding(sector, g, lev, o, t2, omega, l1, l2, r1, r2, f_ov)
    for n, it in enumerate(Q.items(sector, o)):
        i, j, k = it if sector == IP else (it[0], it[1], ghost)
        oracle = 0.0
        for a, b, c in itertools.combinations(range(vg), 3):
            d_eps = levg[og + a] + levg[og + b] + levg[og + c] - levg[i] - levg[j] - levg[k]
            oracle += ell[i, j, k, a, b, c] * m[i, j, k, a, b, c] / (omega - d_eps)
        assert abs(float(val[n]) - oracle) <= 1e-12 * float(S[n]), (it, float(val[n]), oracle)


@pytest.mark.parametrize("sector", [IP, EA])
def test_bilinearity_scale_invariance_and_minimal_extents(sector):
    """(iii)"""
    c = T.so_case(*T.SO_CASES[2])
    w = 0.3
    rv = lambda seed: Q.random_vectors(sector, c.o, c.v, seed)
    (a1, a2), (b1, b2), (r1, r2), (s1, s2) = rv(4), rv(5), rv(6), rv(7)
    f = lambda L, R, om=w: Q.per_item_explicit(sector, c.g, c.lev, c.o, c.t2, om, *L, *R, c.f_ov)
    vaa, Saa = f((a1, a2), (r1, r2))
    vba, Sba = f((b1, b2), (r1, r2))
    vab, Sab = f((a1, a2), (s1, s2))
    vl, _ = f((a1 + 2 * b1, a2 + 2 * b2), (r1, r2))
    vr, _ = f((a1, a2), (r1 - 3 * s1, r2 - 3 * s2))
    assert np.all(np.abs(vl - (vaa + 2 * vba)) <= LD(1e-16) * (Saa + 2 * Sba))
    assert np.all(np.abs(vr - (vaa - 3 * vab)) <= LD(1e-16) * (Saa + 3 * Sab))
    vs, _ = f((a1 / 4, a2 / 4), (4 * r1, 4 * r2))
    assert np.all(np.abs(vs - vaa) <= LD(1e-17) * Saa)
    v0, _ = f((a1, a2), (r1, r2), 0.0)
    assert np.all(np.abs(v0 - vaa) > LD(1e-6) * Saa)                       # the shift is in
    # below the minimal extents: zeros, one per item
    for o, v in ([(2, 4), (3, 1), (1, 5)] if sector == IP else [(1, 4), (3, 2), (4, 1)]):
        g, lev, f_ov, t2, (l1, l2), (x1, x2) = _system(sector, o, v, 9, True)
        for fn in (Q.per_item_embedding, Q.per_item_explicit):
            val, S = fn(sector, g, lev, o, t2, 0.1, l1, l2, x1, x2, f_ov)
            assert len(val) == Q.nitems(sector, o) and np.all(val == 0) and np.all(S == 0)
    # IP of a two-electron reference: its one-electron final states have no 3h2p determinant
    assert Q.nitems(IP, 2) == 0 and Q.nitems(EA, 2) == 1 and Q.nitems(IP, 3) == 1 and Q.nitems(EA, 1) == 0
    assert Q.pair_order(4) == [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)]


@pytest.mark.parametrize("sector", [IP, EA])
def test_no_reference_value_is_cancelled_away(sector):
    """(iv)"""
    got = Q.cases(sector)
    assert set(T.SO_CASES) <= set(got) and len(got) == len(T.SO_CASES) + 2
    extents = {(na + nb, 2 * n - na - nb) for n, na, nb, _ in got}
    assert ({(3, 3), (4, 2)} if sector == IP else {(3, 3), (2, 4)}) <= extents
    for n, na, nb, fock in got:
        c = T.so_case(n, na, nb, fock)
        omega, L, R, val, S = Q.reference(sector, n, na, nb, fock)
        gap = Q.min_denominator(sector, c.lev, c.o)
        assert np.all(omega > 0) and np.all(omega < 0.5 * gap) and abs(omega[0] - omega[1]) > 0.1 * gap
        for s in range(2):
            assert len(val[s]) == Q.nitems(sector, c.o)
            r = (np.abs(val[s]) / S[s]).astype(np.float64)
            print((n, na, nb, fock), "state", s, "smallest |value| / majorant", r.min())
            assert np.all(r >= 1e3 * Q.tol_factor(sector, c.o, c.v)), r.min()


def test_min_gap_and_the_refusal_of_vectors_that_are_not_biorthonormal():
    """(v)"""
    lev = np.array([-3.0, -1.0, -2.0, -1.5, 0.5, 2.0, 1.0, 0.7])
    gap_ip = (0.5 + 0.7) - (-1.0 - 1.5 - 2.0)
    gap_ea = (0.5 + 0.7 + 1.0) - (-1.0 - 1.5)
    assert np.allclose(eom.ipea_triples_min_gap(eom.SECTOR_IP, [0.1, gap_ip - 0.01], lev, 4), [gap_ip - 0.1, 0.01], rtol=0, atol=1e-14)
    assert np.allclose(eom.ipea_triples_min_gap(eom.SECTOR_EA, [0.1, gap_ea + 0.02], lev, 4), [gap_ea - 0.1, 0.02], rtol=0, atol=1e-14)
    assert np.all(np.isinf(eom.ipea_triples_min_gap(eom.SECTOR_IP, [0.1], lev[2:], 2)))
    assert eom.INTRUDER_GAP == 0.05
    lip = (np.ones(4), np.zeros((4, 4, 4)))
    with pytest.raises(ValueError, match="so_eom_ip_triples_correction: .*biorthonormalise_ipea the vectors first"):
        eom.so_eom_ip_triples_correction(None, [0.1], [lip], [lip])
    lea = (np.ones(4), np.zeros((4, 4, 4)))
    with pytest.raises(ValueError, match="so_eom_ea_triples_correction: .*biorthonormalise_ipea the vectors first"):
        eom.so_eom_ea_triples_correction(None, [0.1], [lea], [lea])
    with pytest.raises(ValueError, match="differ in length"):
        eom.so_eom_ea_triples_correction(None, [0.1, 0.2], [lea], [lea])


def test_eom_ipea_triples_key(tmp_path):
    """(v)"""
    def write(body):
        (tmp_path / "els.in").write_text("&elsinput\n" + body + "\n/\n")
        return str(tmp_path / "els.in")
    assert inputs.read_els_in(write('calc_type="CCSD_spinorb",\neom_ip_nroots=2,\neom_ipea_left=.true.')).eom_ipea_triples is False
    for sec in ("eom_ip_nroots=2", "eom_ea_nroots=1", "eom_ip_nroots=1,\neom_ea_nroots=2"):
        body = f'calc_type="CCSD_spinorb",\n{sec},\neom_ipea_left=.true.,\neom_ipea_triples=.true.'
        assert inputs.read_els_in(write(body)).eom_ipea_triples is True
    bad = ('calc_type="CCSD_spinorb",\neom_ipea_triples=.true.', 'calc_type="CCSD_spinorb",\neom_ip_nroots=2,\neom_ipea_triples=.true.',
           'calc_type="CCSD_spinorb",\neom_nroots=2,\neom_left=.true.,\neom_ipea_triples=.true.')
    for body in bad:
        with pytest.raises(ValueError, match="eom_ipea_triples needs eom_ipea_left"):
            inputs.read_els_in(write(body))
    with pytest.raises(ValueError):
        inputs.read_els_in(write('calc_type="CCSD_spinorb",\neom_ip_nroots=2,\neom_ipea_left=.true.,\neom_ipea_triples=3'))
    if not os.path.exists(HOST_EXE):
        pytest.skip("els_amd not built")
    for body in bad[:2]:
        write(body)
        res = subprocess.run([HOST_EXE], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert res.returncode != 0 and "eom_ipea_triples needs eom_ipea_left" in res.stderr, res.stderr
        assert "system::read_system_in" in res.stderr


def test_library_header_and_wrappers_export_the_calls():
    """(vi)"""
    name, count = "afesp_ccsd_so_eom_ipea_t", "afesp_ccsd_so_eom_ipea_t_nitems"
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.afesp_version() >= 8
    for sym in (name, count):
        assert hasattr(lib, sym) and sym in capi.EXPORTS
        assert getattr(capi.load_library(), sym).argtypes is not None
    nitems = getattr(lib, count)
    nitems.argtypes, nitems.restype = [ctypes.c_int, ctypes.c_int], ctypes.c_int64
    for o in range(0, 9):
        assert nitems(1, o) == Q.nitems(IP, o) and nitems(2, o) == Q.nitems(EA, o)
    assert nitems(0, 5) == 0 and nitems(3, 5) == 0
    out = ctypes.c_double(7.0)
    fn = getattr(lib, name)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_int64,
                                                                                          ctypes.POINTER(ctypes.c_double)]
    assert fn(None, 1, 1, None, None, None, None, None, 0, 1, ctypes.byref(out)) == 1 and out.value == 7.0   # a NULL context is an argument error
    header = open(os.path.join(ROOT, "include", "afesp.h")).read()
    assert f"int {name}(afesp_ctx* ctx, int sector, int nstates, const double* omega, const double* l1, const double* l2," in header
    assert f"int64_t {count}(int sector, int nocc);" in header
    f90 = open(os.path.join(ROOT, "a-fortran-electronic-structure-program_amd", "host", "afesp_capi.f90")).read()
    assert f"bind(C, name='{name}')" in f90 and f"bind(C, name='{count}')" in f90
    assert callable(capi.Engine.so_eom_ipea_t) and callable(capi.Engine.so_eom_ipea_t_nitems)
    assert callable(eom.so_eom_ip_triples_correction) and callable(eom.so_eom_ea_triples_correction) and callable(eom.triples_table)
