"""The numpy restatement of the EOM-CCSD triples correction (np_eom_t.py) held to the operator definition evaluated in the occupation-number
basis (np_fockspace.py), its limits, the condition of the GPU test's reference values, the input key and the exports.  No GPU.

  (i)   element by element and per triple, np_eom_t's P(m), P(l) and value against <mu3| [H, R2] + [[H, R1], T2] |0>, <0| (L1 + L2) H |mu3>
        and sum l m / (omega - D_eps) at o, v = 3, 3 and 4, 6, with and without f_ov: 1e-12 relative to the majorant
  (ii)  omega = 0, l = lambda, r = (0, t2) is np_lambda_t.lt_per_triple; bilinear in L and R; invariant under L -> L / c, R -> c R; no
        triples for o < 3
  (iii) with the vectors the GPU test uses, no triple's value is cancelled away, and no denominator changes sign
  (iv)  eom_triples is accepted with eom_nroots > 0 and eom_left only
  (v)   afesp_version() >= 6, the entry point is exported, declared and bound"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import np_eom_t as ET
import np_fockspace as FS
import np_lambda_t as LT
import np_triples as T
from afesp_amd import capi, eom, inputs
from np_triples import LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EXE = os.path.join(ROOT, "a-fortran-electronic-structure-program_amd", "host", "els_amd")


def _system(o, v, seed, fock):
    """random antisymmetric <pq||rs> with the symmetry of real orbitals, levels with a gap, a random f_ov on the Fock entry"""
    n = o + v
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, n, n, n))
    a = a - a.transpose(1, 0, 2, 3)
    a = a - a.transpose(0, 1, 3, 2)
    g = 0.5 * (a + a.transpose(2, 3, 0, 1))
    lev = np.concatenate([-2.0 - rng.uniform(0, 1, o), 1.0 + rng.uniform(0, 1, v)])
    f = np.diag(lev)
    f_ov = None
    if fock:
        f_ov = rng.uniform(-0.5, 0.5, (o, v))
        f[:o, o:], f[o:, :o] = f_ov, f_ov.T
    _, t2 = T.random_so_amplitudes(o, v, seed + 1)
    return g, lev, f, f_ov, t2, T.random_so_amplitudes(o, v, seed + 2), T.random_so_amplitudes(o, v, seed + 3)


@pytest.mark.parametrize("fock", [False, True])
@pytest.mark.parametrize("o,v", [(3, 3), (4, 6)])
def test_restatement_against_the_operator_definition(o, v, fock):
    """(i)"""
    g, lev, f, f_ov, t2, (l1, l2), (r1, r2) = _system(o, v, 40 + o, fock)
    m, ell = FS.eom_t_numerators(f, g, o, t2, l1, l2, r1, r2)
    pm, pl = ET.numerator_arrays(g, o, t2, l1, l2, r1, r2, f_ov)
    omega = 0.4
    val, S = ET.eom_t_per_triple(g, lev, o, t2, omega, l1, l2, r1, r2, f_ov)
    assert len(val) == len(T.so_order(o))
    worst = 0.0
    for n, (i, j, k) in enumerate(T.so_order(o)):
        oracle = 0.0
        for a, b, c in itertools.combinations(range(v), 3):
            d_eps = lev[o + a] + lev[o + b] + lev[o + c] - lev[i] - lev[j] - lev[k]
            oracle += ell[i, j, k, a, b, c] * m[i, j, k, a, b, c] / (omega - d_eps)
            assert abs(pm[i, j, k, a, b, c] - m[i, j, k, a, b, c]) < 1e-12 * np.max(np.abs(m))
            assert abs(pl[i, j, k, a, b, c] - ell[i, j, k, a, b, c]) < 1e-12 * np.max(np.abs(ell))
        worst = max(worst, abs(float(val[n]) - oracle) / float(S[n]))
        assert abs(float(val[n]) - oracle) <= 1e-12 * float(S[n]), (i, j, k)
    print("largest |restatement - oracle| / S", worst)
    assert np.all(np.abs(val) > 1e-6 * S)


def test_lambda_t_limit_bilinearity_and_scale_invariance():
    """(ii)"""
    c = T.so_case(*T.SO_CASES[2])
    l1, l2 = T.random_so_amplitudes(c.o, c.v, 3)
    zero = np.zeros_like(c.t1)
    val, S = ET.eom_t_per_triple(c.g, c.lev, c.o, c.t2, 0.0, l1, l2, zero, c.t2, c.f_ov)
    ref, Sr = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, l1, l2, c.f_ov)
    assert np.all(np.abs(val - ref) <= LD(1e-13) * Sr) and np.all(np.abs(S - Sr) <= LD(1e-13) * Sr)
    # bilinear
    w = 0.3
    (a1, a2), (b1, b2) = T.random_so_amplitudes(c.o, c.v, 4), T.random_so_amplitudes(c.o, c.v, 5)
    (r1, r2), (s1, s2) = T.random_so_amplitudes(c.o, c.v, 6), T.random_so_amplitudes(c.o, c.v, 7)
    f = lambda L, R: ET.eom_t_per_triple(c.g, c.lev, c.o, c.t2, w, *L, *R, c.f_ov)
    vaa, Saa = f((a1, a2), (r1, r2))
    vba, Sba = f((b1, b2), (r1, r2))
    vab, Sab = f((a1, a2), (s1, s2))
    vl, _ = f((a1 + 2 * b1, a2 + 2 * b2), (r1, r2))
    vr, _ = f((a1, a2), (r1 - 3 * s1, r2 - 3 * s2))
    assert np.all(np.abs(vl - (vaa + 2 * vba)) <= LD(1e-16) * (Saa + 2 * Sba))
    assert np.all(np.abs(vr - (vaa - 3 * vab)) <= LD(1e-16) * (Saa + 3 * Sab))
    # L -> L / c, R -> c R
    vs, _ = f((a1 / 4, a2 / 4), (4 * r1, 4 * r2))
    assert np.all(np.abs(vs - vaa) <= LD(1e-17) * Saa)
    # not the omega = 0 value: the shift is in
    v0, _ = ET.eom_t_per_triple(c.g, c.lev, c.o, c.t2, 0.0, a1, a2, r1, r2, c.f_ov)
    assert np.all(np.abs(v0 - vaa) > LD(1e-6) * Saa)
    # o < 3: no triples
    g2, lev2, _, _, t2, (x1, x2), (y1, y2) = _system(2, 4, 9, False)
    v2, S2 = ET.eom_t_per_triple(g2, lev2, 2, t2, 0.1, x1, x2, y1, y2)
    assert len(v2) == 0 and len(S2) == 0


@pytest.mark.parametrize("n,na,nb,fock", T.SO_CASES)
def test_no_reference_value_is_cancelled_away(n, na, nb, fock):
    """(iii)"""
    c = T.so_case(n, na, nb, fock)
    omega, L, R = ET.case_vectors(c, 2)
    eo, ev = np.sort(c.lev[:c.o]), np.sort(c.lev[c.o:])
    gap = ev[:3].sum() - eo[-3:].sum()
    assert np.all(omega > 0) and np.all(omega < 0.5 * gap) and abs(omega[0] - omega[1]) > 0.1 * gap
    for s in range(2):
        val, S = ET.eom_t_per_triple(c.g, c.lev, c.o, c.t2, omega[s], *L[s], *R[s], c.f_ov)
        assert len(val) == len(T.so_order(c.o))
        r = (np.abs(val) / S).astype(np.float64)
        print("state", s, "smallest |value| / majorant", r.min())
        assert np.all(r >= 1e3 * ET.tol_factor(c.o, c.v)), r.min()


def test_min_gap_and_the_refusal_of_vectors_that_are_not_biorthonormal():
    lev = np.array([-3.0, -1.0, -2.0, -1.5, 0.5, 2.0, 1.0, 0.7])
    gap = (0.5 + 0.7 + 1.0) - (-1.0 - 1.5 - 2.0)
    out = eom.triples_min_gap([0.1, gap - 0.01], lev, 4)
    assert np.allclose(out, [gap - 0.1, 0.01], rtol=0, atol=1e-14)
    assert eom.INTRUDER_GAP == 0.05
    l = (np.ones((4, 4)), np.zeros((4, 4, 4, 4)))
    with pytest.raises(ValueError, match="biorthonormalise the vectors first"):
        eom.so_eom_triples_correction(None, [0.1], [l], [l])
    text = eom.triples_table(np.array([0.1, 0.2]), np.array([-0.01, 0.02]), dict(min_gap=np.array([1.0, 0.01]), intruder=[1]))
    assert len(text.splitlines()) == 4 and "root 2" in text.splitlines()[-1] and "not reliable" in text


def test_eom_triples_key(tmp_path):
    """(iv)"""
    def write(body):
        (tmp_path / "els.in").write_text("&elsinput\n" + body + "\n/\n")
        return str(tmp_path / "els.in")
    assert inputs.read_els_in(write('calc_type="CCSD_spinorb",\neom_nroots=2,\neom_left=.true.')).eom_triples is False
    for calc in inputs.CC_DENSITY_TYPES:
        assert inputs.read_els_in(write(f'calc_type="{calc}",\neom_nroots=2,\neom_left=.true.,\neom_triples=.true.')).eom_triples is True
    bad = ('calc_type="CCSD_spinorb",\neom_triples=.true.', 'calc_type="CCSD_spinorb",\neom_nroots=2,\neom_triples=.true.',
           'calc_type="UCCSD",\neom_left=.false.,\neom_nroots=3,\neom_triples=.true.')
    for body in bad:
        with pytest.raises(ValueError, match="eom_triples needs eom_nroots > 0 and eom_left"):
            inputs.read_els_in(write(body))
    with pytest.raises(ValueError):
        inputs.read_els_in(write('calc_type="CCSD_spinorb",\neom_nroots=2,\neom_left=.true.,\neom_triples=3'))
    if not os.path.exists(HOST_EXE):
        pytest.skip("els_amd not built")
    for body in bad[:2]:
        write(body)
        res = subprocess.run([HOST_EXE], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert res.returncode != 0 and "eom_triples needs eom_nroots > 0 and eom_left" in res.stderr, res.stderr
        assert "system::read_system_in" in res.stderr


def test_library_header_and_wrappers_export_the_call():
    """(v)"""
    name = "afesp_ccsd_so_eom_t"
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.afesp_version() >= 6
    assert hasattr(lib, name) and name in capi.EXPORTS
    assert getattr(capi.load_library(), name).argtypes is not None
    out = ctypes.c_double(7.0)
    fn = getattr(lib, name)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]
    assert fn(None, 1, None, None, None, None, None, 0, 1, ctypes.byref(out)) == 1 and out.value == 7.0   # a NULL context is an argument error
    header = open(os.path.join(ROOT, "include", "afesp.h")).read()
    assert f"int {name}(afesp_ctx* ctx, int nstates, const double* omega, const double* l1, const double* l2, const double* r1," in header
    f90 = open(os.path.join(ROOT, "a-fortran-electronic-structure-program_amd", "host", "afesp_capi.f90")).read()
    assert f"bind(C, name='{name}')" in f90
    assert callable(capi.Engine.so_eom_t) and callable(eom.so_eom_triples_correction) and callable(eom.triples_table)
