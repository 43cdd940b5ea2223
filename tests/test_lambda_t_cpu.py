"""CPU checks of the Lambda-CCSD(T) reference (np_lambda_t.py): its left numerator against the CCSDT feeds of T3 into the singles and doubles
equations, l = t against (T), that the GPU test's Lambda seeds cancel no value away, linearity in Lambda; and what the built library, the
header, the input readers and the host export for it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import np_lambda_t as LT
import np_triples as T
from afesp_amd import capi, density, inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EXE = os.path.join(ROOT, "a-fortran-electronic-structure-program_amd", "host", "els_amd")
LD = np.longdouble


def _random_g(n, rng):
    """<pq||rs> = -<qp||rs> = -<pq||sr> = <rs||pq>, real, of order one"""
    a = rng.uniform(-1.0, 1.0, (n, n, n, n))
    g = a - a.transpose(1, 0, 2, 3)
    g = g - g.transpose(0, 1, 3, 2)
    return 0.5 * (g + g.transpose(2, 3, 0, 1))


def test_left_numerator_is_the_derivative_of_the_t3_feeds():
    """(i) sum_{i<j<k} sum_abc P(wc_l + wd_l) X / 6 = sum l1 R1[X] + 1/4 sum l2 R2[X] for a random fully antisymmetric X at o, v = 4, 5 with a
    random f_ov: every sign and factor of the left numerator, the f_ov l2 term included, is CCSDT's."""
    o, v = 4, 5
    rng = np.random.default_rng(11)
    g = _random_g(o + v, rng)
    f_ov = rng.uniform(-0.5, 0.5, (o, v))
    l1, l2 = T.random_so_amplitudes(o, v, 12)
    X = LT.random_antisymmetric_triples(o, v, 13)
    assert np.max(np.abs(X + X.transpose(1, 0, 2, 3, 4, 5))) < 1e-15 and np.max(np.abs(X + X.transpose(0, 1, 2, 3, 5, 4))) < 1e-15
    lhs, rhs = LT.left_contraction(g, o, l1, l2, f_ov, X), LT.functional(g, f_ov, l1, l2, X)
    assert abs(rhs) > 1.0                                   # (a sum of a few thousand products of order one: nothing to hide behind)
    assert abs(lhs - rhs) <= 1e-12 * abs(rhs), (lhs, rhs)
    # each part alone: the singles feed, the f_ov term, the two doubles feeds
    zero1, zero2, zerof = np.zeros_like(l1), np.zeros_like(l2), np.zeros_like(f_ov)
    for a1, a2, ff in ((l1, zero2, f_ov), (zero1, l2, zerof), (zero1, l2, f_ov)):
        lhs, rhs = LT.left_contraction(g, o, a1, a2, ff, X), LT.functional(g, ff, a1, a2, X)
        assert abs(rhs) > 1e-2 and abs(lhs - rhs) <= 1e-12 * abs(rhs), (lhs, rhs)


@pytest.mark.parametrize("n,na,nb,fock", T.SO_CASES)
def test_lambda_equal_to_t_is_the_triples_correction(n, na, nb, fock):
    """(ii) with l = t the expression is (T) term for term"""
    c = T.so_case(n, na, nb, fock)
    val, S = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, c.t1, c.t2, c.f_ov)
    assert np.all(np.abs(val - c.val) <= LD(1e-18) * c.S), np.max(np.abs(val - c.val) / c.S)
    assert np.all(np.abs(S - c.S) <= LD(1e-18) * c.S)


@pytest.mark.parametrize("n,na,nb,fock", T.SO_CASES)
def test_no_value_is_cancelled_away_with_the_gpu_tests_lambda(n, na, nb, fock):
    """(iii) the condition test_triples_cpu.py puts on the (T) cases: the tolerance is at most 1e-3 of every triple's value"""
    c = T.so_case(n, na, nb, fock)
    l1, l2 = T.random_so_amplitudes(c.o, c.v, LT.lambda_seed(c.n, c.o))
    assert np.max(np.abs(l2 - c.t2)) > 0.1
    val, S = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, l1, l2, c.f_ov)
    assert len(val) == len(T.so_order(c.o))
    r = (np.abs(val) / S).astype(np.float64)
    print("smallest |value| / majorant", r.min())
    assert np.all(r >= 1e3 * T.tol_factor(c.o, c.v)), r.min()
    assert abs(np.sum(val)) >= 1e6 * T.tol_factor(c.o, c.v) * np.sum(S)
    if fock:   # the f_ov l2 term is far above the tolerance on every triple
        plain, _ = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, l1, l2, None)
        assert np.all(np.abs(plain - val) > 1e6 * T.tol_factor(c.o, c.v) * S)


def test_linear_in_lambda_and_zero_without_it():
    """(iv)"""
    c = T.so_case(*T.SO_CASES[2])
    a1, a2 = T.random_so_amplitudes(c.o, c.v, 3)
    b1, b2 = T.random_so_amplitudes(c.o, c.v, 4)
    va, Sa = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, a1, a2, c.f_ov)
    vb, Sb = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, b1, b2, c.f_ov)
    vc, _ = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, a1 + 2.0 * b1, a2 + 2.0 * b2, c.f_ov)
    assert np.all(np.abs(vc - (va + 2 * vb)) <= LD(1e-17) * (Sa + 2 * Sb))
    v0, S0 = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, 0.0 * a1, 0.0 * a2, c.f_ov)
    assert not np.any(v0) and not np.any(S0)
    # ... and not linear in t alone: the right factor carries t2 only, the left factor none of t
    vt, _ = LT.lt_per_triple(c.g, c.lev, c.o, 3.0 * c.t1, c.t2, a1, a2, c.f_ov)
    assert np.all(np.abs(vt - va) <= LD(1e-17) * Sa)


def test_library_header_and_wrappers_export_the_call():
    """(v)"""
    name = "afesp_ccsd_so_lambda_t"
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(lib, name) and name in capi.EXPORTS
    assert getattr(capi.load_library(), name).argtypes is not None
    out = ctypes.c_double(7.0)
    lib.afesp_ccsd_so_lambda_t.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]
    assert lib.afesp_ccsd_so_lambda_t(None, 0, 1, ctypes.byref(out)) == 1 and out.value == 7.0    # a NULL context is an argument error
    header = open(os.path.join(ROOT, "include", "afesp.h")).read()
    assert f"int {name}(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double* e_lt);" in header
    f90 = open(os.path.join(ROOT, "a-fortran-electronic-structure-program_amd", "host", "afesp_capi.f90")).read()
    assert f"bind(C, name='{name}')" in f90
    assert callable(capi.Engine.so_lambda_t) and callable(density.so_lambda_t_correction)


def test_cc_lambda_t_key_is_taken_where_cc_density_is_and_on_a_uhf_fcidump(tmp_path):
    def write(body):
        (tmp_path / "els.in").write_text("&elsinput\n" + body + "\n/\n")
        return str(tmp_path / "els.in")
    assert inputs.read_els_in(write('calc_type="UCCSD"')).cc_lambda_t is False
    for calc in inputs.CC_DENSITY_TYPES:
        assert inputs.read_els_in(write(f'calc_type="{calc}",\ncc_lambda_t=.true.')).cc_lambda_t is True
    assert inputs.read_els_in(write('calc_type="UCCSD(T)",\ncc_lambda_t=.true.,\nfcidump_in=.true.')).cc_lambda_t is True   # no overlap needed
    bad = ("CCSD_spatial", "CCSD(T)_spatial", "CRCCSD(T)_spatial", "MP2_spinorb", "UMP2", "RHF")
    for calc in bad:
        with pytest.raises(ValueError, match="takes no cc_lambda_t"):
            inputs.read_els_in(write(f'calc_type="{calc}",\ncc_lambda_t=.true.'))
    with pytest.raises(ValueError):
        inputs.read_els_in(write('calc_type="UCCSD",\ncc_lambda_t=3'))
    if not os.path.exists(HOST_EXE):
        pytest.skip("els_amd not built")
    for calc in bad + ("ROHF-MP2",):
        write(f'calc_type="{calc}",\ncc_lambda_t=.true.' + (",\nfcidump_in=.true." if calc.startswith("ROHF") else ""))
        res = subprocess.run([HOST_EXE], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert res.returncode != 0 and f"{calc} takes no cc_lambda_t" in res.stderr, (calc, res.stderr)
        assert "system::read_system_in" in res.stderr
