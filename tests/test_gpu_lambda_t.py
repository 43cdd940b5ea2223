"""Lambda-CCSD(T) on the device (afesp_ccsd_so_lambda_t: csrc/triples.hip so_lambda_triples, csrc/triples_orbit.h
triples_so_lambda_orbit_kernel) triple by triple against np_lambda_t.py, on the spin-orbital cases of np_triples.py with t and Lambda
amplitudes of order one handed in (so_set_amplitudes, so_lambda_init, so_set_lambda: no solve), under both GEMM back ends.

Tolerance, per range: |engine - reference| <= (2 (v + o) + 64) 2^-53 S, S the reference's majorant summed over the range
(np_triples.tol_factor): the expression has the two-factor, K-term structure of (T), for which that bound is derived.
Largest error / bound seen on an MI355X: 9e-4 (the bound is a worst case over summation orders; it is not tuned to this figure)."""
import functools
import re

import numpy as np
import pytest

import np_lambda_t as LT
import np_triples as T
from afesp_amd import density
from afesp_amd.capi import AfespError

pytestmark = pytest.mark.gpu

KERNELS = {"tgemm": {}, "gett": {"AFESP_T_GEMM": "gett"}}
DEBUG_LINE = re.compile(r"afesp Lambda-\(T\): o (\d+) v (\d+) triples (\d+) per chunk (\d+) chunks (\d+) kernel (\w+)")


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _knobs(monkeypatch, kernel, **more):
    for k, val in dict(KERNELS[kernel], **more).items():
        monkeypatch.setenv(k, str(val))


@functools.lru_cache(maxsize=None)
def _reference(n, na, nb, fock, seed=None):
    """(l1, l2, val, S) of one case: the Lambda amplitudes of seed (default: the seed test_lambda_t_cpu.py checks) and the per-triple reference"""
    c = T.so_case(n, na, nb, fock)
    l1, l2 = T.random_so_amplitudes(c.o, c.v, LT.lambda_seed(c.n, c.o) if seed is None else seed)
    val, S = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, l1, l2, c.f_ov)
    return l1, l2, val, S


def _load(eng, c):
    """the state of case c with its t amplitudes and a Lambda state with l = t; the closed-shell entry as published (Lambda refuses the other)"""
    n, o = c.n, c.o
    if c.fock:
        eng.do_mp2_spatial(n, c.na, np.eye(n), c.e, c.eri, want_eri_mo=False)     # leaves the AO (= MO) integrals resident
        eng.mo_rotate_uhf(n, np.eye(n), np.eye(n))
        eng.uso_init_fock(n, c.na, c.nb, c.fa, c.fb, 2)
        assert np.array_equal(eng.so_tensor("f_ov"), c.f_ov)
    else:
        eng.init_cc_spinorb(n, o, c.e, c.eri, 2, foo_as_published=True)
    assert (eng.so_o, eng.so_v) == (c.o, c.v)
    assert np.max(np.abs(eng.so_tensor("oovv") - c.g[:o, :o, o:, o:])) < 1e-14
    eng.so_set_amplitudes(c.t1, c.t2)
    eng.so_lambda_init(2)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n,na,nb,fock", T.SO_CASES)
def test_lambda_triples_one_by_one(eng, n, na, nb, fock, kernel, monkeypatch):
    """Every i < j < k alone, the whole list and a ragged three-part split; l = t right after the init against (T) of the same range; a new
    Lambda under the cached operand copies; a new t refused until the next init; (T) untouched by the call."""
    _knobs(monkeypatch, kernel)
    c = T.so_case(n, na, nb, fock)
    l1, l2, val, S = _reference(n, na, nb, fock)
    _load(eng, c)
    nt = len(val)
    assert eng.so_ntriples() == nt
    tol = T.tol_factor(c.o, c.v)
    worst = 0.0
    # ---- l = t: (T) itself, within the two bounds added
    e_t = eng.do_ccsd_t_spinorb(0, nt)
    assert abs(e_t - float(np.sum(c.val))) <= tol * float(np.sum(c.S))
    for a, b in ((0, nt), (1, 2), (nt // 3, nt - 1)):
        bound = tol * float(np.sum(c.S[a:b]))
        assert abs(eng.so_lambda_t(a, b) - eng.do_ccsd_t_spinorb(a, b)) <= 2 * bound, (a, b)
    assert eng.do_ccsd_t_spinorb(0, nt) == e_t                      # bit for bit after Lambda-(T) calls
    # ---- Lambda of its own
    eng.so_set_lambda(l1, l2)

    def run(a, b, val=val, S=S):
        nonlocal worst
        out = eng.so_lambda_t(a, b)
        ref, bound = float(np.sum(val[a:b])), tol * float(np.sum(S[a:b]))
        print((a, b), "error / bound", abs(out - ref) / bound)
        assert abs(out - ref) <= bound, (a, b, T.so_order(c.o)[a:b][:3], out, ref, abs(out - ref) / bound)
        worst = max(worst, abs(out - ref) / bound)
        return out, bound

    whole, bound = run(0, nt)
    ones = sum(run(t, t + 1)[0] for t in range(nt))
    assert abs(ones - whole) <= 2 * bound
    thirds = run(0, nt // 3)[0] + run(nt // 3, nt - 1)[0] + run(nt - 1, nt)[0]
    assert abs(thirds - whole) <= 2 * bound
    assert eng.so_lambda_t(2, 2) == 0.0 and eng.so_lambda_t(nt, nt + 5) == 0.0
    assert eng.do_ccsd_t_spinorb(0, nt) == e_t
    # ---- a new Lambda under the cached operand copies and plan follows the new reference
    m1, m2, val2, S2 = _reference(n, na, nb, fock, 7)
    eng.so_set_lambda(m1, m2)
    out2 = run(0, nt, val2, S2)[0]
    assert abs(out2 - whole) > 1e3 * bound
    eng.so_set_lambda(m1, l2)                                       # (l2 alone changes: the copies follow)
    val3, S3 = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, m1, l2, c.f_ov)
    run(0, nt, val3, S3)
    # ---- a new t: refused until the Lambda state is made again, then served with l = t
    t1, t2 = T.random_so_amplitudes(c.o, c.v, 5)
    eng.so_set_amplitudes(t1, t2)
    with pytest.raises(AfespError, match="status 21: .*stale"):
        eng.so_lambda_t(0, nt)
    eng.so_lambda_init(2)
    vt, St = T.so_per_triple(c.g, c.lev, c.o, t1, t2, c.f_ov)
    assert abs(eng.so_lambda_t(0, nt) - float(np.sum(vt))) <= tol * float(np.sum(St))
    print(f"largest error / bound (Lambda-(T)): {worst:.4f}")


@pytest.mark.parametrize("n,na,nb,fock", [T.SO_CASES[0], T.SO_CASES[3]])
def test_lambda_residual_and_iteration_do_not_see_the_call(eng, n, na, nb, fock):
    """so_lambda() and one so_lambda_iterate give the same bits whether or not Lambda-(T) ran in between: no scratch name collides, nothing
    of the Lambda state is written."""
    c = T.so_case(n, na, nb, fock)
    l1, l2, _, _ = _reference(n, na, nb, fock)
    _load(eng, c)
    eng.so_set_lambda(l1, l2)
    step_a = eng.so_lambda_iterate(1e-11, 1e-11)
    lam_a = eng.so_lambda()
    eng.so_lambda_init(2)
    eng.so_set_lambda(l1, l2)
    e_lt = eng.so_lambda_t()
    b1, b2 = eng.so_lambda()
    assert np.array_equal(b1, l1) and np.array_equal(b2, l2)
    t1, t2 = eng.so_amplitudes()
    assert np.array_equal(t1, c.t1) and np.array_equal(t2, c.t2)
    step_b = eng.so_lambda_iterate(1e-11, 1e-11)
    lam_b = eng.so_lambda()
    assert step_a == step_b
    assert np.array_equal(lam_a[0], lam_b[0]) and np.array_equal(lam_a[1], lam_b[1])
    # the iteration wrote Lambda: the next call follows it (the stamp of the operand copies), and differs from the one before
    val, S = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, lam_b[0], lam_b[1], c.f_ov)
    out = eng.so_lambda_t()
    assert abs(out - float(np.sum(val))) <= T.tol_factor(c.o, c.v) * float(np.sum(S))
    assert abs(out - e_lt) > 1e3 * T.tol_factor(c.o, c.v) * float(np.sum(S))
    d_a = eng.so_density()
    eng.so_lambda_t(0, 2)
    assert np.array_equal(eng.so_density(), d_a)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n,na,nb,fock", [T.SO_CASES[1], T.SO_CASES[2]])
def test_more_than_one_chunk(eng, n, na, nb, fock, kernel, monkeypatch, capfd):
    """A pool budget of nothing (AFESP_T_POOL_GIB=0) makes a chunk per triple: the second pool's blocks and the descriptor offsets past
    chunk 0, against the reference and the one-chunk evaluation."""
    c = T.so_case(n, na, nb, fock)
    l1, l2, val, S = _reference(n, na, nb, fock)
    _knobs(monkeypatch, kernel, AFESP_T_DEBUG=1)
    _load(eng, c)
    eng.so_set_lambda(l1, l2)
    nt = len(val)
    capfd.readouterr()
    one = eng.so_lambda_t()
    e_t = eng.do_ccsd_t_spinorb()
    dbg = [m.groups() for m in DEBUG_LINE.finditer(capfd.readouterr().err)]
    assert dbg == [(str(c.o), str(c.v), str(nt), str(nt), "1", "tgemm" if kernel == "tgemm" and T.kc(c.o, c.v) >= 32 else "gett")], dbg
    monkeypatch.setenv("AFESP_T_POOL_GIB", "0")
    many = eng.so_lambda_t()
    dbg = [m.groups() for m in DEBUG_LINE.finditer(capfd.readouterr().err)]
    assert len(dbg) == 1 and dbg[0][3] == "1" and int(dbg[0][4]) == nt > 1, dbg
    bound = T.tol_factor(c.o, c.v) * float(np.sum(S))
    assert abs(many - float(np.sum(val))) <= bound and abs(many - one) <= 2 * bound
    part = eng.so_lambda_t(1, nt - 1)
    assert abs(part - float(np.sum(val[1:nt - 1]))) <= T.tol_factor(c.o, c.v) * float(np.sum(S[1:nt - 1]))
    e_t_many = eng.do_ccsd_t_spinorb()
    assert abs(e_t_many - e_t) <= 2 * T.tol_factor(c.o, c.v) * float(np.sum(c.S))
    monkeypatch.delenv("AFESP_T_POOL_GIB")
    assert eng.so_lambda_t() == one and eng.do_ccsd_t_spinorb() == e_t      # the default plan again: the same bits


def test_errors_leave_the_engine_usable(eng):
    from afesp_amd.capi import Engine
    from test_gpu_lambda import _case, _feed
    c = T.so_case(*T.SO_CASES[0])
    with Engine(0) as fresh:                                           # no state at all
        fresh.so_o, fresh.so_v = c.o, c.v
        with pytest.raises(AfespError, match="status 1: .*no converged spin-orbital CCSD state"):
            fresh.so_lambda_t()
    eng.init_cc_spinorb(c.n, c.o, c.e, c.eri, 2, foo_as_published=True)
    eng.so_set_amplitudes(c.t1, c.t2)
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):   # no Lambda state
        eng.so_lambda_t()
    e_t = eng.do_ccsd_t_spinorb()                                      # ... and the engine serves
    eng.so_lambda_init(2)
    assert eng.so_lambda_t(3, 3) == 0.0 and eng.so_lambda_t(-4, 0) == 0.0   # empty ranges
    bound = T.tol_factor(c.o, c.v) * float(np.sum(c.S))
    assert abs(eng.so_lambda_t() - e_t) <= 2 * bound
    f = _case("fock_rotated")                                          # a Fock state whose f_oo is not diagonal
    _feed(eng, f)
    foo = eng.so_tensor("f_oo")
    assert np.max(np.abs(foo - np.diag(np.diag(foo)))) > 1e-3
    eng.so_lambda_init(2)
    with pytest.raises(AfespError, match="status 1: .*not diagonal"):
        eng.so_lambda_t()
    eng.so_lambda_iterate()                                            # the Lambda state is still served
    _load(eng, c)
    assert abs(eng.so_lambda_t() - e_t) <= 2 * bound


def test_converged_amplitudes(eng):
    """Converged CCSD and converged Lambda on the o, v = 4, 6 shape of test_gpu_lambda.py: the value at the fetched amplitudes, and the
    helper of afesp_amd.density (which solves Lambda itself where there is none)."""
    from test_gpu_lambda import _case, _feed
    c = _case("rhf_fed")
    o, v = c["o"], c["v"]
    assert (o, v) == (4, 6)
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    e_lt, e_t = density.so_lambda_t_correction(eng, maxiter=300, e_tol=1e-11, l_tol=1e-11)      # no Lambda state yet: solved here
    t1, t2 = eng.so_amplitudes()
    l1, l2 = eng.so_lambda()
    assert np.max(np.abs(l2 - t2)) > 1e-6                              # Lambda was iterated away from its start
    lev = np.diag(c["f"]).copy()
    val, S = LT.lt_per_triple(c["g"], lev, o, t1, t2, l1, l2)
    tol = T.tol_factor(o, v)
    print("E(Lambda-T)", e_lt, "E(T)", e_t, "reference", float(np.sum(val)))
    assert abs(e_lt - float(np.sum(val))) <= tol * float(np.sum(S))
    vt, St = T.so_per_triple(c["g"], lev, o, t1, t2)
    assert abs(e_t - float(np.sum(vt))) <= tol * float(np.sum(St))
    assert abs(e_lt - e_t) > 1e3 * tol * float(np.sum(S))
    # a live Lambda state is used as it stands: the same bits, no second solve
    assert density.so_lambda_t_correction(eng) == (e_lt, e_t)
    nt = eng.so_ntriples()
    parts = density.so_lambda_t_correction(eng, 0, nt // 2)[0] + density.so_lambda_t_correction(eng, nt // 2, nt)[0]
    assert abs(parts - e_lt) <= 2 * tol * float(np.sum(S))
