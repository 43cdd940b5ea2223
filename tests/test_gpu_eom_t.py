"""The triples correction to EOM-EE-CCSD excitation energies on the device (afesp_ccsd_so_eom_t: csrc/triples.hip so_eom_triples and
eom_t_build_right_kernel, csrc/triples_orbit.h triples_so_eom_orbit_kernel) triple by triple against np_eom_t.py, on the four spin-orbital
cases of np_triples.py with t2 and left / right vectors of order one handed in (no solve), under both GEMM back ends.

Tolerance, per range: |engine - reference| <= (4 (v + o) + 2 (v + 2 o) + 64) 2^-53 S, S the reference's majorant summed over the range
(np_eom_t.tol_factor): two roundings per term of every nested sum -- outer sums over the concatenated index of length 2 (v + o), the
elements of gR sums of at most v + 2 o products.  It is not tuned to the kernel; largest error / bound seen on an MI355X: 6e-5."""
import functools

import numpy as np
import pytest

import np_eom_t as ET
import np_lambda_t as LT
import np_triples as T
from afesp_amd import eom
from afesp_amd.capi import AfespError
from test_gpu_lambda_t import KERNELS, _knobs, _load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _reference(n, na, nb, fock):
    """(omega[2], L, R, val[2][nt], S[2][nt]) of one case: two states (the vectors test_eom_t_cpu.py checks) and their per-triple references"""
    c = T.so_case(n, na, nb, fock)
    omega, L, R = ET.case_vectors(c, 2)
    per = [ET.eom_t_per_triple(c.g, c.lev, c.o, c.t2, omega[s], *L[s], *R[s], c.f_ov) for s in range(2)]
    return omega, L, R, [p[0] for p in per], [p[1] for p in per]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n,na,nb,fock", T.SO_CASES)
def test_eom_triples_one_by_one(eng, n, na, nb, fock, kernel, monkeypatch):
    """Every i < j < k alone, the whole list and a ragged three-part split against np_eom_t; two states in one call equal two calls."""
    _knobs(monkeypatch, kernel)
    c = T.so_case(n, na, nb, fock)
    omega, L, R, val, S = _reference(n, na, nb, fock)
    _load(eng, c)
    nt = len(val[0])
    assert eng.so_ntriples() == nt
    tol = ET.tol_factor(c.o, c.v)
    worst = 0.0

    def run(a, b):
        nonlocal worst
        out = eng.so_eom_t(omega, L, R, a, b)
        for s in range(2):
            ref, bound = float(np.sum(val[s][a:b])), tol * float(np.sum(S[s][a:b]))
            print((a, b), s, "error / bound", abs(out[s] - ref) / bound if bound else 0.0)
            assert abs(out[s] - ref) <= bound, (a, b, s, out[s], ref, abs(out[s] - ref) / bound)
            worst = max(worst, abs(out[s] - ref) / bound)
        return out, np.array([tol * float(np.sum(S[s][a:b])) for s in range(2)])

    whole, bound = run(0, nt)
    ones = sum(run(t, t + 1)[0] for t in range(nt))
    assert np.all(np.abs(ones - whole) <= 2 * bound)
    thirds = run(0, nt // 3)[0] + run(nt // 3, nt - 1)[0] + run(nt - 1, nt)[0]
    assert np.all(np.abs(thirds - whole) <= 2 * bound)
    # two states in one call = two calls, in either order
    for s in (1, 0):
        one = eng.so_eom_t(omega[s:s + 1], L[s:s + 1], R[s:s + 1])
        assert one.shape == (1,) and one[0] == whole[s]
    assert np.all(eng.so_eom_t(omega, L, R, 2, 2) == 0.0) and np.all(eng.so_eom_t(omega, L, R, nt, nt + 5) == 0.0)
    print(f"largest error / bound (EOM-(T)): {worst:.4f}")


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n,na,nb,fock", T.SO_CASES)
def test_lambda_t_limit(eng, n, na, nb, fock, kernel, monkeypatch):
    """omega = 0, l = lambda, r = (0, t2) is Lambda-CCSD(T): within the sum of both bounds"""
    _knobs(monkeypatch, kernel)
    c = T.so_case(n, na, nb, fock)
    _load(eng, c)
    l1, l2 = T.random_so_amplitudes(c.o, c.v, LT.lambda_seed(c.n, c.o))
    eng.so_set_lambda(l1, l2)
    _, S = LT.lt_per_triple(c.g, c.lev, c.o, c.t1, c.t2, l1, l2, c.f_ov, dtype=np.float64)
    nt = len(S)
    for a, b in ((0, nt), (1, 2), (nt // 3, nt - 1)):
        bound = (ET.tol_factor(c.o, c.v) + T.tol_factor(c.o, c.v)) * float(np.sum(S[a:b]))
        out = eng.so_eom_t([0.0], [(l1, l2)], [(np.zeros_like(c.t1), c.t2)], a, b)[0]
        ref = eng.so_lambda_t(a, b)
        print((a, b), out, ref, abs(out - ref) / bound)
        assert abs(out - ref) <= bound, (a, b, out, ref)


@pytest.mark.parametrize("n,na,nb,fock", [T.SO_CASES[0], T.SO_CASES[3]])
def test_no_side_effects(eng, n, na, nb, fock):
    """(T), Lambda-(T), the Lambda residual step and an EOM sigma give the same bits before and after the call; t and lambda are not written"""
    c = T.so_case(n, na, nb, fock)
    omega, L, R, _, _ = _reference(n, na, nb, fock)
    l1, l2 = T.random_so_amplitudes(c.o, c.v, LT.lambda_seed(c.n, c.o))

    def probes():
        _load(eng, c)
        eng.so_set_lambda(l1, l2)
        eng.so_eom_init(2, 8)
        return eng

    probes()
    before = [eng.do_ccsd_t_spinorb(), eng.so_lambda_t(), eng.so_eom_sigma(*R[0])]
    step_a = eng.so_lambda_iterate(1e-11, 1e-11)
    lam_a = eng.so_lambda()
    probes()
    a0 = [eng.do_ccsd_t_spinorb(), eng.so_lambda_t()]
    eng.so_eom_t(omega, L, R)
    eng.so_eom_t(omega, L, R, 1, 3)
    after = [eng.do_ccsd_t_spinorb(), eng.so_lambda_t(), eng.so_eom_sigma(*R[0])]
    assert a0 == before[:2] and after[:2] == before[:2]
    assert all(np.array_equal(x, y) for x, y in zip(after[2], before[2]))
    t1, t2 = eng.so_amplitudes()
    assert np.array_equal(t1, c.t1) and np.array_equal(t2, c.t2)
    b1, b2 = eng.so_lambda()
    assert np.array_equal(b1, l1) and np.array_equal(b2, l2)
    step_b = eng.so_lambda_iterate(1e-11, 1e-11)
    lam_b = eng.so_lambda()
    assert step_a == step_b and np.array_equal(lam_a[0], lam_b[0]) and np.array_equal(lam_a[1], lam_b[1])


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n,na,nb,fock", [T.SO_CASES[1], T.SO_CASES[2]])
def test_a_chunk_per_triple(eng, n, na, nb, fock, kernel, monkeypatch, capfd):
    """AFESP_T_POOL_GIB=0: a chunk per triple (both pools' blocks and the descriptor offsets past chunk 0), against the reference and the
    one-chunk evaluation; the default plan afterwards gives the first bits again"""
    import re
    c = T.so_case(n, na, nb, fock)
    omega, L, R, val, S = _reference(n, na, nb, fock)
    _knobs(monkeypatch, kernel, AFESP_T_DEBUG=1)
    _load(eng, c)
    nt = len(val[0])
    one = eng.so_eom_t(omega, L, R)
    capfd.readouterr()
    monkeypatch.setenv("AFESP_T_POOL_GIB", "0")
    many = eng.so_eom_t(omega, L, R)
    dbg = re.findall(r"afesp EOM-\(T\): o \d+ v \d+ states (\d+) triples (\d+) per chunk (\d+) chunks (\d+) kernel (\w+)", capfd.readouterr().err)
    assert dbg == [("2", str(nt), "1", str(nt), "tgemm" if kernel == "tgemm" and T.kc(c.o, c.v) >= 32 else "gett")], dbg
    part = eng.so_eom_t(omega, L, R, 1, nt - 1)
    tol = ET.tol_factor(c.o, c.v)
    for s in range(2):
        bound = tol * float(np.sum(S[s]))
        assert abs(many[s] - float(np.sum(val[s]))) <= bound and abs(many[s] - one[s]) <= 2 * bound
        assert abs(part[s] - float(np.sum(val[s][1:nt - 1]))) <= tol * float(np.sum(S[s][1:nt - 1]))
    monkeypatch.delenv("AFESP_T_POOL_GIB")
    assert np.array_equal(eng.so_eom_t(omega, L, R), one)


def test_statuses(eng):
    import ctypes as C
    from afesp_amd.capi import Engine
    from test_gpu_lambda import _case, _feed
    c = T.so_case(*T.SO_CASES[0])
    omega, L, R, val, S = _reference(*T.SO_CASES[0])
    with Engine(0) as fresh:                                           # no state at all
        fresh.so_o, fresh.so_v = c.o, c.v
        with pytest.raises(AfespError, match="status 1: .*no converged spin-orbital CCSD state"):
            fresh.so_eom_t(omega, L, R, 0, 4)
    eng.init_cc_spinorb(c.n, c.o, c.e, c.eri, 2, foo_as_published=True)
    eng.so_set_amplitudes(c.t1, c.t2)                                  # no Lambda state: none is needed
    out = eng.so_eom_t(omega, L, R)
    tol = ET.tol_factor(c.o, c.v)
    assert all(abs(out[s] - float(np.sum(val[s]))) <= tol * float(np.sum(S[s])) for s in range(2))
    with pytest.raises(AfespError, match="status 1: .*nstates < 1 or a NULL argument"):
        eng.so_eom_t([], [], [])
    x = np.zeros(c.o * c.o * c.v * c.v)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d = np.full(1, 7.0)
    assert eng.L.afesp_ccsd_so_eom_t(eng.h, 1, p(x), None, p(x), p(x), p(x), 0, 4, p(d)) == 1 and d[0] == 7.0
    assert eng.L.afesp_ccsd_so_eom_t(eng.h, 1, p(x), p(x), p(x), p(x), p(x), 0, 4, None) == 1
    assert np.all(eng.so_eom_t(omega, L, R, 3, 3) == 0.0) and np.all(eng.so_eom_t(omega, L, R, -4, 0) == 0.0)   # empty ranges
    f = _case("fock_rotated")                                          # a Fock state whose f_oo is not diagonal
    _feed(eng, f)
    o, v = eng.so_o, eng.so_v
    z = [(np.zeros((o, v)), np.zeros((o, o, v, v)))]
    with pytest.raises(AfespError, match="status 1: .*not diagonal"):
        eng.so_eom_t([0.1], z, z)
    # o < 3: zeros
    import molecules
    _, e2, eri2 = molecules.synthetic_system(1, 3, scale=T.SCALE, seed=11)
    eng.init_cc_spinorb(4, 2, e2, eri2, 2, foo_as_published=True)
    z = [(np.ones((2, 6)), np.ones((2, 2, 6, 6)))]
    assert np.all(eng.so_eom_t([0.1], z, z) == 0.0)
    eng.init_cc_spinorb(c.n, c.o, c.e, c.eri, 2, foo_as_published=True)   # ... and the engine serves
    eng.so_set_amplitudes(c.t1, c.t2)
    assert np.array_equal(eng.so_eom_t(omega, L, R), out)


def test_converged_vectors(eng):
    """Converged CCSD, Lambda, right and left EOM-CCSD for three roots at o, v = 4, 6 (test_gpu_lambda.py's shape), biorthonormalised: the
    device's delta against numpy at the fetched vectors; the three components of the lowest triplet get the same delta to 1e-8."""
    from afesp_amd import density
    from test_gpu_lambda import _case, _feed
    c = _case("rhf_fed")
    o, v = c["o"], c["v"]
    assert (o, v) == (4, 6)
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    density.so_lambda_solve(eng, maxiter=300, e_tol=1e-11, l_tol=1e-11)
    omega, R, info = eom.so_eom_solve(eng, 3, tol=1e-9)
    wl, Lv, _ = eom.so_eom_left_solve(eng, R, tol=1e-9)
    assert np.max(np.abs(wl - omega)) < 1e-7
    Lb = eom.biorthonormalise(omega, Lv, R)
    delta, corrected, tinfo = eom.so_eom_triples_correction(eng, omega, Lb, R)
    t1, t2 = eng.so_amplitudes()
    lev = np.diag(c["f"]).copy()
    tol = ET.tol_factor(o, v)
    for k in range(3):
        val, S = ET.eom_t_per_triple(c["g"], lev, o, t2, omega[k], *Lb[k], *R[k])
        print("root", k, "omega", omega[k], "delta", delta[k], "reference", float(np.sum(val)), "gap", tinfo["min_gap"][k])
        assert abs(delta[k] - float(np.sum(val))) <= tol * float(np.sum(S))
    assert np.allclose(corrected, omega + delta, rtol=0, atol=0)
    eo, ev = np.sort(lev[:o]), np.sort(lev[o:])
    assert np.allclose(tinfo["min_gap"], np.abs(omega - (ev[:3].sum() - eo[-3:].sum())), rtol=0, atol=1e-12)
    triplets = [cl for cl in eom.clusters(omega) if len(cl) == 3]
    assert triplets, (omega, info["degeneracy"])                            # the lowest root of this closed-shell case is a triplet
    for cl in triplets:
        assert np.max(delta[cl]) - np.min(delta[cl]) < 1e-8, (cl, delta)
    nt = eng.so_ntriples()
    parts = eng.so_eom_t(omega, Lb, R, 0, nt // 2) + eng.so_eom_t(omega, Lb, R, nt // 2, nt)
    assert np.max(np.abs(parts - delta)) < 1e-12
    with pytest.raises(ValueError, match="biorthonormalise"):
        eom.so_eom_triples_correction(eng, omega, Lv, [(2 * r[0], 2 * r[1]) for r in R])
