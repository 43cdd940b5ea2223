"""The triples correction to EOM-IP-CCSD and EOM-EA-CCSD roots on the device (afesp_ccsd_so_eom_ipea_t: csrc/eom_ipea_t_so.hip) item by
item against np_eom_ipea_t.py (the ghost embedding on np_eom_t), on the four spin-orbital cases of np_triples.py and the smallest extents
that can be loaded (np_eom_ipea_t.MINIMAL_CASES), with t2 and left / right vectors of order one handed in (no solve).  Every product runs
through contract(): there is one GEMM back end here, so nothing is parametrised over kernels.

Tolerance, per range: |engine - reference| <= (4 (v + o) + 2 o + 64) 2^-53 S for IP and (4 (v + o) + 2 v + 64) 2^-53 S for EA, S the
reference's majorant summed over the range (np_eom_ipea_t.tol_factor): two roundings per term of every nested sum -- outer sums of length
v + o on either side, the elements of U and Y sums of o (IP) or v (EA) products.  It is not tuned to the kernels."""
import numpy as np
import pytest

import np_eom_ipea_t as Q
import np_lambda_t as LT
import np_triples as T
from afesp_amd import eom
from afesp_amd.capi import AfespError
from test_gpu_lambda_t import _load

pytestmark = pytest.mark.gpu
IP, EA = Q.IP, Q.EA
SECTORS = {"ip": IP, "ea": EA}
CASES = [(name, c) for name, sec in SECTORS.items() for c in Q.cases(sec)]


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("sector,case", CASES)
def test_items_one_by_one(eng, sector, case):
    """Every item alone, the whole list and a ragged three-part split against the reference; two states in one call equal two calls; a
    second call returns the same bits."""
    sec = SECTORS[sector]
    c = T.so_case(*case)
    omega, L, R, val, S = Q.reference(sec, *case)
    _load(eng, c)
    ni = len(val[0])
    assert eng.so_eom_ipea_t_nitems(sec) == ni == Q.nitems(sec, c.o)
    assert np.allclose(eng.so_abs_levels(), c.lev, rtol=0, atol=1e-14)       # (what the drivers' min_gap reads)
    tol = Q.tol_factor(sec, c.o, c.v)
    worst = 0.0

    def run(a, b):
        nonlocal worst
        out = eng.so_eom_ipea_t(sec, omega, L, R, a, b)
        for s in range(2):
            ref, bound = float(np.sum(val[s][a:b])), tol * float(np.sum(S[s][a:b]))
            print((a, b), s, "error / bound", abs(out[s] - ref) / bound if bound else 0.0)
            assert abs(out[s] - ref) <= bound, (a, b, s, out[s], ref, abs(out[s] - ref) / bound)
            worst = max(worst, abs(out[s] - ref) / bound if bound else 0.0)
        return out, np.array([tol * float(np.sum(S[s][a:b])) for s in range(2)])

    whole, bound = run(0, ni)
    assert np.array_equal(eng.so_eom_ipea_t(sec, omega, L, R), whole)
    ones = sum(run(t, t + 1)[0] for t in range(ni))
    assert np.all(np.abs(ones - whole) <= 2 * bound)
    thirds = run(0, ni // 3)[0] + run(ni // 3, ni - 1)[0] + run(ni - 1, ni)[0]
    assert np.all(np.abs(thirds - whole) <= 2 * bound)
    for s in (1, 0):                                                       # two states in one call = two calls, in either order
        one = eng.so_eom_ipea_t(sec, omega[s:s + 1], L[s:s + 1], R[s:s + 1])
        assert one.shape == (1,) and one[0] == whole[s]
    assert np.all(eng.so_eom_ipea_t(sec, omega, L, R, 1, 1) == 0.0) and np.all(eng.so_eom_ipea_t(sec, omega, L, R, ni, ni + 5) == 0.0)
    print(f"largest error / bound (EOM-{sector.upper()}-(T)): {worst:.4f}")


@pytest.mark.parametrize("sector,case", [("ip", T.SO_CASES[1]), ("ip", T.SO_CASES[2]), ("ea", T.SO_CASES[1]), ("ea", T.SO_CASES[2])])
def test_a_chunk_per_item(eng, sector, case, monkeypatch, capfd):
    """AFESP_T_POOL_GIB=0: a chunk per item (the tables' offsets past chunk 0, the groups of one and two images), against the reference and
    the one-chunk evaluation; the default chunking afterwards gives the first bits again"""
    import re
    sec = SECTORS[sector]
    c = T.so_case(*case)
    omega, L, R, val, S = Q.reference(sec, *case)
    monkeypatch.setenv("AFESP_T_DEBUG", "1")
    _load(eng, c)
    ni = len(val[0])
    one = eng.so_eom_ipea_t(sec, omega, L, R)
    line = re.compile(r"afesp EOM-(IP|EA)-\(T\): o \d+ v \d+ states (\d+) items (\d+) per chunk (\d+) chunks (\d+)")
    assert line.findall(capfd.readouterr().err) == [(sector.upper(), "2", str(ni), str(ni), "1")]
    monkeypatch.setenv("AFESP_T_POOL_GIB", "0")
    many = eng.so_eom_ipea_t(sec, omega, L, R)
    assert line.findall(capfd.readouterr().err) == [(sector.upper(), "2", str(ni), "1", str(ni))]
    part = eng.so_eom_ipea_t(sec, omega, L, R, 1, ni - 1)
    tol = Q.tol_factor(sec, c.o, c.v)
    for s in range(2):
        bound = tol * float(np.sum(S[s]))
        assert abs(many[s] - float(np.sum(val[s]))) <= bound and abs(many[s] - one[s]) <= 2 * bound
        assert abs(part[s] - float(np.sum(val[s][1:ni - 1]))) <= tol * float(np.sum(S[s][1:ni - 1]))
    monkeypatch.delenv("AFESP_T_POOL_GIB")
    assert np.array_equal(eng.so_eom_ipea_t(sec, omega, L, R), one)


@pytest.mark.parametrize("case", [T.SO_CASES[0], T.SO_CASES[3]])
def test_no_side_effects(eng, case):
    """(T), Lambda-(T), EOM-(T), a Lambda iteration and an IP / EA sigma and left sigma give the same bits before and after calls of both
    sectors; t and lambda are not written"""
    import np_eom_t as ET
    c = T.so_case(*case)
    ref = {sec: Q.reference(sec, *case) for sec in (IP, EA)}
    l1, l2 = T.random_so_amplitudes(c.o, c.v, LT.lambda_seed(c.n, c.o))
    w_ee, L_ee, R_ee = ET.case_vectors(c, 1)

    def probes():
        _load(eng, c)
        eng.so_set_lambda(l1, l2)

    def sigmas():
        out = []
        for sec in (IP, EA):
            x1, x2 = ref[sec][2][0]
            out += [*eng.so_eom_ipea_sigma(sec, x1, x2), *eng.so_eom_ipea_lsigma(sec, x1, x2)]
        return out

    probes()
    before = [eng.do_ccsd_t_spinorb(), eng.so_lambda_t(), eng.so_eom_t(w_ee, L_ee, R_ee)[0]]
    sig_before = sigmas()
    step_a = eng.so_lambda_iterate(1e-11, 1e-11)
    lam_a = eng.so_lambda()
    probes()
    a0 = [eng.do_ccsd_t_spinorb(), eng.so_lambda_t(), eng.so_eom_t(w_ee, L_ee, R_ee)[0]]
    for sec in (IP, EA):
        omega, L, R = ref[sec][:3]
        eng.so_eom_ipea_t(sec, omega, L, R)
        eng.so_eom_ipea_t(sec, omega, L, R, 1, 3)
    after = [eng.do_ccsd_t_spinorb(), eng.so_lambda_t(), eng.so_eom_t(w_ee, L_ee, R_ee)[0]]
    assert a0 == before and after == before
    assert all(np.array_equal(x, y) for x, y in zip(sigmas(), sig_before))
    t1, t2 = eng.so_amplitudes()
    assert np.array_equal(t1, c.t1) and np.array_equal(t2, c.t2)
    b1, b2 = eng.so_lambda()
    assert np.array_equal(b1, l1) and np.array_equal(b2, l2)
    step_b = eng.so_lambda_iterate(1e-11, 1e-11)
    lam_b = eng.so_lambda()
    assert step_a == step_b and np.array_equal(lam_a[0], lam_b[0]) and np.array_equal(lam_a[1], lam_b[1])


def test_statuses(eng):
    import ctypes as C
    import molecules
    from afesp_amd.capi import Engine
    from test_gpu_lambda import _case, _feed
    case = T.SO_CASES[0]
    c = T.so_case(*case)
    ref = {sec: Q.reference(sec, *case) for sec in (IP, EA)}
    with Engine(0) as fresh:                                               # no state at all
        fresh.so_o, fresh.so_v = c.o, c.v
        for sec in (IP, EA):
            with pytest.raises(AfespError, match="status 1: .*no converged spin-orbital CCSD state"):
                fresh.so_eom_ipea_t(sec, *ref[sec][:3], 0, 4)
    eng.init_cc_spinorb(c.n, c.o, c.e, c.eri, 2, foo_as_published=True)
    eng.so_set_amplitudes(c.t1, c.t2)                                      # no Lambda state and no Davidson state: none is needed
    out = {}
    for sec in (IP, EA):
        omega, L, R, val, S = ref[sec]
        out[sec] = eng.so_eom_ipea_t(sec, omega, L, R)
        tol = Q.tol_factor(sec, c.o, c.v)
        assert all(abs(out[sec][s] - float(np.sum(val[s]))) <= tol * float(np.sum(S[s])) for s in range(2))
        with pytest.raises(AfespError, match="status 1: .*nstates < 1 or a NULL argument"):
            eng.so_eom_ipea_t(sec, [], [], [])
        assert np.all(eng.so_eom_ipea_t(sec, omega, L, R, 3, 3) == 0.0) and np.all(eng.so_eom_ipea_t(sec, omega, L, R, -4, 0) == 0.0)
    omega, L, R = ref[IP][:3]
    for bad in (0, 3, -1):
        with pytest.raises(AfespError, match="status 1: .*sector is neither 1"):
            eng.so_eom_ipea_t(bad, omega, L, R)
        assert eng.so_eom_ipea_t_nitems(bad) == 0
    x = np.zeros(c.o * c.v * c.v + c.o * c.o * c.v)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d = np.full(1, 7.0)
    fn = eng.L.afesp_ccsd_so_eom_ipea_t
    for sec in (IP, EA):
        for hole in range(5):
            args = [p(x)] * 5
            args[hole] = None
            assert fn(eng.h, sec, 1, *args, 0, 4, p(d)) == 1 and d[0] == 7.0
        assert fn(eng.h, sec, 1, p(x), p(x), p(x), p(x), p(x), 0, 4, None) == 1
        assert fn(eng.h, sec, 0, p(x), p(x), p(x), p(x), p(x), 0, 4, p(d)) == 1 and d[0] == 7.0
    f = _case("fock_rotated")                                              # a Fock state whose f_oo is not diagonal
    _feed(eng, f)
    o, v = eng.so_o, eng.so_v
    for sec in (IP, EA):
        z = [(np.zeros(o if sec == IP else v), np.zeros((o, o, v) if sec == IP else (o, v, v)))]
        with pytest.raises(AfespError, match="status 1: .*not diagonal"):
            eng.so_eom_ipea_t(sec, [0.1], z, z)
    # below the minimal extents: zeros.  o, v = 2, 6: IP has no item (a two-electron reference); o, v = 6, 2: EA has no a<b<c
    _, e2, eri2 = molecules.synthetic_system(1, 3, scale=T.SCALE, seed=11)
    eng.init_cc_spinorb(4, 2, e2, eri2, 2, foo_as_published=True)
    assert eng.so_eom_ipea_t_nitems(IP) == 0 and eng.so_eom_ipea_t_nitems(EA) == 1
    assert np.all(eng.so_eom_ipea_t(IP, [0.1], [(np.ones(2), np.ones((2, 2, 6)))], [(np.ones(2), np.ones((2, 2, 6)))]) == 0.0)
    _, e3, eri3 = molecules.synthetic_system(3, 1, scale=T.SCALE, seed=12)
    eng.init_cc_spinorb(4, 6, e3, eri3, 2, foo_as_published=True)
    assert eng.so_eom_ipea_t_nitems(EA) == 15
    assert np.all(eng.so_eom_ipea_t(EA, [0.1], [(np.ones(2), np.ones((6, 2, 2)))], [(np.ones(2), np.ones((6, 2, 2)))]) == 0.0)
    eng.init_cc_spinorb(c.n, c.o, c.e, c.eri, 2, foo_as_published=True)   # ... and the engine serves
    eng.so_set_amplitudes(c.t1, c.t2)
    for sec in (IP, EA):
        assert np.array_equal(eng.so_eom_ipea_t(sec, *ref[sec][:3]), out[sec])


@pytest.mark.parametrize("sector", sorted(SECTORS))
def test_converged_vectors(eng, sector):
    """Converged CCSD, Lambda, right and left vectors of four roots of the sector at o, v = 4, 6 (test_gpu_lambda.py's rhf_fed shape),
    biorthonormalised: the device's delta against numpy at the fetched vectors; the two members of each doublet get the same delta to
    1e-10; shards add up; the driver refuses vectors that are not biorthonormal."""
    from afesp_amd import density
    from test_gpu_lambda import _case, _feed
    sec = SECTORS[sector]
    ip = sec == IP
    c = _case("rhf_fed")
    o, v = c["o"], c["v"]
    assert (o, v) == (4, 6)
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    density.so_lambda_solve(eng, maxiter=300, e_tol=1e-11, l_tol=1e-11)
    omega, R, info = (eom.so_eom_ip_solve if ip else eom.so_eom_ea_solve)(eng, 4, tol=1e-9)
    wl, Lv, _ = (eom.so_eom_ip_left_solve if ip else eom.so_eom_ea_left_solve)(eng, R, tol=1e-9)
    assert np.max(np.abs(wl - omega)) < 1e-8
    Lb = eom.biorthonormalise_ipea(omega, Lv, R)
    correct = eom.so_eom_ip_triples_correction if ip else eom.so_eom_ea_triples_correction
    delta, corrected, tinfo = correct(eng, omega, Lb, R)
    _, t2 = eng.so_amplitudes()
    lev = np.diag(c["f"]).copy()
    tol = Q.tol_factor(sec, o, v)
    for k in range(4):
        val, S = Q.per_item_embedding(sec, c["g"], lev, o, t2, omega[k], *Lb[k], *R[k])
        print(sector, "root", k, "omega", omega[k], "delta", delta[k], "reference", float(np.sum(val)), "gap", tinfo["min_gap"][k])
        assert abs(delta[k] - float(np.sum(val))) <= tol * float(np.sum(S))
    assert np.array_equal(corrected, omega + delta)
    assert np.allclose(tinfo["min_gap"], np.abs(omega - Q.min_denominator(sec, lev, o)), rtol=0, atol=1e-12)
    assert tinfo["intruder"] == [k for k in range(4) if tinfo["min_gap"][k] < eom.INTRUDER_GAP]
    doublets = [cl for cl in eom.clusters(omega) if len(cl) == 2]
    assert doublets, (omega, info)                                         # a closed-shell reference: every root is a doublet
    for cl in doublets:
        assert abs(delta[cl[0]] - delta[cl[1]]) < 1e-10, (cl, delta)
    ni = eng.so_eom_ipea_t_nitems(sec)
    parts = correct(eng, omega, Lb, R, 0, ni // 2)[0] + correct(eng, omega, Lb, R, ni // 2, ni)[0]
    assert np.max(np.abs(parts - delta)) < 1e-12
    with pytest.raises(ValueError, match="biorthonormalise_ipea"):
        correct(eng, omega, Lv, [(2 * r[0], 2 * r[1]) for r in R])
