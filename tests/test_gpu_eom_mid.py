"""The EOM-EE-CCSD sigma build (csrc/eom_so.hip: so_eom_sigma) at extents where the planner leaves its smallest branch: sigma1 and sigma2
of one random vector at O(0.3) random amplitudes against the explicit restatement np_eom.sigma_explicit alone (the complex step is
infeasible here; tests/test_eom_cpu.py shows the two equal at small extents).  Shapes, systems, amplitudes and the H-bar reference are
those of tests/test_gpu_lambda_mid.py (MID, _ref): rhf_mid (10, 18), fock_odd (9, 13) with every f term, rhf_cap (12, 46).

Tolerance: 1e-11 x max(1, max |ref|) per tensor; every comparison prints its error and its bound.

BRANCHES.  One row per product of so_eom_sigma, per shape: kernel extents M x N x K, tile code tm,tn (1, 2, 4: 32, 64, 128 rows or
columns), K slices s, 16-byte staging w, and T where the product runs on the tall kernel once AFESP_TALL_MIN is o^2 v
(test_sigma_products_on_the_tall_kernel; the default threshold sends none of them there).  `pair-form ladder` is so_ladder_bare's own
launch on its packed pair buffers.  As printed on an MI355X (tools/eom_branches.py prints this table).
  product           | rhf_mid (10, 18)             | fock_odd (9, 13)             | rhf_cap (12, 46)
  ae,ie>ia          | 18x10x18 1,1 s1 w1           | 13x9x13 1,1 s1 w0            | 46x12x46 2,1 s1 w1
  mi,ma>ia          | 18x10x10 1,1 s1 w1           | 13x9x9 1,1 s1 w0             | 46x12x12 2,1 s1 w1
  imae,me>ia        | 1x180x180 1,4 s3 w1          | 1x117x117 1,4 s2 w0          | 1x552x552 1,4 s7 w1
  maei,me>ia        | 1x180x180 1,4 s3 w1          | 1x117x117 1,4 s2 w0          | 1x552x552 1,4 s7 w1
  mnae,mnie>ia      | 18x10x1800 1,1 s23 w1        | 13x9x1053 1,1 s14 w0         | 46x12x6624 2,1 s83 w1
  imef,amef>ia      | 18x10x3240 1,1 s41 w1        | 13x9x1521 1,1 s24 w0         | 46x12x25392 2,1 s318 w1
  bmef,mf>be        | 1x324x180 1,4 s3 w1          | 1x169x117 1,4 s2 w0          | 1x2116x552 1,4 s7 w1
  mnef,mnbf>be      | 18x18x1800 1,1 s23 w1        | 13x13x1053 1,1 s14 w0        | 46x46x6624 2,2 s83 w1
  mnje,ne>mj        | 1x100x180 1,4 s3 w1          | 1x81x117 1,4 s2 w0           | 1x144x552 1,4 s7 w1
  mnef,jnef>mj      | 10x10x3240 1,1 s41 w1        | 9x9x1521 1,1 s24 w0          | 12x12x25392 1,1 s318 w1
  pair-form ladder  | 153x46x154 4,2 s2 w1         | 78x36x78 4,2 s1 w1           | 1035x66x1036 4,4 s13 w1
  ijef,amef>ijam    | 180x100x324 4,4 s5 w1        | 117x81x169 4,4 s2 w0         | 552x144x2116 4,4 s27 w1
  ijam,mb>ijab      | 18x1800x10 1,4 s1 w1         | 13x1053x9 1,4 s1 w0          | 46x6624x12 2,4 s1 w1
  ijbm,ma>ijab      | 18x1800x10 1,4 s1 w1         | 13x1053x9 1,4 s1 w0          | 46x6624x12 2,4 s1 w1
  ijef,mnef>ijmn    | 100x100x324 4,4 s5 w1        | 81x81x169 4,4 s2 w0          | 144x144x2116 4,4 s27 w1
  ijmn,mnab>ijab    | 324x100x100 4,4 s1 w1        | 169x81x81 4,4 s1 w0          | 2116x144x144 4,2 s2 w1
  mnij,mnab>ijab    | 324x100x100 4,4 s1 w1        | 169x81x81 4,4 s1 w0          | 2116x144x144 4,2 s2 w1
  imae,mbej>ijab    | 180x180x180 4,4 s3 w1        | 117x117x117 4,4 s2 w0        | 552x552x552 4,4 s7 w1
  mj,imab>ijab      | 10x3240x10 1,4 s1 w1         | 9x1521x9 1,4 s1 w0           | 12x25392x12 1,4 s1 w1
  ie,jeab>ijab      | 3240x10x18 4,1 s1 w1 T       | 1521x9x13 4,1 s1 w0          | 25392x12x46 4,1 s1 w1 T
  mj,imab>ijab      | 10x3240x10 1,4 s1 w1         | 9x1521x9 1,4 s1 w0           | 12x25392x12 1,4 s1 w1
  ijae,be>ijab      | 18x1800x18 1,4 s1 w1 T       | 13x1053x13 1,4 s1 w0         | 46x6624x46 2,4 s1 w1
  mbij,ma>ijab      | 18x1800x10 1,4 s1 w1         | 13x1053x9 1,4 s1 w0          | 46x6624x12 2,4 s1 w1
  ijae,be>ijab      | 18x1800x18 1,4 s1 w1 T       | 13x1053x13 1,4 s1 w0         | 46x6624x46 2,4 s1 w1

ERRORS.  Largest error over its bound, per shape: rhf_mid 1.2e-4 (sigma1: 5.8e-15 against 5.0e-11), fock_odd 6.5e-5 (sigma1: 3.1e-15
against 4.8e-11), rhf_cap 1.2e-4 (sigma1: 2.3e-14 against 1.9e-10); the largest absolute error is 2.6e-14, in sigma2 at rhf_cap.  With
AFESP_TALL_MIN at o^2 v three products of rhf_mid and one of rhf_cap run on the tall kernel (the rows marked T), and the tall kernel and the
gather kernel agree to the bit on sigma1 and sigma2.  No product of the sigma build is re-laid-out at these shapes."""
import numpy as np
import pytest

import np_eom
import np_lambda
from test_gpu_gett_matrix import _FIELDS, LAUNCH
from test_gpu_lambda import _close, _feed
from test_gpu_lambda_mid import EXTENTS, MID, _ref

pytestmark = pytest.mark.gpu

_SIGMA = {}


def _sigma_ref(name):
    """one random vector per shape and its sigma by the explicit numpy form, made once and left unchanged"""
    if name not in _SIGMA:
        r = _ref(name)
        cc = r["c"]["cc"]
        r1, r2 = np_lambda.antisym_random(np.random.default_rng(9), cc.o, cc.v)
        _SIGMA[name] = (r1, r2, *np_eom.sigma_explicit(cc, *r["t"], r1, r2, r["I"]))
    return _SIGMA[name]


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _sigma_pass(eng, name, tag):
    """one sigma build on a live Lambda state at the shape's first amplitudes, checked against numpy -> (sigma1, sigma2)"""
    r1, r2, x1, x2 = _sigma_ref(name)
    s1, s2 = eng.so_eom_sigma(r1, r2)
    _close(s1, x1, 1e-11, f"{tag} sigma1")
    _close(s2, x2, 1e-11, f"{tag} sigma2")
    assert np.array_equal(s2, -s2.transpose(1, 0, 2, 3)) and np.array_equal(s2, -s2.transpose(0, 1, 3, 2))   # to the bit
    return s1, s2


@pytest.mark.parametrize("name", sorted(MID))
def test_sigma_at_mid_size_and_the_branches_it_ran_on(eng, capfd, monkeypatch, name):
    r = _ref(name)
    _feed(eng, r["c"])
    eng.so_set_amplitudes(*r["t"])
    eng.so_lambda_init(0)
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    capfd.readouterr()
    _sigma_pass(eng, name, name)
    cap = capfd.readouterr()
    monkeypatch.delenv("AFESP_GETT_DEBUG")
    print(cap.out, end="")
    ls = [dict(zip(_FIELDS, map(int, m.groups()))) for m in LAUNCH.finditer(cap.err)]
    o, v = EXTENTS[name]
    npo, npv = o * (o - 1) // 2, v * (v - 1) // 2
    for l in ls:
        print("launch", {k: l[k] for k in ("M", "N", "K", "akc", "bkc", "wide", "tm", "tn", "split")})
    assert len(ls) >= 24, cap.err                                           # the 23 products of the planner and so_ladder_bare's own launch
    ladder = [l for l in ls if l["M"] == npv and l["N"] in (npo, npo + 1) and l["K"] in (npv, npv + 1)]
    assert len(ladder) == 1, ladder
    rest = [l for l in ls if l is not ladder[0]]
    if name == "fock_odd":
        assert all(l["wide"] == 0 for l in rest)                            # odd extents: 8-byte staging
    else:
        assert any(l["wide"] == 1 for l in rest)
        assert any(l["tm"] == 4 or l["tn"] == 4 for l in rest)              # 128-row tiles
        assert any(l["split"] > 1 for l in rest)                            # K slices
    if name == "rhf_cap":
        assert any(l["tm"] == 2 or l["tn"] == 2 for l in rest)              # 64-row tiles


@pytest.mark.parametrize("name", ["rhf_mid", "rhf_cap"])
def test_sigma_products_on_the_tall_kernel(monkeypatch, name):
    """With AFESP_TALL_MIN at o^2 v the products of a two-index operand with a four-index array go to csrc/tall.hip: the counter rises
    in so_eom_sigma, the result matches numpy again, and the same run with AFESP_TALL=0."""
    from afesp_amd.capi import Engine
    r = _ref(name)
    o, v = EXTENTS[name]
    r1, r2, _, x2 = _sigma_ref(name)
    out = {}
    for tall in ("1", "0"):
        monkeypatch.setenv("AFESP_TALL_MIN", str(o * o * v))
        monkeypatch.setenv("AFESP_TALL", tall)
        with Engine(0) as fresh:
            _feed(fresh, r["c"])
            fresh.so_set_amplitudes(*r["t"])
            fresh.so_lambda_init(0)
            n0 = fresh.launch_counts()["tall"]
            out[tall] = _sigma_pass(fresh, name, f"{name} tall {tall}")
            n1 = fresh.launch_counts()["tall"]
            print(name, "AFESP_TALL", tall, "tall launches in one sigma build", n1 - n0)
            assert n1 > n0 if tall == "1" else n1 == n0
    for a, b in zip(out["1"], out["0"]):
        assert np.array_equal(a, b)                                         # the tall kernel and the gather kernel: one K step order
