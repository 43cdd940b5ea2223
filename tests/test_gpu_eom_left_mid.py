"""The left sigma build and the bilinear density (csrc/eom_left_so.hip: so_eom_lsigma, so_eom_density) at extents where the planner leaves
its smallest branch: one random vector (pair) at O(0.3) random amplitudes against the explicit restatements np_eom_left.lsigma_explicit
and density_explicit alone (the Jacobian and the central difference in f are infeasible here; tests/test_eom_left_cpu.py shows the forms
equal at small extents).  Shapes, systems, amplitudes and the H-bar reference are those of tests/test_gpu_lambda_mid.py (MID, _ref):
rhf_mid (10, 18), fock_odd (9, 13) with every f term, rhf_cap (12, 46).

Tolerance: 1e-11 x max(1, max |ref|) per tensor; every comparison prints its error and its bound.

BRANCHES.  One row per product, per shape: kernel extents M x N x K, tile code tm,tn (1, 2, 4: 32, 64, 128 rows or columns), K slices s,
16-byte staging w, and T where the product runs on the tall kernel once AFESP_TALL_MIN is o^2 v (test_left_sigma_products_on_the_tall_kernel;
the default threshold sends none of them there).  `pair-form ladder` is so_ladder_bare's own launch on its packed pair buffers.  As printed
on an MI355X (tools/eom_branches.py --left and --density print these tables).
 so_eom_lsigma:
  product           | rhf_mid (10, 18)             | fock_odd (9, 13)             | rhf_cap (12, 46)
  mnef,mnaf>ae      | 18x18x1800 1,1 s23 w1        | 13x13x1053 1,1 s14 w0        | 46x46x6624 2,2 s83 w1
  mnef,inef>mi      | 10x10x3240 1,1 s41 w1        | 9x9x1521 1,1 s24 w0          | 12x12x25392 1,1 s318 w1
  ie,ea>ia          | 18x10x18 1,1 s1 w1           | 13x9x13 1,1 s1 w0            | 46x12x46 2,1 s1 w1
  im,ma>ia          | 18x10x10 1,1 s1 w1           | 13x9x9 1,1 s1 w0             | 46x12x12 2,1 s1 w1
  me,ieam>ia        | 1x180x180 1,4 s3 w1          | 1x117x117 1,4 s2 w0          | 1x552x552 1,4 s7 w1
  imef,maef>ia      | 18x10x3240 1,1 s41 w1        | 13x9x1521 1,1 s24 w0         | 46x12x25392 2,1 s318 w1
  mnae,iemn>ia      | 18x10x1800 1,1 s23 w1        | 13x9x1053 1,1 s14 w0         | 46x12x6624 2,1 s83 w1
  ef,eifa>ia        | 1x180x324 1,4 s5 w1          | 1x117x169 1,4 s2 w0          | 1x552x2116 1,4 s27 w1
  mn,mina>ia        | 1x180x100 1,4 s1 w1          | 1x117x81 1,4 s1 w0           | 1x552x144 1,4 s2 w1
  pair-form ladder  | 153x46x154 4,2 s2 w1         | 78x36x78 4,2 s1 w1           | 1035x66x1036 4,4 s13 w1
  ijef,mf>ijme      | 10x1800x18 1,4 s1 w1 T       | 9x1053x13 1,4 s1 w0          | 12x6624x46 1,4 s1 w1 T
  ijme,emab>ijab    | 324x100x180 4,4 s3 w1        | 169x81x117 4,4 s2 w0         | 2116x144x552 4,2 s7 w1
  ijef,mnef>ijmn    | 100x100x324 4,4 s5 w1        | 81x81x169 4,4 s2 w0          | 144x144x2116 4,4 s27 w1
  ijmn,mnab>ijab    | 324x100x100 4,4 s1 w1        | 169x81x81 4,4 s1 w0          | 2116x144x144 4,2 s2 w1
  ijmn,mnab>ijab    | 324x100x100 4,4 s1 w1        | 169x81x81 4,4 s1 w0          | 2116x144x144 4,2 s2 w1
  imae,jebm>ijab    | 180x180x180 4,4 s3 w1        | 117x117x117 4,4 s2 w0        | 552x552x552 4,4 s7 w1
  jm,imab>ijab      | 10x3240x10 1,4 s1 w1         | 9x1521x9 1,4 s1 w0           | 12x25392x12 1,4 s1 w1
  ie,ejab>ijab      | 3240x10x18 4,1 s1 w1 T       | 1521x9x13 4,1 s1 w0          | 25392x12x46 4,1 s1 w1 T
  imab,mj>ijab      | 10x3240x10 1,4 s1 w1         | 9x1521x9 1,4 s1 w0           | 12x25392x12 1,4 s1 w1
  ijae,eb>ijab      | 18x1800x18 1,4 s1 w1 T       | 13x1053x13 1,4 s1 w0         | 46x6624x46 2,4 s1 w1
  ijmb,ma>ijab      | 18x1800x10 1,4 s1 w1         | 13x1053x9 1,4 s1 w0          | 46x6624x12 2,4 s1 w1
  ijae,be>ijab      | 18x1800x18 1,4 s1 w1 T       | 13x1053x13 1,4 s1 w0         | 46x6624x46 2,4 s1 w1
 so_eom_density, both vectors given (without a right vector: the two G, the four products of the lambda part and the last row; without
 a left vector: none):
  product           | rhf_mid (10, 18)             | fock_odd (9, 13)             | rhf_cap (12, 46)
  mnef,mnaf>ae      | 18x18x1800 1,1 s23 w1        | 13x13x1053 1,1 s14 w0        | 46x46x6624 2,2 s83 w1
  mnef,inef>mi      | 10x10x3240 1,1 s41 w1        | 9x9x1521 1,1 s24 w0          | 12x12x25392 1,1 s318 w1
  ijab,ia>jb        | 1x180x180 1,4 s3 w1          | 1x117x117 1,4 s2 w0          | 1x552x552 1,4 s7 w1
  ma,ia>mi          | 10x10x18 1,1 s1 w1           | 9x9x13 1,1 s1 w0             | 12x12x46 1,1 s1 w1
  ia,ie>ae          | 18x18x10 1,1 s1 w1           | 13x13x9 1,1 s1 w0            | 46x46x12 2,2 s1 w1
  ia,imae>me        | 1x180x180 1,4 s3 w1          | 1x117x117 1,4 s2 w0          | 1x552x552 1,4 s7 w1
  mj,je>me          | 18x10x10 1,1 s1 w1           | 13x9x9 1,1 s1 w0             | 46x12x12 2,1 s1 w1
  mnef,mnaf>ae      | 18x18x1800 1,1 s23 w1        | 13x13x1053 1,1 s14 w0        | 46x46x6624 2,2 s83 w1
  mnef,inef>mi      | 10x10x3240 1,1 s41 w1        | 9x9x1521 1,1 s24 w0          | 12x12x25392 1,1 s318 w1
  ma,ia>mi          | 10x10x18 1,1 s1 w1           | 9x9x13 1,1 s1 w0             | 12x12x46 1,1 s1 w1
  ia,ie>ae          | 18x18x10 1,1 s1 w1           | 13x13x9 1,1 s1 w0            | 46x46x12 2,2 s1 w1
  ia,ie>ae          | 18x18x10 1,1 s1 w1           | 13x13x9 1,1 s1 w0            | 46x46x12 2,2 s1 w1
  ia,imae>me        | 1x180x180 1,4 s3 w1          | 1x117x117 1,4 s2 w0          | 1x552x552 1,4 s7 w1
  mb,be>me          | 18x10x18 1,1 s1 w1           | 13x9x13 1,1 s1 w0            | 46x12x46 2,1 s1 w1
  mj,je>me          | 18x10x10 1,1 s1 w1           | 13x9x9 1,1 s1 w0             | 46x12x12 2,1 s1 w1
  mj,je>me          | 18x10x10 1,1 s1 w1           | 13x9x9 1,1 s1 w0             | 46x12x12 2,1 s1 w1
  mb,be>me          | 18x10x18 1,1 s1 w1           | 13x9x13 1,1 s1 w0            | 46x12x46 2,1 s1 w1
(the ladder is the one o^2 v^4 product, and the density has no product above o^2 v^2 in cost at all)

ERRORS.  Largest error over its bound: left sigma 2.5e-4 at rhf_mid (sigma1: 3.6e-14 against 1.4e-10) and 1.3e-4 at rhf_cap (sigma1:
1.3e-13 against 9.9e-10; sigma2: 2.9e-14 against 3.7e-10); the density 3.5e-4 at rhf_mid (6.7e-15 against 1.9e-11), 1.4e-4 at fock_odd,
1.0e-4 at rhf_cap (7.4e-15 against 7.2e-11).  With AFESP_TALL_MIN at o^2 v four products of rhf_mid and two of rhf_cap run on the tall
kernel (the rows marked T), and the tall kernel and the gather kernel agree to the bit on sigma1 and sigma2.  No product is re-laid-out at
these shapes."""
import numpy as np
import pytest

import np_eom_left
import np_lambda
from test_gpu_gett_matrix import _FIELDS, LAUNCH
from test_gpu_lambda import _close, _feed
from test_gpu_lambda_mid import EXTENTS, MID, _ref

pytestmark = pytest.mark.gpu

_LEFT = {}


def _left_ref(name):
    """one random left and one random right vector per shape, sigma_L of the first and the density of the pair (0.7, l; -0.4, r) by the
    explicit numpy forms, made once and left unchanged"""
    if name not in _LEFT:
        r = _ref(name)
        cc = r["c"]["cc"]
        rng = np.random.default_rng(13)
        l, x = np_lambda.antisym_random(rng, cc.o, cc.v), np_lambda.antisym_random(rng, cc.o, cc.v)
        _LEFT[name] = dict(l=l, r=x, sigma=np_eom_left.lsigma_explicit(cc, *r["t"], *l, r["I"]),
                           density=np_eom_left.density_explicit(cc, *r["t"], 0.7, l, -0.4, x),
                           density_left_only=np_eom_left.density_explicit(cc, *r["t"], 0.7, l, -0.4, None))
    return _LEFT[name]


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _lsigma_pass(eng, name, tag):
    """one left sigma build on a live Lambda state at the shape's first amplitudes, checked against numpy -> (sigma1, sigma2)"""
    ref = _left_ref(name)
    s1, s2 = eng.so_eom_lsigma(*ref["l"])
    _close(s1, ref["sigma"][0], 1e-11, f"{tag} left sigma1")
    _close(s2, ref["sigma"][1], 1e-11, f"{tag} left sigma2")
    assert np.array_equal(s2, -s2.transpose(1, 0, 2, 3)) and np.array_equal(s2, -s2.transpose(0, 1, 3, 2))   # to the bit
    return s1, s2


def _launches(capfd, monkeypatch, call):
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    capfd.readouterr()
    call()
    cap = capfd.readouterr()
    monkeypatch.delenv("AFESP_GETT_DEBUG")
    print(cap.out, end="")
    ls = [dict(zip(_FIELDS, map(int, m.groups()))) for m in LAUNCH.finditer(cap.err)]
    for l in ls:
        print("launch", {k: l[k] for k in ("M", "N", "K", "akc", "bkc", "wide", "tm", "tn", "split")})
    return ls, cap.err


def _check_branches(name, rest):
    if name == "fock_odd":
        assert all(l["wide"] == 0 for l in rest)                            # odd extents: 8-byte staging
    else:
        assert any(l["wide"] == 1 for l in rest)
        assert any(l["tm"] == 4 or l["tn"] == 4 for l in rest)              # 128-row tiles
        assert any(l["split"] > 1 for l in rest)                            # K slices
    if name == "rhf_cap":
        assert any(l["tm"] == 2 or l["tn"] == 2 for l in rest)              # 64-row tiles


@pytest.mark.parametrize("name", sorted(MID))
def test_left_sigma_and_density_at_mid_size_and_the_branches_they_ran_on(eng, capfd, monkeypatch, name):
    r = _ref(name)
    ref = _left_ref(name)
    _feed(eng, r["c"])
    eng.so_set_amplitudes(*r["t"])
    eng.so_lambda_init(0)
    ls, err = _launches(capfd, monkeypatch, lambda: _lsigma_pass(eng, name, name))
    o, v = EXTENTS[name]
    npo, npv = o * (o - 1) // 2, v * (v - 1) // 2
    assert len(ls) >= 22, err                                               # the 21 products of the planner and so_ladder_bare's own launch
    ladder = [l for l in ls if l["M"] == npv and l["N"] in (npo, npo + 1) and l["K"] in (npv, npv + 1)]
    assert len(ladder) == 1, ladder
    _check_branches(name, [l for l in ls if l is not ladder[0]])
    out = {}
    ls, err = _launches(capfd, monkeypatch, lambda: out.update(d=eng.so_eom_density(0.7, ref["l"], -0.4, ref["r"])))
    assert len(ls) >= 17, err
    _check_branches(name, ls)
    _close(out["d"], ref["density"], 1e-11, f"{name} density")
    assert np.array_equal(out["d"], out["d"].T) and abs(np.trace(out["d"])) < 1e-12
    _close(eng.so_eom_density(0.7, ref["l"], -0.4, None), ref["density_left_only"], 1e-11, f"{name} density without a right vector")


@pytest.mark.parametrize("name", ["rhf_mid", "rhf_cap"])
def test_left_sigma_products_on_the_tall_kernel(monkeypatch, name):
    """With AFESP_TALL_MIN at o^2 v the products of a two-index operand with a four-index array go to csrc/tall.hip: the counter rises
    in so_eom_lsigma, the result matches numpy again, and the same run with AFESP_TALL=0."""
    from afesp_amd.capi import Engine
    r = _ref(name)
    o, v = EXTENTS[name]
    out = {}
    for tall in ("1", "0"):
        monkeypatch.setenv("AFESP_TALL_MIN", str(o * o * v))
        monkeypatch.setenv("AFESP_TALL", tall)
        with Engine(0) as fresh:
            _feed(fresh, r["c"])
            fresh.so_set_amplitudes(*r["t"])
            fresh.so_lambda_init(0)
            n0 = fresh.launch_counts()["tall"]
            out[tall] = _lsigma_pass(fresh, name, f"{name} tall {tall}")
            n1 = fresh.launch_counts()["tall"]
            print(name, "AFESP_TALL", tall, "tall launches in one left sigma build", n1 - n0)
            assert n1 > n0 if tall == "1" else n1 == n0
    for a, b in zip(out["1"], out["0"]):
        assert np.array_equal(a, b)                                         # the tall kernel and the gather kernel: one K step order
