"""The EOM-IP-CCSD and EOM-EA-CCSD sigma builds (csrc/eom_ipea_so.hip) at extents where the planner leaves its smallest branch: sigma1 and
sigma2 of one random vector per sector at O(0.3) random amplitudes against the explicit restatements of np_eom_ipea alone (the ghost-
orbital complex step is infeasible here; tests/test_eom_ipea_cpu.py shows the two equal at small extents).  Shapes, systems, amplitudes
and the H-bar reference are those of tests/test_gpu_lambda_mid.py (MID, _ref): rhf_mid (10, 18), fock_odd (9, 13) with every f term,
rhf_cap (12, 46).

Tolerance: 1e-11 x max(1, max |ref|) per tensor; every comparison prints its error and its bound.

BRANCHES.  One row per product of a sigma build, per shape, as tests/test_gpu_eom_mid.py lists them: kernel extents M x N x K, tile code
tm,tn, K slices s, 16-byte staging w, and T where the product runs on the tall kernel once AFESP_TALL_MIN is o^2 v
(test_sigma_products_on_the_tall_kernel; the default threshold sends none of them there).  `pair-form ladder` is the EA sector's own
launch on the T iteration's packed pair buffers.  As printed on an MI355X (tools/eom_ipea_branches.py prints these tables).
  IP product        | rhf_mid (10, 18)             | fock_odd (9, 13)             | rhf_cap (12, 46)
  mi,m>i            | 1x10x10 1,1 s1 w1            | 1x9x9 1,1 s1 w0              | 1x12x12 1,1 s1 w1
  ime,me>i          | 1x10x180 1,1 s3 w1           | 1x9x117 1,1 s2 w0            | 1x12x552 1,1 s7 w1
  mnie,mne>i        | 1x10x1800 1,1 s23 w1         | 1x9x1053 1,1 s14 w0          | 1x12x6624 1,1 s83 w1
  mnef,mnf>e        | 1x18x1800 1,1 s23 w1         | 1x13x1053 1,1 s14 w0         | 1x46x6624 1,2 s83 w1
  mnij,mna>ija      | 18x100x100 1,4 s1 w1         | 13x81x81 1,4 s1 w0           | 46x144x144 2,4 s2 w1
  ije,ae>ija        | 18x100x18 1,4 s1 w1          | 13x81x13 1,4 s1 w0           | 46x144x46 2,4 s1 w1
  maij,m>ija        | 1x1800x10 1,4 s1 w1          | 1x1053x9 1,4 s1 w0           | 1x6624x12 1,4 s1 w1
  ijae,e>ija        | 1x1800x18 1,4 s1 w1 T        | 1x1053x13 1,4 s1 w0          | 1x6624x46 1,4 s1 w1 T
  ime,maej>ija      | 180x10x180 4,1 s3 w1         | 117x9x117 4,1 s2 w0          | 552x12x552 4,1 s7 w1
  ima,mj>ija        | 10x180x10 1,4 s1 w1          | 9x117x9 1,4 s1 w0            | 12x552x12 1,4 s1 w1
  EA product        | rhf_mid (10, 18)             | fock_odd (9, 13)             | rhf_cap (12, 46)
  ae,e>a            | 1x18x18 1,1 s1 w1            | 1x13x13 1,1 s1 w0            | 1x46x46 1,2 s1 w1
  mae,me>a          | 1x18x180 1,1 s3 w1           | 1x13x117 1,1 s2 w0           | 1x46x552 1,2 s7 w1
  amef,mef>a        | 1x18x3240 1,1 s41 w1         | 1x13x1521 1,1 s24 w0         | 1x46x25392 1,2 s318 w1
  mnef,nef>m        | 1x10x3240 1,1 s41 w1         | 1x9x1521 1,1 s24 w0          | 1x12x25392 1,1 s318 w1
  ief,amef>iam      | 180x10x324 4,1 s5 w1         | 117x9x169 4,1 s2 w0          | 552x12x2116 4,1 s27 w1
  ief,mnef>imn      | 100x10x324 4,1 s5 w1         | 81x9x169 4,1 s2 w0           | 144x12x2116 4,1 s27 w1
  pair-form ladder  | 153x10x154 4,1 s2 w1         | 78x10x78 4,1 s1 w1           | 1035x12x1036 4,1 s13 w1
  imn,mnab>iab      | 324x10x100 4,1 s1 w1         | 169x9x81 4,1 s1 w0           | 2116x12x144 4,1 s2 w1
  imab,m>iab        | 1x3240x10 1,4 s1 w1          | 1x1521x9 1,4 s1 w0           | 1x25392x12 1,4 s1 w1
  mi,mab>iab        | 324x10x10 4,1 s1 w1          | 169x9x9 4,1 s1 w0            | 2116x12x12 4,1 s1 w1
  ieab,e>iab        | 1x3240x18 1,4 s1 w1 T        | 1x1521x13 1,4 s1 w0          | 1x25392x46 1,4 s1 w1 T
  iam,mb>iab        | 18x180x10 1,4 s1 w1          | 13x117x9 1,4 s1 w0           | 46x552x12 2,4 s1 w1
  mae,mbei>iab      | 18x180x180 1,4 s3 w1         | 13x117x117 1,4 s2 w0         | 46x552x552 2,4 s7 w1
  iae,be>iab        | 18x180x18 1,4 s1 w1          | 13x117x13 1,4 s1 w0          | 46x552x46 2,4 s1 w1

ERRORS.  Largest error over its bound, per shape and sector: rhf_mid IP 8.9e-5 (sigma1: 1.8e-15 against 2.0e-11), EA 5.8e-5; fock_odd IP
4.9e-5, EA 4.0e-5; rhf_cap IP 7.2e-5, EA 8.1e-5 (sigma2: 1.6e-14 against 2.0e-10, the largest absolute error).  With AFESP_TALL_MIN at
o^2 v one product of each sector runs on the tall kernel at rhf_mid and rhf_cap (the rows marked T: K = v is at least 16 there, not at
fock_odd), and the tall kernel and the gather kernel agree to the bit on sigma1 and sigma2.  The pair-form ladder never qualifies: at
rhf_mid and fock_odd its 153 / 78 rows are fewer than 64 per column, at rhf_cap (and at every larger v) the K = v (v - 1) / 2 rows of
its skinny operand exceed the tall kernel's LDS image.  No product of either sigma build is re-laid-out at these shapes."""
import numpy as np
import pytest

import np_eom_ipea as X
from test_gpu_gett_matrix import _FIELDS, LAUNCH
from test_gpu_lambda import _close, _feed
from test_gpu_lambda_mid import EXTENTS, MID, _ref

pytestmark = pytest.mark.gpu

SECTORS = {"IP": X.IP, "EA": X.EA}
PRODUCTS = {X.IP: 10, X.EA: 13}      # products of the planner in one sigma build (EA: and the pair-form ladder's own launch)
_SIGMA = {}


def _sigma_ref(name, sec):
    """one random vector per shape and sector and its sigma by the explicit numpy form, made once and left unchanged"""
    if (name, sec) not in _SIGMA:
        r = _ref(name)
        cc = r["c"]["cc"]
        r1, r2 = X.random_vector(np.random.default_rng(9), sec, cc.o, cc.v)
        _SIGMA[name, sec] = (r1, r2, *X.sigma_explicit(sec, cc, *r["t"], r1, r2, r["I"]))
    return _SIGMA[name, sec]


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _sigma_pass(eng, name, sec, tag):
    """one sigma build on a live Lambda state at the shape's first amplitudes, checked against numpy -> (sigma1, sigma2)"""
    r1, r2, x1, x2 = _sigma_ref(name, sec)
    s1, s2 = eng.so_eom_ipea_sigma(sec, r1, r2)
    _close(s1, x1, 1e-11, f"{tag} sigma1")
    _close(s2, x2, 1e-11, f"{tag} sigma2")
    assert np.array_equal(s2, -(s2.transpose(1, 0, 2) if sec == X.IP else s2.transpose(0, 2, 1)))   # to the bit
    return s1, s2


@pytest.mark.parametrize("sector", sorted(SECTORS))
@pytest.mark.parametrize("name", sorted(MID))
def test_sigma_at_mid_size_and_the_branches_it_ran_on(eng, capfd, monkeypatch, name, sector):
    sec = SECTORS[sector]
    r = _ref(name)
    _feed(eng, r["c"])
    eng.so_set_amplitudes(*r["t"])
    eng.so_lambda_init(0)
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    capfd.readouterr()
    _sigma_pass(eng, name, sec, f"{sector} {name}")
    cap = capfd.readouterr()
    monkeypatch.delenv("AFESP_GETT_DEBUG")
    print(cap.out, end="")
    ls = [dict(zip(_FIELDS, map(int, m.groups()))) for m in LAUNCH.finditer(cap.err)]
    o, v = EXTENTS[name]
    npv, oa = v * (v - 1) // 2, o + o % 2
    for l in ls:
        print("launch", {k: l[k] for k in ("M", "N", "K", "akc", "bkc", "wide", "tm", "tn", "split")})
    assert len(ls) >= PRODUCTS[sec] + (sec == X.EA), cap.err
    ladder = [l for l in ls if l["M"] == npv and l["N"] == oa and l["K"] in (npv, npv + 1)]
    assert len(ladder) == (1 if sec == X.EA else 0), ladder                # M = K = v (v - 1) / 2, N = o: tall x skinny
    if sec == X.EA:
        assert ladder[0]["wide"] == 1 and ladder[0]["akc"] == 1
    rest = [l for l in ls if not ladder or l is not ladder[0]]
    if name == "fock_odd":
        assert all(l["wide"] == 0 for l in rest)                            # odd extents: 8-byte staging
    else:
        assert any(l["wide"] == 1 for l in rest)
        assert any(l["split"] > 1 for l in rest)                            # K slices


@pytest.mark.parametrize("name", ["rhf_mid", "rhf_cap"])
def test_sigma_products_on_the_tall_kernel(monkeypatch, name):
    """With AFESP_TALL_MIN at o^2 v (the threshold of tests/test_gpu_eom_mid.py) the product of y_e with t2 (IP) and of r_e with H_abei
    (EA) go to csrc/tall.hip: the counter rises in both sigma builds, the result matches numpy again, and the same run with AFESP_TALL=0
    (the gather kernel) to the bit.  The EA pair-form ladder stays with the gather kernel (the module's docstring says why)."""
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
            for sector, sec in sorted(SECTORS.items()):
                n0 = fresh.launch_counts()["tall"]
                out[tall, sec] = _sigma_pass(fresh, name, sec, f"{sector} {name} tall {tall}")
                n1 = fresh.launch_counts()["tall"]
                print(name, sector, "AFESP_TALL", tall, "tall launches in one sigma build", n1 - n0)
                assert n1 > n0 if tall == "1" else n1 == n0
    for sec in SECTORS.values():
        for a, b in zip(out["1", sec], out["0", sec]):
            assert np.array_equal(a, b)                                     # the tall kernel and the gather kernel: one K step order
