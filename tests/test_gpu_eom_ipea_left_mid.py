"""The left sigma builds and the Dyson vectors of EOM-IP-CCSD and EOM-EA-CCSD (csrc/eom_ipea_left_so.hip) at extents where the planner
leaves its smallest branch: sigma_L1, sigma_L2 and both Dyson vectors of one random vector pair per sector at O(0.3) random amplitudes and
lambda against the explicit restatements of np_eom_ipea_left alone (the ghost-orbital definitions are infeasible here;
tests/test_eom_ipea_left_cpu.py shows the two equal at small extents).  Shapes, systems, amplitudes, lambda and the H-bar reference are
those of tests/test_gpu_lambda_mid.py (MID, _ref): rhf_mid (10, 18), fock_odd (9, 13) with every f term, rhf_cap (12, 46) -- where the
mid tests of the right-hand builds reach the 64- and 128-row tiles, K slices of 318 and both staging widths.

Tolerance: 1e-11 x max(1, max |ref|) per tensor; every comparison prints its error and its bound.

BRANCHES.  One row per product of a left sigma build, per shape, in the form of the table in tests/test_gpu_eom_ipea_mid.py: kernel extents
M x N x K, tile code tm,tn, K slices s, 16-byte staging w, and T where the product runs on the tall kernel once AFESP_TALL_MIN is o^2 v
(test_left_sigma_products_on_the_tall_kernel; the default threshold sends none of them there).  `pair-form ladder` is the EA sector's own
launch on the T iteration's packed pair buffers, the right-hand build's with l2 in place of r2.  As printed on an MI355X
(tools/eom_ipea_branches.py --left prints these tables).
  IP product        | rhf_mid (10, 18)             | fock_odd (9, 13)             | rhf_cap (12, 46)
  mi,i>m            | 1x10x10 1,1 s1 w1            | 1x9x9 1,1 s1 w0              | 1x12x12 1,1 s1 w1
  maij,ija>m        | 1x10x1800 1,1 s23 w1         | 1x9x1053 1,1 s14 w0          | 1x12x6624 1,1 s83 w1
  ijae,ija>e        | 1x18x1800 1,1 s23 w1         | 1x13x1053 1,1 s14 w0         | 1x46x6624 1,2 s83 w1
  mnij,ije>mne      | 18x100x100 1,4 s1 w1         | 13x81x81 1,4 s1 w0           | 46x144x144 2,4 s2 w1
  mna,ae>mne        | 18x100x18 1,4 s1 w1          | 13x81x13 1,4 s1 w0           | 46x144x46 2,4 s1 w1
  mnie,i>mne        | 1x1800x10 1,4 s1 w1          | 1x1053x9 1,4 s1 w0           | 1x6624x12 1,4 s1 w1
  mnae,a>mne        | 1x1800x18 1,4 s1 w1 T        | 1x1053x13 1,4 s1 w0          | 1x6624x46 1,4 s1 w1 T
  mja,naej>mne      | 180x10x180 4,1 s3 w1         | 117x9x117 4,1 s2 w0          | 552x12x552 4,1 s7 w1
  mje,nj>mne        | 10x180x10 1,4 s1 w1          | 9x117x9 1,4 s1 w0            | 12x552x12 1,4 s1 w1
  EA product        | rhf_mid (10, 18)             | fock_odd (9, 13)             | rhf_cap (12, 46)
  ae,a>e            | 1x18x18 1,1 s1 w1            | 1x13x13 1,1 s1 w0            | 1x46x46 1,2 s1 w1
  ieab,iab>e        | 1x18x3240 1,1 s41 w1         | 1x13x1521 1,1 s24 w0         | 1x46x25392 1,2 s318 w1
  imab,iab>m        | 1x10x3240 1,1 s41 w1         | 1x9x1521 1,1 s24 w0          | 1x12x25392 1,1 s318 w1
  iab,mb>iam        | 10x180x18 1,4 s1 w1          | 9x117x13 1,4 s1 w0           | 12x552x46 1,4 s1 w1
  iab,mnab>imn      | 100x10x324 4,1 s5 w1         | 81x9x169 4,1 s2 w0           | 144x12x2116 4,1 s27 w1
  pair-form ladder  | 153x10x154 4,1 s2 w1         | 78x10x78 4,1 s1 w1           | 1035x12x1036 4,1 s13 w1
  imn,mnef>ief      | 324x10x100 4,1 s1 w1         | 169x9x81 4,1 s1 w0           | 2116x12x144 4,1 s2 w1
  mief,m>ief        | 1x3240x10 1,4 s1 w1          | 1x1521x9 1,4 s1 w0           | 1x25392x12 1,4 s1 w1
  im,mef>ief        | 324x10x10 4,1 s1 w1          | 169x9x9 4,1 s1 w0            | 2116x12x12 4,1 s1 w1
  aief,a>ief        | 1x3240x18 1,4 s1 w1 T        | 1x1521x13 1,4 s1 w0          | 1x25392x46 1,4 s1 w1 T
  iam,amef>ief      | 324x10x180 4,1 s3 w1         | 169x9x117 4,1 s2 w0          | 2116x12x552 4,1 s7 w1
  mab,ibem>iae      | 18x180x180 1,4 s3 w1         | 13x117x117 1,4 s2 w0         | 46x552x552 2,4 s7 w1
  iab,be>iae        | 18x180x18 1,4 s1 w1          | 13x117x13 1,4 s1 w0          | 46x552x46 2,4 s1 w1

The products are the transposes of the right-hand table's, with its extents: no product of either left build is re-laid-out at these
shapes, and the pair-form ladder stays with the gather kernel for the reasons given there."""
import numpy as np
import pytest

import np_eom_ipea as X
import np_eom_ipea_left as XL
from test_gpu_gett_matrix import _FIELDS, LAUNCH
from test_gpu_lambda import _close, _feed
from test_gpu_lambda_mid import EXTENTS, MID, _ref

pytestmark = pytest.mark.gpu

SECTORS = {"IP": X.IP, "EA": X.EA}
PRODUCTS = {X.IP: 9, X.EA: 12}       # products of the planner in one left sigma build (EA: and the pair-form ladder's own launch)
_LEFT = {}


def _left_ref(name, sec):
    """one random vector pair per shape and sector with sigma_L and the Dyson vectors by the explicit numpy forms, made once"""
    if (name, sec) not in _LEFT:
        r = _ref(name)
        cc = r["c"]["cc"]
        rng = np.random.default_rng(19)
        l, x = X.random_vector(rng, sec, cc.o, cc.v), X.random_vector(rng, sec, cc.o, cc.v)
        _LEFT[name, sec] = (l, x, XL.lsigma_explicit(sec, cc, *r["t"], *l, r["I"]), XL.dyson_explicit(sec, cc, *r["t"], *r["l"], l, x))
    return _LEFT[name, sec]


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _lsigma_pass(eng, name, sec, tag):
    l, _, (x1, x2), _ = _left_ref(name, sec)
    s1, s2 = eng.so_eom_ipea_lsigma(sec, *l)
    _close(s1, x1, 1e-11, f"{tag} left sigma1")
    _close(s2, x2, 1e-11, f"{tag} left sigma2")
    assert np.array_equal(s2, -(s2.transpose(1, 0, 2) if sec == X.IP else s2.transpose(0, 2, 1)))   # to the bit
    return s1, s2


@pytest.mark.parametrize("sector", sorted(SECTORS))
@pytest.mark.parametrize("name", sorted(MID))
def test_left_sigma_at_mid_size_and_the_branches_it_ran_on(eng, capfd, monkeypatch, name, sector):
    sec = SECTORS[sector]
    r = _ref(name)
    _feed(eng, r["c"])
    eng.so_set_amplitudes(*r["t"])
    eng.so_lambda_init(0)
    eng.so_set_lambda(*r["l"])
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    capfd.readouterr()
    _lsigma_pass(eng, name, sec, f"{sector} {name}")
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
    assert len(ladder) == (1 if sec == X.EA else 0), ladder                # the right-hand build's ladder launch, on l2
    rest = [l for l in ls if not ladder or l is not ladder[0]]
    if name == "fock_odd":
        assert all(l["wide"] == 0 for l in rest)                            # odd extents: 8-byte staging
    else:
        assert any(l["wide"] == 1 for l in rest)
        assert any(l["split"] > 1 for l in rest)                            # K slices
    l, x, _, (gl, gr) = _left_ref(name, sec)
    dl, dr = eng.so_eom_ipea_dyson(sec, l, x)
    _close(dl, gl, 1e-11, f"{sector} {name} left Dyson vector")
    _close(dr, gr, 1e-11, f"{sector} {name} right Dyson vector")
    again = eng.so_eom_ipea_dyson(sec, l, x)
    assert np.array_equal(again[0], dl) and np.array_equal(again[1], dr)


@pytest.mark.parametrize("name", ["rhf_mid", "rhf_cap"])
def test_left_sigma_products_on_the_tall_kernel(monkeypatch, name):
    """With AFESP_TALL_MIN at o^2 v (the threshold of tests/test_gpu_eom_ipea_mid.py) one product of each sector's left build goes to
    csrc/tall.hip -- G_a <mn||ae> (IP) and H_aief l_a (EA), the products with K = v: the counter rises in both builds, the result matches
    numpy again, and the same run with AFESP_TALL=0 (the gather kernel) to the bit."""
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
                out[tall, sec] = _lsigma_pass(fresh, name, sec, f"{sector} {name} tall {tall}")
                n1 = fresh.launch_counts()["tall"]
                print(name, sector, "AFESP_TALL", tall, "tall launches in one left sigma build", n1 - n0)
                assert n1 > n0 if tall == "1" else n1 == n0
    for sec in SECTORS.values():
        for a, b in zip(out["1", sec], out["0", sec]):
            assert np.array_equal(a, b)                                     # the tall kernel and the gather kernel: one K step order
