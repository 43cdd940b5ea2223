"""The two-particle density at mid-size extents, block by block against the explicit numpy form alone (np_density2.gamma_explicit, itself
held to the defining finite difference on the CPU at 3,3 / 2,4 / 5,7): the shapes of test_gpu_lambda_mid.py -- 10,18 (RHF-fed), 9,13 (odd
extents, every f term) and 12,46 (the pair product at M = N = 1035, K = 66) -- with its random O(0.3) amplitudes.

Rule: 1e-11 x max(1, max |ref|) per block.  Largest error of a block measured on the MI355X: 1.4e-15 at 9,13, 3.1e-15 at 10,18 (oovv),
8.9e-15 at 12,46.  The launcher's own line (AFESP_GETT_DEBUG) shows the vvvv term as ONE product over the packed pairs:
M = N = v (v - 1) / 2, K = o (o - 1) / 2 -- 1035 x 1035 x 66 at 12,46, tm = tn = 4 (128 x 128 tiles), no K split."""
import numpy as np
import pytest

import np_density2
import np_lambda
from test_gpu_gett_matrix import _FIELDS, LAUNCH
from test_gpu_lambda import _close, _feed
from test_gpu_lambda_mid import EXTENTS, MID, _ref

pytestmark = pytest.mark.gpu

NAMES = ("oooo", "ooov", "oovv", "ovov", "ovvv")
_GAMMA = {}


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _gamma(name):
    """the explicit form at the shape's first amplitudes, made once"""
    if name not in _GAMMA:
        r = _ref(name)
        _GAMMA[name] = np_density2.gamma_explicit(*r["t"], *r["l"])
    return _GAMMA[name]


@pytest.mark.parametrize("name", sorted(MID))
def test_blocks_at_mid_size(eng, capfd, monkeypatch, name):
    r, G = _ref(name), _gamma(name)
    c = r["c"]
    o, v = EXTENTS[name]
    npo, npv = o * (o - 1) // 2, v * (v - 1) // 2
    _feed(eng, c)
    eng.so_set_amplitudes(*r["t"])
    eng.so_lambda_init(0)
    eng.so_set_lambda(*r["l"])
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    capfd.readouterr()
    eng.so_density2_build()
    cap = capfd.readouterr()
    monkeypatch.delenv("AFESP_GETT_DEBUG")
    ls = [dict(zip(_FIELDS, map(int, m.groups()))) for m in LAUNCH.finditer(cap.err)]
    pair = [l for l in ls if l["M"] == npv and l["N"] == npv and l["K"] == npo]
    print(name, "launches of the build", len(ls), "pair product", [{k: l[k] for k in ("M", "N", "K", "tm", "tn", "split")} for l in pair])
    assert len(pair) == 1, cap.err                                        # ONE product over the packed pairs, K = o (o - 1) / 2
    worst = 0.0
    for k in NAMES:
        got = eng.so_density2_get(k)
        _close(got, G[k], 1e-11, f"{name} {k}")
        worst = max(worst, float(np.max(np.abs(got - G[k]))))
    pairs = eng.so_density2_get("vvvv_pairs")
    ref = np_density2.pairs_of(G["vvvv"])
    _close(pairs, ref, 1e-11, f"{name} vvvv_pairs")
    assert np.array_equal(pairs, pairs.T)
    worst = max(worst, float(np.max(np.abs(pairs - ref))))
    print(name, "largest error of a block", worst)
    e = eng.so_density2_energy()
    fam = np_density2.family_energies(G, c["g"], o)
    for k, x, y in zip(NAMES + ("vvvv",), e[1:7], fam):
        err = abs(x - y)
        print(name, "1/4 g Gamma over", k, x, "error", err)
        assert err < 1e-11 * max(1.0, abs(y))
    L = np_lambda.lagrangian(c["cc"], *r["t"], *r["l"])
    print(name, "density-side Lagrangian", e[0] + e[7], "reference", L)
    assert abs(e[0] + e[7] - L) < 1e-11 * max(1.0, abs(L))
