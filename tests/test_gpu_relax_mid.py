"""The orbital gradient at mid-size extents against the explicit numpy form alone (np_relax.gradient_explicit: X = f D + 1/2 g Gamma over
the whole arrays, itself held to the defining finite difference on the CPU): the shapes of test_gpu_density2_mid.py -- 10,18 (RHF-fed;
153 pair columns, an odd count, one per block), 9,13 (odd extents, every f term, two occupied tiles of a work item) and 12,46 (1035 pair
columns over 345 blocks of 3: a real split of K; 46 x 2 work items) -- with its random O(0.3) amplitudes.  At 12,46 the pair-row kernel
also runs on its other paths, forced through AFESP_RELAX_MCAP / AFESP_RELAX_QCAP: columns walked in LDS segments of at most 300 doubles
(a dozen segments of whole b), and the (i,b) slice of Q read through the caches instead of LDS.

Rule: 1e-11 x max(1, max |ref|).  Largest error measured on the MI355X: 1.4e-14 at 9,13, 3.9e-14 at 10,18, 7.7e-13 at 12,46 (max |w| 345)."""
import numpy as np
import pytest

import np_density2
import np_relax
from test_gpu_lambda import _close, _feed
from test_gpu_lambda_mid import EXTENTS, MID, _ref

pytestmark = pytest.mark.gpu

_W = {}


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _w(name):
    """the explicit gradient (both flags), the two pair-row terms and A x at the shape's first amplitudes, made once"""
    if name not in _W:
        r = _ref(name)
        c = r["c"]
        o, v = EXTENTS[name]
        G = np_density2.gamma_explicit(*r["t"], *r["l"])
        F = np_density2.expand(G, o, v)
        w = [np_relax.gradient_explicit(c["g"], c["f"], o, r["density"], F, fr) for fr in (0, 1)]
        del F
        _, terms = np_relax.gradient_blocks(c["cc"], c["f"], r["density"], G, 1)
        x = np.random.default_rng(11).uniform(-1.0, 1.0, (o, v))
        g = c["g"]
        lev = np.diag(c["f"])
        y = (np.einsum("abij,jb->ia", g[o:, o:, :o, :o], x, optimize=True) + np.einsum("ajib,jb->ia", g[o:, :o, :o, o:], x, optimize=True)
             + (lev[None, o:] - lev[:o, None]) * x)
        _W[name] = dict(w=w, terms=terms, x=x, y=y)
    return _W[name]


@pytest.mark.parametrize("name", sorted(MID))
def test_gradient_at_mid_size(eng, monkeypatch, name):
    r, ref = _ref(name), _w(name)
    _feed(eng, r["c"])
    eng.so_set_amplitudes(*r["t"])
    eng.so_lambda_init(0)
    eng.so_set_lambda(*r["l"])
    eng.so_density2_build()
    before = eng.launch_counts()
    eng.so_orbital_gradient(1)
    after = eng.launch_counts()
    print(name, "GEMM-layer launches of one gradient", {k: after[k] - before[k] for k in after})
    worst = 0.0
    for fr in (0, 1):
        w = eng.so_orbital_gradient(fr)
        _close(w, ref["w"][fr], 1e-11, f"{name} w fock_response={fr}")
        worst = max(worst, float(np.max(np.abs(w - ref["w"][fr]))))
        assert np.array_equal(eng.so_orbital_gradient(fr), w)
    plain = []
    for which, key in ((0, "pair_ai"), (1, "pair_ia")):
        out, _ = eng.so_relax_pair_row(which)
        _close(out, ref["terms"][key], 1e-11, f"{name} pair-row term {key}")
        worst = max(worst, float(np.max(np.abs(out - ref["terms"][key]))))
        plain.append(out)
    _close(eng.so_zvector_apply(ref["x"]), ref["y"], 1e-11, f"{name} A x")
    print(name, "largest error", worst, "max |w|", float(np.max(np.abs(ref["w"][1]))))
    if name != "rhf_cap":
        return
    for knob, val in (("AFESP_RELAX_MCAP", "300"), ("AFESP_RELAX_QCAP", "0")):      # segments of whole b; Q through the caches
        monkeypatch.setenv(knob, val)
        for which, key in ((0, "pair_ai"), (1, "pair_ia")):
            out, _ = eng.so_relax_pair_row(which)
            _close(out, ref["terms"][key], 1e-11, f"{name} pair-row term {key} with {knob}={val}")
            if knob == "AFESP_RELAX_QCAP":
                assert np.array_equal(out, plain[which])                            # the same sums in the same order
        _close(eng.so_orbital_gradient(1), ref["w"][1], 1e-11, f"{name} w with {knob}={val}")
        monkeypatch.delenv(knob)
