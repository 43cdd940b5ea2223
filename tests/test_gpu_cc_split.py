"""The rank-split closed-shell CCSD iteration (csrc/ccsd.hip: slice_bounds, pp_b_range, the s.sharded branches of ccsd_intermediates /
ccsd_amplitudes, ooov_sh, the ladder on row ranges) rank by rank on ONE device, term by term against the oracle.

AFESP_CC_TIME_SLICE="rank,world" makes a context without a communicator do rank `rank`'s share of a `world`-rank split iteration and skip
the exchange; knobs follow the environment call by call.  One engine plays every rank in turn from the same O(1) amplitudes (t1, t2 =
0.3 N(0,1): a missing or mis-sliced term, the t1^4 parts of c included, shows at 1e-3 of a tensor's scale or more) and the test does the
all-reduce itself: sum over ranks of r2 and of r1_sh.  tests/test_gpu_ranks.py stays the only test of the exchange.

Cases (o, v, world): a-slices [v rank / world, v (rank + 1) / world) of the last index of I_ovov / I_voov / x_voov / ooov_sh and of the
columns of I_vv; ladder b-ranges by pp_b_range's square-root cuts.  Both restated as literals in CASES and held against the supports the
engine shows (the non-zero rows of a rank's packed PP; the a of the ooov_sh buffer that a rank's pass changes, bit for bit -- the getter
serves both buffers as they lie).
    4, 9, 2    a [0,4) [4,9)                    b [0,6) [6,9)                   odd v, unequal slices, a-slice != b-range on a rank
    5, 13, 3   a [0,4) [4,8) [8,13)             b [0,8) [8,11) [11,13)          odd o (no 16-byte staging), odd pair counts
    6, 10, 4   a [0,2) [2,5) [5,7) [7,10)       b [0,5) [5,7) [7,9) [9,10)      slices of 2 and 3, last b-range one column
    3, 5, 8    a ranks 0, 2, 5 empty, others 1  b ranks 2, 4, 5, 7 empty        v1 == v0, p1 == p0, q1 == q0 guards; world > v
    2, 4, 3    a [0,1) [1,2) [2,4)              b [0,2) [2,3) [3,4)             one antisymmetric occupied pair
    1, 6, 2    a [0,3) [3,6)                    b [0,4) [4,6)                   o == 1: I_vv written whole then added to, pp_pa null
    12, 40, 8  a eight slices of 5              b [0,14) [14,20) [20,24) [24,28) [28,32) [32,35) [35,37) [37,40)
                                                                                the benchmark's rank count; o v = 480, 820 pair rows
Each with AFESP_PP_SYM = 0 and 1.

Tolerance: |engine - oracle| < 1e-11 max(1, max|oracle|) per tensor, the bound the unsplit pass of the same case is
held to in the same test (the yardstick: the split results sum the same products, at most regrouped over two ranks per element).
Largest error / bound over all comparisons of a case, as printed on the MI355X (the unsplit pass | the split passes and their sums):
                 AFESP_PP_SYM=0         AFESP_PP_SYM=1
    1, 6, 2    5.6e-06 | 6.2e-06      5.6e-06 | 6.2e-06
    2, 4, 3    8.3e-06 | 8.3e-06      1.1e-05 | 8.3e-06
    3, 5, 8    1.7e-05 | 1.7e-05      1.7e-05 | 1.7e-05
    4, 9, 2    7.8e-05 | 7.8e-05      7.8e-05 | 7.8e-05
    5, 13, 3   2.1e-04 | 2.2e-04      2.1e-04 | 2.2e-04
    6, 10, 4   3.2e-04 | 3.7e-04      3.2e-04 | 3.7e-04
    12, 40, 8  2.2e-03 | 1.8e-03      2.2e-03 | 1.8e-03
(at 12, 40 the unsplit pass is 1.2e-13 off in r1 against a bound of 6.8e-11: 1e-11 holds there with room, no case needs another bound).
The state-hazard test: 3.6e-04 against the oracle, and every pass bit for bit the pass it is held against.  The whole file runs in about 1.3 s.
"""
import functools

import numpy as np
import pytest

import molecules
import orc
from test_gpu_cc import INTERMEDIATES, _p

pytestmark = pytest.mark.gpu

# (o, v, world): (a-slices, ladder b-ranges), rank by rank -- slice_bounds and pp_b_range of csrc/ccsd.hip restated by hand
CASES = {
    (4, 9, 2): ([(0, 4), (4, 9)], [(0, 6), (6, 9)]),
    (5, 13, 3): ([(0, 4), (4, 8), (8, 13)], [(0, 8), (8, 11), (11, 13)]),
    (6, 10, 4): ([(0, 2), (2, 5), (5, 7), (7, 10)], [(0, 5), (5, 7), (7, 9), (9, 10)]),
    (3, 5, 8): ([(0, 0), (0, 1), (1, 1), (1, 2), (2, 3), (3, 3), (3, 4), (4, 5)],
                [(0, 2), (2, 3), (3, 3), (3, 4), (4, 4), (4, 4), (4, 5), (5, 5)]),
    (2, 4, 3): ([(0, 1), (1, 2), (2, 4)], [(0, 2), (2, 3), (3, 4)]),
    (1, 6, 2): ([(0, 3), (3, 6)], [(0, 4), (4, 6)]),
    (12, 40, 8): ([(5 * r, 5 * r + 5) for r in range(8)],
                  [(0, 14), (14, 20), (20, 24), (24, 28), (28, 32), (32, 35), (35, 37), (37, 40)]),
}
REPLICATED = ["asym_t2", "c_oovv", "I_vo", "I_oo_p", "I_oo", "I_oooo"]
SLICED = ["I_ovov", "I_voov", "x_voov", "I_vv"]      # the slice is the last index of each (the column a of I_vv(b,a))
SPLIT_ONLY = ["r1_sh", "pp", "ooov_sh"]
TOL = 1e-11


class _Worst:
    """largest error / bound of the comparisons made through it"""
    def __init__(self):
        self.ratio = 0.0

    def close(self, x, ref, what, tol=TOL):
        err, bound = float(np.max(np.abs(x - ref))), tol * max(1.0, float(np.max(np.abs(ref))))
        print(what, "error", err, "bound", bound)
        self.ratio = max(self.ratio, err / bound)
        assert err < bound, what


@pytest.fixture(scope="module")
def eng():
    """runs unsplit passes only"""
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_split():
    """never runs an unsplit iteration"""
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _system(o, v):
    """tests/test_gpu_cc.py::test_one_iteration_term_by_term's two recipes"""
    if o * v > 100:
        from afesp_amd import inputs
        e = np.concatenate([-2.0 + np.arange(o) / (o - 1), 1.0 + 2.0 * np.arange(v) / (v - 1)])
        eri = 0.02 * (2.0 * np.random.default_rng(11).random(inputs.neri(o + v)) - 1.0)
        return e, eri
    n, e, eri = molecules.synthetic_system(o, v, scale=0.05)
    return e, eri


@functools.lru_cache(maxsize=None)
def _reference(o, v):
    """System, amplitudes and ONE oracle pass from them -- shared by every test of the extents, never modified."""
    e, eri = _system(o, v)
    rng = np.random.default_rng(100 * o + v)
    t1 = 0.3 * rng.standard_normal((o, v))
    t2 = 0.3 * rng.standard_normal((o, o, v, v))
    t2 = 0.5 * (t2 + t2.transpose(1, 0, 3, 2))       # t2(ijab) = t2(jiba)
    cc = orc.OracleCC(o, v, eri, e, 8)
    cc.t1[...] = t1
    cc.t2[...] = t2
    cc.L.orc_cc_intermediates(cc.h)
    ref = {name: np.array(cc.field(name)) for name in INTERMEDIATES}
    ref["bare_ooov"] = np.array(cc.field("v_oovo")).transpose(1, 0, 3, 2)       # I_ooov_p(j,k,i,a) = <kj|ai> + ...
    cc.L.orc_cc_amplitudes(cc.h)
    ref["r1"], ref["r2"] = np.array(cc.field("r1")), np.array(cc.field("r2"))
    ref["t1_new"], ref["t2_new"] = np.array(cc.t1), np.array(cc.t2)
    cc.close()
    for a in list(ref.values()) + [t1, t2]:
        a.setflags(write=False)
    return e, eri, t1, t2, ref


def _tiles(ranges, v):
    """disjoint, in order, covering [0, v)"""
    return ranges[0][0] == 0 and ranges[-1][1] == v and all(lo <= hi for lo, hi in ranges) and \
        all(ranges[k][1] == ranges[k + 1][0] for k in range(len(ranges) - 1))


def _rank_pass(eng, t1, t2, rank, world, monkeypatch, iterate=False, only=None):
    """rank `rank`'s share of a `world`-rank split iteration from (t1, t2): everything the getter serves, and the amplitudes that come out
    (only: the intermediates alone, and that one tensor of them)"""
    monkeypatch.setenv("AFESP_CC_TIME_SLICE", f"{rank},{world}")
    eng.set_amplitudes(t1, t2)
    if only:
        eng.update_intermediates()
        out = eng.tensor(only)
        monkeypatch.delenv("AFESP_CC_TIME_SLICE")
        return out
    if iterate:                 # the ordinary entry point: both halves and the tail in one call
        eng.ccsd_iterate(1e-6, 1e-7)
        out = {}
    else:
        eng.update_intermediates()
        out = {name: eng.tensor(name) for name in REPLICATED + SLICED + ["I_ooov_p", "ooov_sh"]}
        eng.update_amplitudes()
        out.update({name: eng.tensor(name) for name in ("r1", "r2", "r1_sh", "pp")})
    out["t1_new"], out["t2_new"] = eng.amplitudes()
    monkeypatch.delenv("AFESP_CC_TIME_SLICE")
    return out


def _unsplit_pass(eng, t1, t2, names=INTERMEDIATES):
    eng.set_amplitudes(t1, t2)
    eng.update_intermediates()
    out = {name: eng.tensor(name) for name in names}
    eng.update_amplitudes()
    out["r1"], out["r2"] = eng.tensor("r1"), eng.tensor("r2")
    out["t1_new"], out["t2_new"] = eng.amplitudes()
    return out


@pytest.mark.parametrize("pp_sym", ["0", "1"])
@pytest.mark.parametrize("o,v,world", sorted(CASES))
def test_every_rank_of_the_split_iteration_term_by_term(eng, eng_split, o, v, world, pp_sym, monkeypatch):
    a_slices, b_ranges = CASES[(o, v, world)]
    assert len(a_slices) == world and len(b_ranges) == world and _tiles(a_slices, v) and _tiles(b_ranges, v)
    monkeypatch.setenv("AFESP_PP_SYM", pp_sym)
    monkeypatch.delenv("AFESP_CC_TIME_SLICE", raising=False)
    e, eri, t1, t2, ref = _reference(o, v)
    tag = f"({o},{v}) pp_sym {pp_sym}"
    # ---- the yardstick: one unsplit pass against the same oracle pass, same bound
    plain = _Worst()
    eng.ccsd_init(o, v, e, eri, 8)
    u = _unsplit_pass(eng, t1, t2)
    for name in INTERMEDIATES:
        plain.close(u[name], ref[name], f"{tag} unsplit {name}")
    plain.close(u["r1"], ref["r1"], f"{tag} unsplit r1")
    plain.close(_p(u["r2"]), _p(ref["r2"]), f"{tag} unsplit P r2")
    plain.close(u["t1_new"], ref["t1_new"], f"{tag} unsplit new t1")
    plain.close(u["t2_new"], ref["t2_new"], f"{tag} unsplit new t2")
    # ---- every rank in turn
    split = _Worst()
    eng_split.ccsd_init(o, v, e, eri, 8)
    # The getter serves the ooov_sh buffer as it lies, and outside a rank's slice it holds what earlier calls left (at first: whatever the
    # allocation held).  So every rank writes its slice once from OTHER amplitudes first; each pass below must then change, bit for bit,
    # exactly the a of its slice -- a write outside the slice by the sliced pair form or contraction would show as a changed a.
    for rank in range(world):
        osh_before = _rank_pass(eng_split, 0.5 * t1, 0.5 * t2, rank, world, monkeypatch, only="ooov_sh")
    ranks = [_rank_pass(eng_split, t1, t2, rank, world, monkeypatch) for rank in range(world)]
    b_of_p = np.repeat(np.arange(v), np.arange(1, v + 1))       # PP(i,j,p): p = a + b (b + 1) / 2 over a <= b
    a_of = np.arange(v)
    for rank, (g, (v0, v1), (b0, b1)) in enumerate(zip(ranks, a_slices, b_ranges)):
        rt = f"{tag} rank {rank}/{world}"
        for name in REPLICATED:
            split.close(g[name], ref[name], f"{rt} {name}")
            assert np.array_equal(g[name], ranks[0][name]), (rt, name)      # same kernels, same order on every rank
        if v1 > v0:                                                          # (outside the slice: stale by design, nothing asserted)
            for name in SLICED:
                split.close(g[name][..., v0:v1], ref[name][..., v0:v1], f"{rt} {name}[..., {v0}:{v1}]")
            split.close(g["ooov_sh"][..., v0:v1], (ref["I_ooov_p"] - ref["bare_ooov"])[..., v0:v1], f"{rt} ooov_sh[..., {v0}:{v1}]")
        split.close(g["I_ooov_p"], ref["bare_ooov"], f"{rt} I_ooov_p = the bare term")
        # supports, read from the buffers themselves: the a of ooov_sh that this pass wrote and the non-zero rows of its packed ladder
        # (zeroed whole by every split update) are exactly the ranges restated above
        wrote = np.any(g["ooov_sh"].view(np.int64) != osh_before.view(np.int64), axis=(0, 1, 2))
        assert np.array_equal(wrote, (a_of >= v0) & (a_of < v1)), (rt, wrote)
        osh_before = g["ooov_sh"]
        assert np.array_equal(np.any(g["pp"] != 0.0, axis=(0, 1)), (b_of_p >= b0) & (b_of_p < b1)), rt
        assert np.all(np.isfinite(g["r2"])) and np.all(np.isfinite(g["r1"]))
    # ---- the exchange, done here: sum over ranks of the partial residuals
    split.close(_p(sum(g["r2"] for g in ranks)), _p(ref["r2"]), f"{tag} P sum_rank r2")
    repl = [g["r1"] - g["r1_sh"] for g in ranks]
    split.close(sum(g["r1_sh"] for g in ranks) + repl[0], ref["r1"], f"{tag} sum_rank r1_sh + replicated r1")
    # the replicated part is the same on every rank -- up to the rounding of r1 = replicated + r1_sh on the device and of the
    # difference here: two roundings of numbers no larger than max|r1| + max|r1_sh|
    for rank, g in enumerate(ranks):
        slack = 4.0 * np.finfo(float).eps * (np.max(np.abs(g["r1"])) + np.max(np.abs(g["r1_sh"])) + np.max(np.abs(ranks[0]["r1"])) +
                                             np.max(np.abs(ranks[0]["r1_sh"])))
        assert np.max(np.abs(repl[rank] - repl[0])) <= slack, (tag, rank)
    print(f"WORST {tag} world {world}: unsplit {plain.ratio:.1e} split {split.ratio:.1e} (error / bound)")


def _same(x, y, what, worst, bitwise=True):
    """within the tolerance; bitwise: and bit for bit, as observed on the MI355X -- the same kernels in the same order on the same data"""
    worst.close(x, y, what)
    if bitwise:
        assert np.array_equal(x, y), what


def test_no_state_carries_over_between_unsplit_and_sliced_passes(monkeypatch):
    """Unsplit iterations down the ring / LDS-DMA path (r1x_valid, cs_packed, live ring buffers) alternating with sliced ones on ONE
    state: the unsplit passes give what a fresh engine's single unsplit pass gives, the sliced ones what the same ranks give in an engine
    that never ran unsplit -- no flag (ring live / packed / res_live, r1x_valid, cs_packed, partials_live, amps_touched) and no buffer
    (pp, r2_sh, r1_sh, ooov_sh) carries over.  And through the ordinary entry point: afesp_ccsd_iterate with the knob set leaves the
    amplitudes that update_intermediates + update_amplitudes left for that rank."""
    from afesp_amd.capi import AfespError, Engine, load_library
    o, v, world = 6, 10, 4
    a_slices, _ = CASES[(o, v, world)]
    monkeypatch.setenv("AFESP_SMALL_MAX", "0")
    monkeypatch.setenv("AFESP_RING_TG_MIN", "1")
    monkeypatch.setenv("AFESP_PP_SYM", "1")
    monkeypatch.delenv("AFESP_CC_TIME_SLICE", raising=False)
    assert load_library().afesp_test_ring_path(o, v) == 1       # the unsplit passes take the ring launches
    e, eri, t1, t2, ref = _reference(o, v)
    w = _Worst()
    with Engine(0) as fresh:
        fresh.ccsd_init(o, v, e, eri, 8)
        u0 = _unsplit_pass(fresh, t1, t2)
    for name in INTERMEDIATES + ["r1", "t1_new", "t2_new"]:
        w.close(u0[name], ref[name], f"fresh unsplit {name}")
    w.close(_p(u0["r2"]), _p(ref["r2"]), "fresh unsplit P r2")
    with Engine(0) as only_split:
        only_split.ccsd_init(o, v, e, eri, 8)
        s0 = {rank: _rank_pass(only_split, t1, t2, rank, world, monkeypatch) for rank in (1, 3)}
        for rank in (1, 3):
            it = _rank_pass(only_split, t1, t2, rank, world, monkeypatch, iterate=True)       # (another update kernel: the tolerance)
            _same(it["t1_new"], s0[rank]["t1_new"], f"rank {rank}: t1 of ccsd_iterate against the two calls", w, bitwise=False)
            _same(it["t2_new"], s0[rank]["t2_new"], f"rank {rank}: t2 of ccsd_iterate against the two calls", w, bitwise=False)
    with Engine(0) as mixed:
        mixed.ccsd_init(o, v, e, eri, 8)
        for step, rank in enumerate((None, 1, None, 3, None)):
            if rank is None:
                u = _unsplit_pass(mixed, t1, t2)
                for name in INTERMEDIATES + ["r1", "t1_new", "t2_new"]:
                    _same(u[name], u0[name], f"step {step} unsplit {name}", w)
                _same(_p(u["r2"]), _p(u0["r2"]), f"step {step} unsplit P r2", w)
                for name in SPLIT_ONLY:       # ... and the split-only names are refused again
                    with pytest.raises(AfespError, match="ran split"):
                        mixed.tensor(name)
            else:
                g = _rank_pass(mixed, t1, t2, rank, world, monkeypatch)
                v0, v1 = a_slices[rank]
                for name in REPLICATED + ["I_ooov_p", "r1", "r2", "r1_sh", "pp", "t1_new", "t2_new"]:
                    _same(g[name], s0[rank][name], f"step {step} rank {rank} {name}", w)
                for name in SLICED + ["ooov_sh"]:
                    _same(g[name][..., v0:v1], s0[rank][name][..., v0:v1], f"step {step} rank {rank} {name}[..., {v0}:{v1}]", w)
    print(f"WORST state hazards: {w.ratio:.1e} (error / bound)")


def test_split_only_tensors_are_refused_after_unsplit_calls(monkeypatch):
    """r1_sh, pp and ooov_sh are what a split call left: status 1 with a message that says so before any iteration and after unsplit
    ones -- ooov_sh follows the last update of the intermediates, r1_sh / pp the last update of the amplitudes -- and the engine stays usable."""
    from afesp_amd.capi import AfespError, Engine
    o, v, world = 4, 9, 2
    monkeypatch.setenv("AFESP_PP_SYM", "1")
    monkeypatch.delenv("AFESP_CC_TIME_SLICE", raising=False)
    e, eri, t1, t2, ref = _reference(o, v)

    def refused(eng, names):
        for name in names:
            with pytest.raises(AfespError, match=r"status 1: .*" + name + r".*ran split"):
                eng.tensor(name)

    w = _Worst()
    with Engine(0) as eng:
        eng.ccsd_init(o, v, e, eri, 8)
        refused(eng, SPLIT_ONLY)                                    # no iteration yet
        u = _unsplit_pass(eng, t1, t2)
        refused(eng, SPLIT_ONLY)
        w.close(u["r1"], ref["r1"], "unsplit r1 after refusals")
        g = _rank_pass(eng, t1, t2, 1, world, monkeypatch)          # served, and right, after a split pass
        v0, v1 = CASES[(o, v, world)][0][1]
        w.close(g["ooov_sh"][..., v0:v1], (ref["I_ooov_p"] - ref["bare_ooov"])[..., v0:v1], "ooov_sh after refusals")
        assert eng.tensor("pp").shape == (o, o, v * (v + 1) // 2) and eng.tensor("r1_sh").shape == (o, v)
        eng.set_amplitudes(t1, t2)
        eng.update_intermediates()                                  # unsplit intermediates: ooov_sh is gone, the residual's parts are not
        refused(eng, ["ooov_sh"])
        eng.tensor("r1_sh"), eng.tensor("pp")
        eng.update_amplitudes()
        refused(eng, SPLIT_ONLY)
        eng.ccsd_init(o, v, e, eri, 8)                              # initialised again where it lies: nothing left over
        monkeypatch.setenv("AFESP_CC_TIME_SLICE", f"0,{world}")
        eng.set_amplitudes(t1, t2)
        eng.update_intermediates()
        eng.tensor("ooov_sh")
        monkeypatch.delenv("AFESP_CC_TIME_SLICE")
        eng.ccsd_init(o, v, e, eri, 8)
        refused(eng, SPLIT_ONLY)
        u = _unsplit_pass(eng, t1, t2)                              # ... and the engine is as good as new
        w.close(_p(u["r2"]), _p(ref["r2"]), "unsplit P r2 at the end")
        w.close(u["t2_new"], ref["t2_new"], "unsplit new t2 at the end")
