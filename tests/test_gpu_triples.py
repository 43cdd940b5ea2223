"""The perturbative-triples pipeline (csrc/triples.hip, csrc/triples_orbit.h) triple by triple against np_triples.py.

Amplitudes of order one are handed in (afesp_ccsd_set_amplitudes after afesp_ccsd_init: no solve), so the t1 terms -- Z, y, the plain
variant's sum Z t_bar, the f_ov t2 term of the Fock states -- weigh as much as W; every flat index [t, t+1) of the engine's list is run
alone, so a weight, a pad bit, a stabiliser division or the enumeration itself cannot hide in a total.

Tolerance, per range and per reported quantity: |engine - reference| <= (2 (v + o) + 64) 2^-53 S, S the reference's majorant summed over the
range (np_triples.tol_factor; derivation there and in test_triples_cpu.py, where the oracle is held to the same bound).
Largest error / bound seen on an MI355X: see LARGEST_SEEN below."""
import re

import numpy as np
import pytest

import np_triples as T

pytestmark = pytest.mark.gpu

# largest |engine - reference| / bound over everything the tests compare, as measured on an MI355X (every test prints its own; -s shows
# it).  The bound is a worst case over summation orders and the roundings are of independent sign, hence the distance; the constant is
# the derivation's and is not tuned to these figures.
LARGEST_SEEN = {"spin-free": 1.8e-3, "spin-orbital": 7e-4}

VARIANTS = ("full", "plain", "cr")
NOUT = {"full": 4, "plain": 2, "cr": 6}
KERNELS = {"tgemm": {}, "gett": {"AFESP_T_GEMM": "gett"}, "gett-split": {"AFESP_T_GEMM": "gett", "AFESP_T_SPLIT_TILES": "1"}}
DEBUG_LINE = re.compile(r"afesp \(T\): o (\d+) v (\d+) block (\d+) chunks (\d+) kernel (\w+)")


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _knobs(monkeypatch, kernel="tgemm", **more):
    for k, val in dict(KERNELS[kernel], AFESP_T_DEBUG="1", **more).items():
        monkeypatch.setenv(k, str(val))


def _load(eng, c, cr=True):
    """The state of case c with its amplitudes; cr: the completely renormalised intermediates from the same amplitudes, I_vo and asym_t2
    included (the reference's data flow takes those two from the last update of the intermediates)"""
    eng.ccsd_init(c.o, c.v, c.e, c.eri, 2)
    _amplitudes(eng, c, cr)


def _amplitudes(eng, c, cr=True):
    eng.set_amplitudes(c.t1, c.t2)
    if cr:
        eng.update_intermediates()
        eng.build_cr_intermediates()


def _call(eng, variant, a, b):
    return {"full": eng.do_ccsd_t_spatial, "plain": eng.do_ccsd_t_spatial_plain, "cr": eng.do_ccsd_t_spatial_cr}[variant](a, b)


class Checker:
    """Runs ranges of the engine's list and holds each to the reference; keeps the largest error / bound."""

    def __init__(self, eng, c, order):
        self.eng, self.c, self.order, self.worst = eng, c, order, 0.0

    def run(self, variant, a, b, c=None):
        c = c or self.c
        n = NOUT[variant]
        out = _call(self.eng, variant, a, b)
        ref, bound = T.expected(c, self.order[a:b], with_base=(a == 0))
        err = np.abs(out - ref[:n])
        print(variant, (a, b), "error / bound", np.array2string(err / bound[:n], precision=3))
        assert np.all(err <= bound[:n]), (variant, a, b, self.order[a:b][:3], out, ref[:n], err / bound[:n])
        self.worst = max(self.worst, float(np.max(err / bound[:n])))
        return out, bound[:n]

    def parts_and_whole(self, variant, cuts):
        """the ranges between consecutive cuts, each against the reference, and their sum against the whole"""
        whole, bound = self.run(variant, cuts[0], cuts[-1])
        parts = sum(self.run(variant, a, b)[0] for a, b in zip(cuts, cuts[1:]))
        assert np.all(np.abs(parts - whole) <= 2 * bound), (variant, cuts, parts, whole)
        return whole

    def report(self, what="spin-free"):
        print(f"largest error / bound ({what}): {self.worst:.4f}")


def _debug(capfd):
    return [(int(m[1]), int(m[2]), int(m[3]), int(m[4]), m[5]) for m in DEBUG_LINE.finditer(capfd.readouterr().err)]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("o,v", T.CASES)
def test_every_triple_alone(eng, o, v, kernel, monkeypatch, capfd):
    """[t, t+1) for every t, the whole list, and the parts against the whole: full, plain (WANT_D = false) and completely renormalised, on
    the LDS-DMA GEMM, on the grouped gather kernel, and on the latter with the coinciding-pair groups in a launch of their own."""
    _knobs(monkeypatch, kernel)
    c = T.case(o, v)
    _load(eng, c)
    sb = eng.t_block_size()
    assert sb == o == eng.t_block_size(cr=True)          # at these extents one block holds every occupied index
    order = T.fused_order(o, sb)
    nt = len(order)
    assert eng.ntriples() == nt
    ck = Checker(eng, c, order)
    for variant in VARIANTS:
        _debug(capfd)
        ck.parts_and_whole(variant, list(range(nt + 1)))
        lines = _debug(capfd)
        assert len(lines) == nt + 1 and set(lines) == {(o, v, sb, 1, "tgemm" if kernel == "tgemm" else "gett")}
    ck.report()


@pytest.mark.parametrize("kernel", ["tgemm", "gett-split"])
@pytest.mark.parametrize("block", [1, 2, 99])
@pytest.mark.parametrize("o,v", [(3, 9), (5, 16), (6, 17)])
def test_block_sizes_of_the_enumeration(eng, o, v, block, kernel, monkeypatch, capfd):
    """AFESP_T_BLOCK = 1, 2 (a ragged last block at odd o) and more than o: the flat index follows fused_order of that block size; every
    block triple as a range of its own (one chunk), the whole list (one chunk per block triple), and the first, a middle and the last block
    triple triple by triple."""
    _knobs(monkeypatch, kernel, AFESP_T_BLOCK=block)
    c = T.case(o, v)
    _load(eng, c)
    sb = min(block, o)
    assert eng.t_block_size() == sb
    order, ranges = T.fused_order(o, sb), T.block_triple_ranges(o, sb)
    nt = len(order)
    name = "tgemm" if kernel == "tgemm" else "gett"
    ck = Checker(eng, c, order)
    for variant in VARIANTS:
        _debug(capfd)
        ck.parts_and_whole(variant, [0] + [e for _, e in ranges])
        lines = _debug(capfd)
        assert lines[0] == (o, v, sb, len(ranges), name) and set(lines[1:]) == {(o, v, sb, 1, name)}
        for b, e in {ranges[0], ranges[len(ranges) // 2], ranges[-1]}:
            if e - b > 1:
                ck.parts_and_whole(variant, list(range(b, e + 1)))
        if nt > 3:   # ranges that cut through block triples
            ck.parts_and_whole(variant, [1, nt // 3, 2 * nt // 3, nt])
    ck.report()


@pytest.mark.parametrize("kernel", ["tgemm", "gett"])
@pytest.mark.parametrize("pool", ["AFESP_T_POOL_GIB", "AFESP_T_ONE_POOL"])
@pytest.mark.parametrize("o,v", [(4, 13), (6, 17)])
def test_block_pool_without_a_budget_and_in_one_allocation(eng, o, v, pool, kernel, monkeypatch, capfd):
    """AFESP_T_POOL_GIB=0: blocks of one occupied index, a chunk per triple.  AFESP_T_ONE_POOL: the pool as one allocation instead of
    pieces of idle memory."""
    _knobs(monkeypatch, kernel, **{pool: 0 if pool == "AFESP_T_POOL_GIB" else 1})
    c = T.case(o, v)
    _load(eng, c)
    sb = 1 if pool == "AFESP_T_POOL_GIB" else o
    assert eng.t_block_size() == sb
    order = T.fused_order(o, sb)
    nt = len(order)
    ck = Checker(eng, c, order)
    for variant in VARIANTS:
        _debug(capfd)
        ck.parts_and_whole(variant, [0, 1, nt // 3, nt // 3 + 1, 2 * nt // 3, nt])
        assert _debug(capfd)[0] == (o, v, sb, nt if sb == 1 else 1, "tgemm" if kernel == "tgemm" else "gett")
    ck.report()


def test_base_term_only_where_the_range_starts_at_zero(eng, monkeypatch):
    """1 + 2 sum t1^2 + sum asym_t2 c_oovv enters D[T] and D(T) of the caller that holds flat index 0, and of nobody else."""
    o, v = 3, 9
    c = T.case(o, v)
    _load(eng, c)
    order = T.fused_order(o, eng.t_block_size())
    nt = len(order)
    ck = Checker(eng, c, order)
    base = float(c.base[0])
    assert base > 10.0
    for variant in ("full", "cr"):
        with0, bound = ck.run(variant, 0, nt)
        first, _ = ck.run(variant, 0, 1)
        rest, _ = ck.run(variant, 1, nt)
        ck.run(variant, 1, 2)                                 # (held to a reference without it)
        assert np.all(np.abs(first + rest - with0) <= 2 * bound)
        # triple (0,0,0) itself is zero (np_triples): what [0, 1) reports is the base term
        assert np.all(np.abs(first[2:4] - base) <= bound[2:4]) and np.all(np.abs(first[:2]) <= bound[:2])
    ck.report()


def test_more_partial_sums_than_one_launch_takes(eng, monkeypatch, capfd):
    """8436 triples x one cube orbit in ONE chunk: ranges of 8192 partial sums (summed and published in one launch) and of more (the
    two-stage sum_partials), with and without the base term behind them; then the same list in ten chunks of up to 364 triples."""
    o, v = T.LARGE_CASE
    _knobs(monkeypatch)
    c = T.case(o, v)
    _load(eng, c)
    assert eng.t_block_size() == o
    order = T.fused_order(o, o)
    nt = len(order)
    assert nt == 8436 and T.facts(o, v)["norb"] == 1
    ck = Checker(eng, c, order)
    for variant in VARIANTS:
        _debug(capfd)
        ck.parts_and_whole(variant, [1, 8193, nt])           # 8192 partials, then 243
        ck.parts_and_whole(variant, [0, 3, 8196, nt])        # 8193 partials in the middle
        assert set(_debug(capfd)) == {(o, v, o, 1, "tgemm")}
    monkeypatch.setenv("AFESP_T_BLOCK", "12")
    assert eng.t_block_size() == 12
    ck = Checker(eng, c, T.fused_order(o, 12))
    ranges = T.block_triple_ranges(o, 12)
    assert len(ranges) == 10
    for variant in VARIANTS:
        _debug(capfd)
        ck.parts_and_whole(variant, [0, ranges[4][0] + 5, ranges[7][1], nt])
        assert _debug(capfd)[0] == (o, v, 12, 10, "tgemm")
    ck.report()


@pytest.mark.parametrize("kernel", ["tgemm", "gett"])
def test_operand_copies_follow_the_amplitudes_and_the_intermediates(eng, kernel, monkeypatch):
    """The concatenated operands are cached while the amplitude epoch, the epoch of the completely renormalised intermediates and the
    scratch epoch stand: (T), new amplitudes, (T) again must give the new amplitudes' values, in every variant and order of variants;
    likewise across afesp_ccsd_cr_intermediates alone (amplitudes of one set with intermediates of the other)."""
    _knobs(monkeypatch, kernel)
    o, v = 4, 13
    c0, c1 = T.case(o, v), T.case(o, v, 1)
    assert np.max(np.abs(c0.t2 - c1.t2)) > 0.5
    _load(eng, c0)
    order = T.fused_order(o, eng.t_block_size())
    nt = len(order)
    ck = Checker(eng, c0, order)
    cuts = [0, 2, nt // 2, nt]
    for first in VARIANTS:
        for c in (c1, c0):
            for variant in (first,) + tuple(x for x in VARIANTS if x != first):
                ck.run(variant, 2, nt // 2, c=ck.c)          # leaves its operand copies and plan behind
            _amplitudes(eng, c)
            ck.c = c
            for variant in (first,) + tuple(x for x in VARIANTS if x != first):
                ck.parts_and_whole(variant, cuts)
    # the completely renormalised intermediates of c1 under the amplitudes of c0, and back
    vvov, oovo, oovv = T.slices(o, v, c0.eri)
    val, S = T.spin_free_ordered(c0.e, c0.t1, c0.t2, vvov, oovo, oovv, c1.ipp, c1.ioo)
    mixed = c0._replace(val=T.sorted_sums(T.reported(val)), S=T.sorted_sums(T.reported(S)))
    _amplitudes(eng, c1)
    ck.c = c1
    ck.run("cr", 0, nt)
    eng.set_amplitudes(c0.t1, c0.t2)                     # amplitude epoch only
    ck.c = mixed
    ck.parts_and_whole("cr", cuts)
    eng.update_intermediates()
    eng.build_cr_intermediates()                          # epoch of the intermediates only
    ck.c = c0
    ck.parts_and_whole("cr", cuts)
    ck.report()


@pytest.mark.parametrize("o,v", [(3, 9), (5, 16)])
def test_cached_plan_follows_the_plan_shaping_knobs(eng, o, v, monkeypatch, capfd):
    """Every knob follows the environment per C-ABI call (csrc/knobs.h).  For a sub-range the flat order depends on AFESP_T_BLOCK: the same
    range after another block size must be the new order's triples, not the cached plan's; AFESP_T_POOL_GIB, AFESP_T_ONE_POOL and
    AFESP_T_SPLIT_TILES shape the plan as well (block size, pool, launches of the coinciding-pair groups)."""
    _knobs(monkeypatch)
    c = T.case(o, v)
    _load(eng, c)
    a, b = 1, 4
    two, all_ = T.fused_order(o, 2), T.fused_order(o, o)
    assert set(two[a:b]) != set(all_[a:b])
    for variant in VARIANTS:
        for block, order in ((2, two), (o, all_), (2, two)):
            monkeypatch.setenv("AFESP_T_BLOCK", str(block))
            assert eng.t_block_size() == block
            _debug(capfd)
            Checker(eng, c, order).run(variant, a, b)
            assert _debug(capfd) == [(o, v, block, len({(i // block, j // block, k // block) for i, j, k in order[a:b]}), "tgemm")]
        monkeypatch.delenv("AFESP_T_BLOCK")
        # same range, same order (blocks of one index list the triples as one block of all does), another plan
        Checker(eng, c, all_).run(variant, a, b)
        monkeypatch.setenv("AFESP_T_POOL_GIB", "0")
        _debug(capfd)
        Checker(eng, c, all_).run(variant, a, b)
        assert _debug(capfd) == [(o, v, 1, b - a, "tgemm")]
        monkeypatch.delenv("AFESP_T_POOL_GIB")
        for knob in ("AFESP_T_ONE_POOL", "AFESP_T_SPLIT_TILES"):
            monkeypatch.setenv("AFESP_T_GEMM", "gett")
            Checker(eng, c, all_).run(variant, a, b)
            monkeypatch.setenv(knob, "1")
            Checker(eng, c, all_).run(variant, a, b)
            monkeypatch.delenv(knob)
            monkeypatch.delenv("AFESP_T_GEMM")


# ------------------------------------------------------------------------------------------------------------ spin-orbital
def _load_so(eng, c):
    n, o = c.n, c.o
    if c.fock:
        eng.do_mp2_spatial(n, c.na, np.eye(n), c.e, c.eri, want_eri_mo=False)     # leaves the AO (= MO) integrals resident
        eng.mo_rotate_uhf(n, np.eye(n), np.eye(n))
        eng.uso_init_fock(n, c.na, c.nb, c.fa, c.fb, 2)
        assert np.array_equal(eng.so_tensor("f_ov"), c.f_ov)
        assert not np.any(eng.so_tensor("f_oo")) and not np.any(eng.so_tensor("f_vv"))
    else:
        eng.init_cc_spinorb(n, o, c.e, c.eri, 2)
    assert (eng.so_o, eng.so_v) == (c.o, c.v)
    assert np.max(np.abs(eng.so_tensor("oovv") - c.g[:o, :o, o:, o:])) < 1e-14
    eng.so_set_amplitudes(c.t1, c.t2)


@pytest.mark.parametrize("kernel", ["tgemm", "gett"])
@pytest.mark.parametrize("n,na,nb,fock", T.SO_CASES)
def test_spin_orbital_triples_one_by_one(eng, n, na, nb, fock, kernel, monkeypatch):
    """Every i < j < k alone, the whole list and ragged parts: the closed-shell entry and Fock states with an f_ov of order one (the
    f_ov t2 term of the disconnected part), v odd and even, below two K steps (gather kernel whatever the knob) and above."""
    _knobs(monkeypatch, kernel)
    c = T.so_case(n, na, nb, fock)
    _load_so(eng, c)
    nt = len(c.val)
    assert eng.so_ntriples() == nt
    tol = T.tol_factor(c.o, c.v)
    worst = 0.0

    def run(a, b):
        nonlocal worst
        out = eng.do_ccsd_t_spinorb(a, b)
        ref, bound = float(np.sum(c.val[a:b])), tol * float(np.sum(c.S[a:b]))
        assert abs(out - ref) <= bound, (a, b, T.so_order(c.o)[a:b][:3], out, ref, abs(out - ref) / bound)
        worst = max(worst, abs(out - ref) / bound)
        return out, bound

    whole, bound = run(0, nt)
    ones = sum(run(t, t + 1)[0] for t in range(nt))
    assert abs(ones - whole) <= 2 * bound
    thirds = run(0, nt // 3)[0] + run(nt // 3, nt - 1)[0] + run(nt - 1, nt)[0]
    assert abs(thirds - whole) <= 2 * bound
    # new amplitudes under the cached operand copies and plan
    t1, t2 = T.random_so_amplitudes(c.o, c.v, 5)
    eng.so_set_amplitudes(t1, t2)
    val, S = T.so_per_triple(c.g, c.lev, c.o, t1, t2, c.f_ov)
    out = eng.do_ccsd_t_spinorb(0, nt)
    assert abs(out - float(np.sum(val))) <= tol * float(np.sum(S))
    print(f"largest error / bound (spin-orbital): {worst:.4f}")
