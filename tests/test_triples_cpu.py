"""np_triples.py, the per-triple reference of the (T) tests, pinned to the oracle; the enumeration; what the case table covers.  No GPU."""
import itertools

import numpy as np
import pytest

import np_rocc
import np_triples as T
import np_ucc
import orc

_f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel(order="F"))


@pytest.mark.parametrize("o,v", [(2, 7), (3, 9), (4, 13)])
def test_reference_equals_the_oracle_on_every_ordered_triple(o, v):
    """orc_ccsd_t_cr on [t, t+1) for every ordered (i,j,k) = t of o^3: all six sums.  The oracle works in binary64 with dot products of
    length v and o, so it carries the same forward-error bound as the engine (np_triples.tol_factor x the majorant)."""
    c = T.case(o, v)
    vvov, oovo, oovv = T.slices(o, v, c.eri)
    val, S = T.spin_free_ordered(c.e, c.t1, c.t2, vvov, oovo, oovv, c.ipp, c.ioo)
    L = orc.lib()
    args = (o, v, np.ascontiguousarray(c.e), _f(c.t1), _f(c.t2), _f(vvov), _f(oovo), _f(oovv))
    total, worst = np.zeros(6), 0.0
    for t, (i, j, k) in enumerate(itertools.product(range(o), repeat=3)):
        out = np.zeros(6)
        L.orc_ccsd_t_cr(*args, _f(c.ipp), _f(c.ioo), t, t + 1, out)
        plain = np.zeros(4)
        L.orc_ccsd_t(*args, t, t + 1, plain)
        assert np.array_equal(plain, out[:4])
        ref, maj = T.reported(val[i, j, k]), T.reported(S[i, j, k])
        if t == 0:   # the caller that holds t_begin == 0 adds the base term
            ref[2:4] += c.base[0]
            maj[2:4] += c.base[1]
        err = np.abs(out - ref.astype(np.float64))
        bound = (T.tol_factor(o, v) * maj).astype(np.float64)
        assert np.all(err <= bound), (i, j, k, err / bound)
        worst = max(worst, float(np.max(err / bound)))
        total += out
    print("largest error / bound of the oracle:", worst)
    # the sorted-triple sums (what the engine's i <= j <= k list is compared with) add up to the oracle's total
    whole = np.zeros(6)
    L.orc_ccsd_t_cr(*args, _f(c.ipp), _f(c.ioo), 0, o ** 3, whole)
    ref, bound = T.expected(c, list(c.val), True)
    assert np.all(np.abs(whole - ref) <= bound)
    assert np.all(np.abs(total - ref) <= bound)


def test_symmetric_amplitudes_only_as_far_as_the_derivation_needs():
    t1, t2 = T.random_amplitudes(3, 5, 1)
    assert np.array_equal(t2, t2.transpose(1, 0, 3, 2))
    assert np.max(np.abs(t2 - t2.transpose(1, 0, 2, 3))) > 0.1 and np.max(np.abs(t2 - t2.transpose(0, 1, 3, 2))) > 0.1
    assert np.max(np.abs(t1)) <= 1.0
    s1, s2 = T.random_so_amplitudes(4, 6, 1)
    assert np.array_equal(s2, -s2.transpose(1, 0, 2, 3)) and np.array_equal(s2, -s2.transpose(0, 1, 3, 2))


@pytest.mark.parametrize("o", [1, 2, 3, 5, 6, 7])
def test_fused_order_lists_every_sorted_triple_once(o):
    every = sorted(itertools.combinations_with_replacement(range(o), 3))
    for sb in range(1, o + 2):
        order = T.fused_order(o, sb)
        assert sorted(order) == every
        ranges = T.block_triple_ranges(o, sb)
        assert ranges[0][0] == 0 and ranges[-1][1] == len(order) and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        for b, e in ranges:   # one block triple: the blocks of i, j, k do not change inside
            assert len({(i // sb, j // sb, k // sb) for i, j, k in order[b:e]}) == 1
        nbk = (o + sb - 1) // sb
        assert len(ranges) == nbk * (nbk + 1) * (nbk + 2) // 6
    # blocks of one index and one block of all: the plain lexicographic list; anything between: another order (o >= 3)
    assert T.fused_order(o, 1) == every and T.fused_order(o, o) == every
    if o >= 3:
        assert T.fused_order(o, 2) != every
    assert T.so_order(o) == sorted(t for t in every if t[0] < t[1] < t[2])


def test_case_table_covers_what_it_claims():
    F = [dict(T.facts(o, v), o=o, v=v) for o, v in T.CASES]
    assert all(f["v"] <= 24 and f["o"] <= 6 for f in F)
    assert {f["nt8"] for f in F} == {1, 2, 3}
    assert {f["norb"] for f in F} == {1, 4, 10}                    # 10: the first all-distinct tile orbit A < B < C (v >= 17)
    mod = {f["vmod8"] for f in F}
    assert {0, 1, 7} <= mod and any(m % 2 == 0 and m for m in mod)
    assert any(f["v"] == 1 for f in F)
    assert {f["nk1"] == 1 for f in F} == {True, False}             # v + o <= 16: one K step, no half-length coinciding-pair groups on tgemm
    assert {f["ktail4"] for f in F} == {1, 2, 3, 4}
    assert {f["c_pairs"] for f in F} == {True, False}
    assert {1, 2, 3} <= {f["o"] for f in F} and any(f["o"] >= 5 for f in F)
    assert any(f["o"] % 2 for f in F if f["o"] >= 3)               # AFESP_T_BLOCK=2 leaves a ragged last block
    o, v = T.LARGE_CASE
    assert T.facts(o, v)["norb"] * (o * (o + 1) * (o + 2) // 6 - 1) > 8192
    S = [(2 * n - na - nb, na + nb, fock) for n, na, nb, fock in T.SO_CASES]
    assert {v % 2 for v, o, _ in S} == {0, 1} and all(3 <= o <= 6 for _, o, _ in S)
    assert {T.kc(o, v) < 32 for v, o, _ in S} == {True, False}     # below two K steps the spin-orbital plan stays on the gather kernel
    assert {(v + 7) // 8 for v, o, _ in S} == {1, 2, 3} and {f for _, _, f in S} == {True, False}


@pytest.mark.parametrize("o,v", T.CASES + [T.LARGE_CASE])
def test_no_reference_value_is_cancelled_away(o, v):
    """The tolerance of the GPU test is about 1.5e-14 S (S: the majorant).  A value far below its S would make it a test of nothing.

    E[T] and E(T): |value| >= 1e-3 S on every triple of every case with the seeds of np_triples.SEEDS (smallest: 1.6e-3 at (6, 24); E[T] is
    a definite form, what cancels is W itself, |W| / sum |products| ~ 1 / sqrt(6 (v + o))).
    D[T], D(T) and the two M3 sums are sums of v^3 products of independent sign, so |value| / S is of the order of
    |W| / sum|products| / sqrt(v^3): its MEDIAN over the triples is 1e-4 .. 7e-4 at v >= 13 whatever the seed (measured: (6,17) 6.6e-4, 7.2e-4,
    1.0e-4, 1.0e-4; (6,24) 3.0e-4, 3.0e-4, 7.3e-5, 6.3e-5), so 1e-3 S cannot be asked of them.  What is asked instead is what `vacuous`
    means: the tolerance is at most 1e-3 of the value, |value| >= 1e3 tol_factor S (smallest measured |value| / S: 2e-7, tol_factor: 1.5e-14).
    Two kinds of triples are zero by construction and are excepted: i = j = k (W is then symmetric in (abc) and the weights of x_bar add up to
    zero) and everything at v = 1 (the same, for every triple)."""
    c = T.case(o, v)
    for t in c.val:
        r = (np.abs(c.val[t]) / c.S[t]).astype(np.float64)
        if v == 1 or t[0] == t[2]:
            assert np.all(r < 1e-15), (t, r)
            continue
        if (o, v) != T.LARGE_CASE:   # (outside the table: used as ranges of thousands of triples, 1400 of its 8436 E(T) are below 1e-3 S)
            assert np.all(r[:2] >= 1e-3), (t, r)
        assert np.all(r >= 1e3 * T.tol_factor(o, v)), (t, r)


@pytest.mark.parametrize("n,na,nb,fock", T.SO_CASES)
def test_spin_orbital_reference(n, na, nb, fock):
    """The per-triple sums add up to the whole-sum forms: the oracle's (closed-shell entry; also pins the interleaved spin-orbital order) and
    np_rocc.ROCC.triples (Fock states; also pins the block order)."""
    c = T.so_case(n, na, nb, fock)
    total, S = float(np.sum(c.val)), float(np.sum(c.S))
    assert len(c.val) == len(T.so_order(c.o)) and np.all(np.abs(c.val) >= 1e-3 * c.S)
    if fock:
        chem = np_ucc.unpack_eri(n, c.eri)
        g, lev, o = np_ucc.so_integrals(chem, chem, chem, np.diag(c.fa).copy(), np.diag(c.fb).copy(), na, nb)
        assert o == c.o and np.array_equal(g, c.g) and np.array_equal(lev, c.lev)
        cc = np_rocc.ROCC(g, np_rocc.so_fock(c.fa, c.fb, na, nb), o)
        assert np.array_equal(cc.f_ov, c.f_ov) and np.max(np.abs(c.f_ov)) > 0.1
        assert not np.any(cc.f_oo) and not np.any(cc.f_vv)
        cc.t1, cc.t2 = c.t1, c.t2
        assert abs(cc.triples() - total) <= T.tol_factor(c.o, c.v) * S
        # ... and the f_ov term is far above the tolerance on every triple
        plain, _ = T.so_per_triple(c.g, c.lev, c.o, c.t1, c.t2, None)
        assert np.all(np.abs(plain - c.val) > 1e6 * T.tol_factor(c.o, c.v) * c.S)
    else:
        so = orc.OracleSO(n, na + nb, c.eri, c.e, 2)
        assert np.array_equal(so.field("oovv"), c.g[:c.o, :c.o, c.o:, c.o:])
        so.t1[...] = c.t1
        so.t2[...] = c.t2
        assert abs(so.triples() - total) <= T.tol_factor(c.o, c.v) * S
        so.close()
