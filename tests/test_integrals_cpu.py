"""The reference of the integral-layer tests (np_integrals.py) held to its own bound, without a GPU: float64 against longdouble within
1 x the bound test_gpu_integrals.py holds the engine to, against np_ucc's einsum restatement, and hashed_mp2 against the explicitly
built and transformed tensor."""
import numpy as np
import pytest

import np_integrals as I
import np_ucc

LD = np.longdouble
SIZES = [3, 17, 33]      # (longdouble at n = 33 takes half a second and grows as n^5: nothing above it)


def _inputs(n, seed=0):
    rng = np.random.default_rng(1000 + 17 * n + seed)
    eri = rng.standard_normal(I.neri(n))
    Ca, Cb = rng.standard_normal((n, n)), rng.standard_normal((n, n))       # general, not orthogonal
    H = rng.standard_normal((n, n))
    H = H + H.T
    Da, Db = rng.standard_normal((n, n)), rng.standard_normal((n, n))       # Da non-symmetric
    Db = Db + Db.T
    return eri, Ca, Cb, H, Da, Db


@pytest.mark.parametrize("n", SIZES)
def test_float64_transform_is_within_the_bound_of_the_longdouble_one(n):
    eri, Ca, Cb, *_ = _inputs(n)
    V = I.unpack(n, eri)
    lo, hi, major = I.mo_blocks(n, Ca, Cb, V, np.float64), I.mo_blocks(n, Ca, Cb, V, LD), I.mo_majorant(n, Ca, Cb, V)
    worst = 0.0
    for a, b, m in zip(lo, hi, major):
        assert a.dtype == np.float64 and b.dtype == LD
        ratio = float(np.max(np.abs(a - b) / (I.xform_factor(n) * m)))
        worst = max(worst, ratio)
    print(f"n = {n}: transform, float64 against longdouble, largest error / bound {worst:.4f}")
    assert worst <= 1.0
    assert np.max(np.abs(hi[0] - hi[0].transpose(2, 3, 0, 1))) <= float(I.xform_factor(n) * np.max(major[0]))


@pytest.mark.parametrize("n", SIZES)
def test_float64_fock_builds_are_within_the_bound_of_the_longdouble_ones(n):
    eri, _, _, H, Da, Db = _inputs(n)
    V = I.unpack(n, eri)
    worst = 0.0
    for D in (Da, Db):                                                       # non-symmetric and symmetric
        lo, hi, m = I.fock_rhf(n, H, V, D, np.float64), I.fock_rhf(n, H, V, D, LD), I.fock_majorant(n, H, V, D)
        assert lo.dtype == np.float64 and hi.dtype == LD
        worst = max(worst, float(np.max(np.abs(lo - hi) / (I.fock_factor(n) * m))))
    lo, hi, m = I.fock_uhf(n, H, V, Da, Db, np.float64), I.fock_uhf(n, H, V, Da, Db, LD), I.fock_majorant(n, H, V, Da, Db)
    for s in range(2):
        worst = max(worst, float(np.max(np.abs(lo[s] - hi[s]) / (I.fock_factor(n) * m[s]))))
    print(f"n = {n}: Fock builds, float64 against longdouble, largest error / bound {worst:.4f}")
    assert worst <= 1.0
    # the defining sums, element by element, for one element of each
    i, j = n - 1, 0
    ref = H[i, j] + sum(Da[k, l] * (2.0 * V[i, j, k, l] - V[i, k, j, l]) for k in range(n) for l in range(n))
    assert abs(I.fock_rhf(n, H, V, Da)[i, j] - ref) <= I.fock_factor(n) * I.fock_majorant(n, H, V, Da)[i, j]
    refb = H[i, j] + sum((Da[k, l] + Db[k, l]) * V[i, j, k, l] - Db[k, l] * V[i, k, j, l] for k in range(n) for l in range(n))
    assert abs(lo[1][i, j] - refb) <= I.fock_factor(n) * m[1][i, j]
    same = I.fock_uhf(n, H, V, Da, Da)
    assert np.max(np.abs(same[0] - I.fock_rhf(n, H, V, Da))) <= float(np.max(I.fock_factor(n) * I.fock_majorant(n, H, V, Da)))


def test_transform_equals_the_einsum_restatement():
    n = 7
    eri, Ca, Cb, *_ = _inputs(n)
    ours, theirs = I.mo_blocks(n, Ca, Cb, eri), np_ucc.mo_blocks(n, Ca, Cb, eri)
    assert np.array_equal(I.unpack(n, eri), np_ucc.unpack_eri(n, eri))
    for a, b in zip(ours, theirs):
        assert np.max(np.abs(a - b)) < 1e-13 * np.max(np.abs(b))
    V = I.unpack(n, eri)                                                      # (symmetric to the bit in both pairs)
    assert np.array_equal(I.unpair_matrix(n, np_ucc.pair_matrix(V)), V)
    ea, eb = np.sort(np.random.default_rng(5).uniform(-2, 2, n)), np.sort(np.random.default_rng(6).uniform(-2, 2, n))
    ea[3:] += 3.0
    eb[2:] += 3.0
    e2, major = I.ump2(*ours, ea, eb, 3, 2)
    ref = np_ucc.ump2(*theirs, ea, eb, 3, 2)
    assert abs(e2 - ref) < 1e-13 * major and abs(ref) > 1e-3 * major
    assert I.ump2(*ours, ea, eb, n, 0) == (0.0, 0.0)                          # no virtual orbital, no occupied one: every list empty


def test_hashed_mp2_equals_mp2_of_the_built_and_transformed_tensor():
    n, o, scale, seed = 9, 3, 0.3, 4242
    rng = np.random.default_rng(17)
    perm, sign = rng.permutation(n), rng.choice([-1.0, 1.0], n)
    c = np.zeros((n, n))
    c[np.arange(n), perm] = sign
    e = np.concatenate([-2.0 + np.arange(o) / (o - 1), 1.0 + 2.0 * np.arange(n - o) / (n - o - 1)])
    ao = scale * (2.0 * I._hash_uniform(np.arange(I.neri(n)).astype(np.uint64), seed) - 1.0)
    mo = I.mo_blocks(n, c, c, ao, LD)[0]
    ref, ref_major = I.mp2(mo, e, o, LD)
    got, major = I.hashed_mp2(n, o, perm, sign, e, scale, seed)
    assert abs(got - float(ref)) <= 4 * I.EPS53 * major                       # (both exact term by term: the two sums' own roundings)
    assert abs(major - ref_major) <= 1e-14 * major and abs(got) > 0.01 * major
    # the plain loop over the terms
    V = I.unpack(n, ao)
    P, loop = perm, 0.0
    for i in range(o):
        for j in range(o):
            for a in range(o, n):
                for b in range(o, n):
                    x = sign[i] * sign[a] * sign[j] * sign[b] * V[P[i], P[a], P[j], P[b]]
                    xt = sign[i] * sign[a] * sign[j] * sign[b] * V[P[i], P[b], P[j], P[a]]
                    loop += x * (2.0 * x - xt) / (e[i] + e[j] - e[a] - e[b])
    assert abs(got - loop) <= (o * o * (n - o) ** 2 + 4) * I.EPS53 * major
