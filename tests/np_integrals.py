"""The integral layer in plain numpy: the reference of test_integrals_cpu.py and test_gpu_integrals.py.  Test infrastructure only.

Every function takes `dtype` (np.float64 or np.longdouble) and carries all of its arithmetic in it.
    unpack        packed (8-fold, integrals.f90:196-210) -> (n,n,n,n), chemist order (ij|kl)
    mo_blocks     (aa|aa), (aa|bb), (bb|bb) by four quarter transforms (mp2.f90:321-385), C as (MO, AO)
    fock_rhf      F = H + sum_kl D(k,l) [2 (ij|kl) - (ik|jl)]                                   (hf.f90:349-385)
    fock_uhf      F_s = H + J[Da + Db] - K[D_s]
    mp2, ump2     the energies from the blocks and the levels                                  (mp2.f90:418-440)
    hashed_mp2    E(MP2) of afesp_synthetic_ao integrals under a signed-permutation coefficient matrix, from the hash alone

Beside every value stands its majorant: the same expression on the absolute values of its inputs, i.e. the sum of the absolute values of
all products that enter.  Bounds (for any summation order, with or without FMA): a sum of K products has |error| <= (K + c) 2^-53 majorant;
    an MO integral is four nested dot products of length n: K = 4 n;   a Fock element is one dot product of length n^2: K = n^2;
c = 64 is the slack np_triples.tol_factor uses (reduction trees, the final additions, the factors 2).
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
EPS53 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------------ bounds
def xform_factor(n):
    """|engine - reference| <= xform_factor(n) * majorant for every MO integral"""
    return (4 * n + 64) * EPS53


def fock_factor(n):
    """|engine - reference| <= fock_factor(n) * majorant for every Fock element"""
    return (n * n + 64) * EPS53


def scalar_bound(ref):
    """the project's rule for the energies of these entry points (test_ao2mo_pair_symmetric_transform)"""
    return 1e-10 * max(1.0, abs(float(ref)))


# ------------------------------------------------------------------------------------------------------------------ the packed array
def _hash_uniform(k, seed):
    """numpy twin of the device generator (csrc/capi.hip, splitmix64) used by afesp_synthetic_ao / afesp_synthetic_init"""
    with np.errstate(over="ignore"):
        x = (k.astype(np.uint64) + np.uint64(seed)) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) / 9007199254740992.0


def _tri(i, j):
    hi, lo = np.maximum(i, j), np.minimum(i, j)
    return hi * (hi + 1) // 2 + lo


def _packed(i, j, k, l):
    return _tri(_tri(i, j), _tri(k, l))          # integrals.f90:196-210, 0-based


def neri(n):
    npair = n * (n + 1) // 2
    return npair * (npair + 1) // 2


def unpack(n, eri):
    """packed -> (n,n,n,n)"""
    idx = np.arange(n)
    pair = _tri(idx[:, None], idx[None, :])
    return np.asarray(eri)[_tri(pair[:, :, None, None], pair[None, None, :, :])]


def unpair_matrix(n, ab):
    """[npair, npair] (the engine's alpha-beta layout, ab[tri(p,q), tri(r,s)] = (pq|rs)) -> (n,n,n,n)"""
    idx = np.arange(n)
    pair = _tri(idx[:, None], idx[None, :])
    return np.asarray(ab)[pair[:, :, None, None], pair[None, None, :, :]]


# ------------------------------------------------------------------------------------------------------------------ the transform
def _quarter(C, T):
    """contracts the leading index of T with C(MO, AO) and appends the new index: four of them bring the order back to (p,q,r,s)"""
    return np.tensordot(T, C, axes=([0], [1]))


def mo_blocks(n, Ca, Cb, V, dtype=np.float64):
    """(aa|aa), (aa|bb), (bb|bb) as (n,n,n,n) arrays from the AO integrals V (n,n,n,n, or packed), by four quarter transforms"""
    V = np.asarray(V)
    if V.ndim == 1:
        V = unpack(n, V)
    V, Ca, Cb = V.astype(dtype), np.asarray(Ca).astype(dtype), np.asarray(Cb).astype(dtype)
    ha = _quarter(Ca, _quarter(Ca, V))           # (k,l,p,q), pq alpha
    hb = _quarter(Cb, _quarter(Cb, V))
    aa = _quarter(Ca, _quarter(Ca, ha))
    ab = _quarter(Cb, _quarter(Cb, ha))          # (p,q,r,s): pq alpha, rs beta
    bb = _quarter(Cb, _quarter(Cb, hb))
    return aa, ab, bb


def mo_majorant(n, Ca, Cb, V):
    """the same transform of |C| and |V|"""
    V = np.asarray(V)
    if V.ndim == 1:
        V = unpack(n, V)
    return mo_blocks(n, np.abs(Ca), np.abs(Cb), np.abs(V), np.float64)


# ------------------------------------------------------------------------------------------------------------------ the Fock builds
def _jk(n, V, D, dtype):
    V, D = np.asarray(V).astype(dtype), np.asarray(D).astype(dtype)
    d = D.reshape(n * n)
    J = (V.reshape(n * n, n * n) @ d).reshape(n, n)                            # sum_kl (ij|kl) D(k,l)
    K = (V.transpose(0, 2, 1, 3).reshape(n * n, n * n) @ d).reshape(n, n)      # sum_kl (ik|jl) D(k,l)
    return J, K


def fock_rhf(n, H, V, D, dtype=np.float64):
    J, K = _jk(n, V, D, dtype)
    return np.asarray(H).astype(dtype) + (dtype(2) * J - K)


def fock_uhf(n, H, V, Da, Db, dtype=np.float64):
    Da, Db = np.asarray(Da).astype(dtype), np.asarray(Db).astype(dtype)
    J, Ka = _jk(n, V, Da + Db, dtype)[0], _jk(n, V, Da, dtype)[1]
    Kb = _jk(n, V, Db, dtype)[1]
    H = np.asarray(H).astype(dtype)
    return H + (J - Ka), H + (J - Kb)


def fock_majorant(n, H, V, Da, Db=None):
    """|H| + the same sums of absolute values: weights 2 and 1 on the J and K terms (RHF: Db None), 1 and 1 (UHF: a pair)"""
    aV, aH = np.abs(V), np.abs(H)
    if Db is None:
        J, K = _jk(n, aV, np.abs(Da), np.float64)
        return aH + 2.0 * J + K
    J = _jk(n, aV, np.abs(Da) + np.abs(Db), np.float64)[0]
    return aH + J + _jk(n, aV, np.abs(Da), np.float64)[1], aH + J + _jk(n, aV, np.abs(Db), np.float64)[1]


# ------------------------------------------------------------------------------------------------------------------ the energies
def _den(eo1, ev1, eo2, ev2):
    return eo1[:, None, None, None] - ev1[None, :, None, None] + eo2[None, None, :, None] - ev2[None, None, None, :]


def mp2(mo, e, o, dtype=np.float64):
    """-> (E(MP2), majorant) from the MO integrals (n,n,n,n) and the n levels: sum (ia|jb) [2 (ia|jb) - (ib|ja)] / D"""
    x = np.asarray(mo)[:o, o:, :o, o:].astype(dtype)
    e = np.asarray(e).astype(dtype)
    d = _den(e[:o], e[o:], e[:o], e[o:])
    xt = x.transpose(0, 3, 2, 1)
    return (x * (dtype(2) * x - xt) / d).sum(dtype=dtype), float((np.abs(x) * (2 * np.abs(x) + np.abs(xt)) / np.abs(d)).sum())


def ump2(aa, ab, bb, ea, eb, na, nb, dtype=np.float64):
    """-> (E(UMP2), majorant): 1/4 sum [(ia|jb) - (ib|ja)]^2 / D per spin + sum (ia|JB)^2 / D; an empty list contributes exactly 0"""
    ea, eb = np.asarray(ea).astype(dtype), np.asarray(eb).astype(dtype)

    def same(g, e, o):
        x = np.asarray(g)[:o, o:, :o, o:].astype(dtype)
        d = _den(e[:o], e[o:], e[:o], e[o:])
        a, m = x - x.transpose(0, 3, 2, 1), np.abs(x) + np.abs(x.transpose(0, 3, 2, 1))
        return (dtype(0.25) * a * a / d).sum(dtype=dtype), float((0.25 * m * m / np.abs(d)).sum())
    x = np.asarray(ab)[:na, na:, :nb, nb:].astype(dtype)
    d = _den(ea[:na], ea[na:], eb[:nb], eb[nb:])
    parts = [same(aa, ea, na), same(bb, eb, nb), ((x * x / d).sum(dtype=dtype), float((x * x / np.abs(d)).sum()))]
    return sum((p[0] for p in parts), dtype(0)), sum(p[1] for p in parts)


def hashed_mp2(n, o, perm, sign, e, scale, seed):
    """E(MP2) and its majorant for afesp_synthetic_ao(n, scale, seed) integrals under the coefficient matrix C(p, perm[p]) = sign[p]:
    (ia|jb) = s_i s_a s_j s_b AO[packed(P(i),P(a),P(j),P(b))], one hashed number each -- evaluated from the hash alone (no tensor is built
    or transformed); the o^2 v^2 terms in float64, their sum in longdouble"""
    perm, sign, e = np.asarray(perm), np.asarray(sign, dtype=np.float64), np.asarray(e, dtype=np.float64)
    i, a = np.arange(o), np.arange(o, n)
    I, A, J, B = perm[i][:, None, None, None], perm[a][None, :, None, None], perm[i][None, None, :, None], perm[a][None, None, None, :]
    s = sign[i][:, None, None, None] * sign[a][None, :, None, None] * sign[i][None, None, :, None] * sign[a][None, None, None, :]
    x = s * (scale * (2.0 * _hash_uniform(_packed(I, A, J, B).astype(np.uint64), seed) - 1.0))
    xt = x.transpose(0, 3, 2, 1)                  # (ib|ja)
    d = _den(e[:o], e[o:], e[:o], e[o:])
    energy = float((x * (2.0 * x - xt) / d).sum(dtype=LD))
    return energy, float((np.abs(x) * (2.0 * np.abs(x) + np.abs(xt)) / np.abs(d)).sum(dtype=LD))
