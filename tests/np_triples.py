"""The perturbative triples in plain numpy, one value set per triple: the reference of the (T) tests.  Test infrastructure only.

Spin-free (src/ccsd.f90:2152-2237, as the oracle reads it): for every ORDERED (i,j,k)
    W(abc)  = sum of the six permuted particle / hole terms                                   :2168-2173
    t3 = W / D,  z3 = [t1(i,a)<jk|bc> + t1(j,b)<ik|ac> + t1(k,c)<ij|ab>] / D                   :2175-2179
    y  = t1 t1 t1 + t1(i,a) t2(jk,bc) + t1(j,b) t2(ik,ac) + t1(k,c) t2(ij,ab)                  :2183-2184
    x_bar(abc) = 4/3 x(abc) - 2 x(acb) + 2/3 x(cab)                                            :2314-2318  (NOT symmetrised)
    E[T] = sum t_bar W,  E(T) - E[T] = sum z_bar W,  D[T] = sum t_bar y,  D(T) - D[T] = sum z_bar y,  and with the completely
    renormalised moment M3 (:2186-2194)  sum t_bar M3,  sum z_bar M3.
All of it in np.longdouble.  The engine visits i <= j <= k only, with a functional symmetrised over the six permutations and a weight 6/3/1;
that this equals the sum of the values above over the distinct ordered permutations of a sorted triple is what the tests check, so it is
not restated here.

Beside every value stands its majorant S: the same expression with |t1|, |t2|, |integral|, 1/|D| and the absolute bar weights
(4/3, 2, 2/3), i.e. the sum of the absolute values of all products that enter -- a bound of the forward error of every summation order.

Spin-orbital (src/ccsd.f90:1812-1922; whole-sum forms: np_ucc.UCC.triples, np_rocc.ROCC.triples): per i<j<k
    E = sum P(wc) (P(wc) + P(wd)) / D / 6,   P(x) = x(abc) - x(bac) - x(cba),
with and without the f_ov t2 term in the disconnected part wd.
"""
from __future__ import annotations

import collections
import functools
import itertools

import numpy as np

from afesp_amd.rhf import unpack_eri

LD = np.longdouble
EPS53 = 2.0 ** -53
NQ = 6   # E[T], E(T)-E[T], D[T], D(T)-D[T], sum t_bar M3, sum z_bar M3

# (o, v): between them nt8 = 1, 2, 3; v % 8 in {0, 1, 7, even non-zero}; v = 1; v + o <= 16 and > 16 (one K step of the LDS-DMA GEMM and more);
# the four ktail4 values; v even and odd; o = 1, 2, 3 and >= 5.  test_triples_cpu.py asserts that they do.
CASES = [(1, 1), (2, 7), (3, 9), (4, 13), (5, 16), (6, 17), (3, 18), (2, 24), (6, 24)]
# seeds (integrals, amplitudes) with which E[T] and E(T) of every triple stay above 1e-3 of their majorants, and the sums of independent
# sign a factor 1e3 above the tolerance (test_triples_cpu.py: test_no_reference_value_is_cancelled_away)
SEEDS = {c: (101 + 7 * n, 211 + 5 * n) for n, c in enumerate(CASES)}
SCALE = 1.0   # O(1) integrals: W, Z and Y of comparable size (the ladder energies keep |D| >= 6)

# one block triple of 8436 triples x one cube orbit: more than the 8192 partials the one-launch sum takes, and the two-stage sum_partials
LARGE_CASE = (36, 2)
SEEDS[LARGE_CASE] = (401, 402)
# spin-orbital cases (n spatial orbitals, n_alpha, n_beta, Fock state?): o_so = n_alpha + n_beta <= 6, v_so = 2 n - o_so even on the closed-shell
# entry and odd on the open-shell Fock states; ceil16(2 n) = 16 (gather kernel only) and 32 (LDS-DMA kernel); nt8 = 1, 2, 3
SO_CASES = [(5, 2, 2, False), (9, 3, 3, False), (6, 3, 2, True), (11, 3, 2, True)]


def tol_factor(o, v):
    """Per triple and quantity |engine - reference| <= tol_factor * S.  Every term of a sum is a product of two computed factors (t_bar or
    z_bar with W, y or M3), each a sum of up to K = v + o products (or a few) with K + a few roundings against its majorant: 2 K; the
    reduction tree over elements, lanes, waves and blocks, rcp_nr and the bars account for the 64.  Not tuned to any kernel."""
    return (2 * (v + o) + 64) * EPS53


def kc(o, v):
    return (v + o + 15) // 16 * 16


def facts(o, v):
    """What the planner and the kernels branch on (csrc/triples.hip, tgemm.h)."""
    K = kc(o, v)
    return dict(nt8=(v + 7) // 8, vmod8=v % 8, nk1=K // 16, ktail4=(v + o - (K - 16) + 3) // 4, c_pairs=v % 2 == 0,
                norb=((v + 7) // 8) * ((v + 7) // 8 + 1) * ((v + 7) // 8 + 2) // 6)


# ------------------------------------------------------------------------------------------------------------------ inputs
def slices(o, v, eri_packed):
    """v_vvov(a,b,i,c) = <ab|ic>, v_oovo(i,j,a,k) = <ij|ak>, v_oovv(i,j,a,b) = <ij|ab> with <pq|rs> = (pr|qs) (ccsd.f90:501)."""
    n = o + v
    chem = unpack_eri(n, eri_packed)
    phys = chem.transpose(0, 2, 1, 3)
    O, V = slice(0, o), slice(o, n)
    return phys[V, V, O, V].copy(), phys[O, O, V, O].copy(), phys[O, O, V, V].copy()


def random_amplitudes(o, v, seed):
    """t1 uniform in [-1, 1]; t2 with t2(i,j,a,b) = t2(j,i,b,a) and no other symmetry."""
    rng = np.random.default_rng(seed)
    t1 = rng.uniform(-1.0, 1.0, (o, v))
    a = rng.uniform(-1.0, 1.0, (o, o, v, v))
    return t1, 0.5 * (a + a.transpose(1, 0, 3, 2))


def random_so_amplitudes(o, v, seed):
    """antisymmetric in (i,j) and in (a,b)"""
    rng = np.random.default_rng(seed)
    t1 = rng.uniform(-1.0, 1.0, (o, v))
    a = rng.uniform(-1.0, 1.0, (o, o, v, v))
    a = a - a.transpose(1, 0, 2, 3)
    return t1, 0.5 * (a - a.transpose(0, 1, 3, 2))


# ------------------------------------------------------------------------------------------------------------- enumeration
def fused_order(o, sb):
    """The flat list of plan_fused: block triples I <= J <= K of sb occupied indices major, i <= j <= k inside."""
    nbk = (o + sb - 1) // sb
    out = []
    for I in range(nbk):
        for J in range(I, nbk):
            for K in range(J, nbk):
                for i in range(I * sb, min(o, (I + 1) * sb)):
                    for j in range(max(i, J * sb), min(o, (J + 1) * sb)):
                        for k in range(max(j, K * sb), min(o, (K + 1) * sb)):
                            out.append((i, j, k))
    return out


def block_triple_ranges(o, sb):
    """[(begin, end)) of every non-empty block triple in fused_order(o, sb)."""
    nbk = (o + sb - 1) // sb
    out, flat = [], 0
    for I in range(nbk):
        for J in range(I, nbk):
            for K in range(J, nbk):
                n = sum(1 for i in range(I * sb, min(o, (I + 1) * sb)) for j in range(max(i, J * sb), min(o, (J + 1) * sb))
                        for k in range(max(j, K * sb), min(o, (K + 1) * sb)))
                if n:
                    out.append((flat, flat + n))
                flat += n
    return out


def so_order(o):
    return list(itertools.combinations(range(o), 3))


# --------------------------------------------------------------------------------------------------------------- spin-free
def _bar(x, w2):
    """x_bar(abc) = 4/3 x(abc) - w2 x(acb) + 2/3 x(cab) over the last three axes (w2 = 2; -2 for the majorant)"""
    return LD(4) / LD(3) * x - w2 * x.swapaxes(-1, -2) + LD(2) / LD(3) * np.moveaxis(x, -3, -1)


def _blocks(t2, part, hole):
    """X[p,q,r,a,b,c] = sum_d t2(p,q,a,d) part(d,r,b,c) - sum_l t2(l,p,b,a) hole(l,r,q,c), and the sum of the absolute products"""
    res = []
    for sign, f in ((LD(-1), lambda z: z), (LD(1), np.abs)):
        p1 = np.tensordot(f(t2), f(part), axes=([3], [0]))                          # [p,q,a, r,b,c]
        p2 = np.tensordot(f(t2).transpose(1, 2, 3, 0), f(hole), axes=([3], [0]))    # [p,b,a, r,q,c]
        res.append(p1.transpose(0, 1, 3, 2, 4, 5) + sign * p2.transpose(0, 4, 3, 2, 1, 5))
    return res


def _w(X, i):
    """W^{ijk}(abc) = X^{ijk}(abc) + X^{jik}(bac) + X^{kji}(cba) + X^{ikj}(acb) + X^{jki}(bca) + X^{kij}(cab) for one i -> [j,k,a,b,c]"""
    return (X[i] + X[:, i].transpose(0, 1, 3, 2, 4) + X[:, :, i].transpose(1, 0, 4, 3, 2) + X[i].transpose(1, 0, 2, 4, 3)
            + X[:, :, i].transpose(0, 1, 4, 2, 3) + X[:, i].transpose(1, 0, 3, 4, 2))


def spin_free_ordered(e, t1, t2, vvov, oovo, oovv, ipp=None, ioo=None):
    """-> (val[o,o,o,NQ], S[o,o,o,NQ]) in np.longdouble, one row per ordered (i,j,k); the M3 columns are zero without ipp / ioo
    (I_vovv_pp(d,k,b,c), I_ooov_pp(j,k,l,a) as the oracle keeps them)."""
    o, v = t1.shape
    e, t1, t2, vvov, oovo, oovv = (np.asarray(x, dtype=LD) for x in (e, t1, t2, vvov, oovo, oovv))
    # term 1 of :2168: t2(i,j,a,d) <cb|kd> - t2(l,i,b,a) <kj|cl>
    X, Xa = _blocks(t2, vvov.transpose(3, 2, 1, 0), oovo.transpose(3, 0, 1, 2))
    cr = ipp is not None
    M = Ma = None
    if cr:
        ipp, ioo = np.asarray(ipp, dtype=LD), np.asarray(ioo, dtype=LD)
        # :2188-2193: t2(i,j,a,d) I_vovv_pp(d,k,b,c) - t2(l,i,b,a) I_ooov_pp(j,k,l,c)
        M, Ma = _blocks(t2, ipp, ioo.transpose(2, 1, 0, 3))
    eo, ev = e[:o], e[o:]
    dv = ev[:, None, None] + ev[None, :, None] + ev[None, None, :]
    val = np.zeros((o, o, o, NQ), dtype=LD)
    S = np.zeros((o, o, o, NQ), dtype=LD)
    ax = (-3, -2, -1)
    for i in range(o):
        D = (eo[i] + eo[:, None] + eo[None, :])[:, :, None, None, None] - dv[None, None]     # [j,k,a,b,c]
        for out, sgn, T1, T2, VV, XX, MM, rD in ((val, LD(1), t1, t2, oovv, X, M, 1 / D),
                                                 (S, LD(-1), np.abs(t1), np.abs(t2), np.abs(oovv), Xa, Ma, 1 / np.abs(D))):
            W = _w(XX, i)
            a = T1[i][None, None, :, None, None]          # t1(i,a)
            b = T1[:, None, None, :, None]                # t1(j,b)
            c = T1[None, :, None, None, :]                # t1(k,c)
            Z = (a * VV[:, :, None, :, :] + b * VV[i][None, :, :, None, :] + c * VV[i][:, None, :, :, None]) * rD
            Y = a * b * c + a * T2[:, :, None, :, :] + b * T2[i][None, :, :, None, :] + c * T2[i][:, None, :, :, None]
            tb, zb = _bar(W * rD, sgn * LD(2)), _bar(Z, sgn * LD(2))
            out[i, :, :, 0], out[i, :, :, 1] = np.sum(tb * W, axis=ax), np.sum(zb * W, axis=ax)
            out[i, :, :, 2], out[i, :, :, 3] = np.sum(tb * Y, axis=ax), np.sum(zb * Y, axis=ax)
            if cr:
                M3 = _w(MM, i)
                out[i, :, :, 4], out[i, :, :, 5] = np.sum(tb * M3, axis=ax), np.sum(zb * M3, axis=ax)
    return val, S


def sorted_sums(x):
    """x[o,o,o,...] per ordered triple -> {(i<=j<=k): sum over the distinct ordered permutations}"""
    o = x.shape[0]
    return {t: sum(x[p] for p in sorted(set(itertools.permutations(t)))) for t in itertools.combinations_with_replacement(range(o), 3)}


def base_term(t1, t2):
    """1 + 2 sum t1^2 + sum (2 t2(ijab) - t2(jiab)) (t2(ijab) + t1(ia) t1(jb))  (:2243) -> (value, majorant)"""
    t1, t2 = np.asarray(t1, dtype=LD), np.asarray(t2, dtype=LD)
    tau = t2 + t1[:, None, :, None] * t1[None, :, None, :]
    val = 1 + 2 * np.sum(t1 * t1) + np.sum((2 * t2 - t2.transpose(1, 0, 2, 3)) * tau)
    a1, a2 = np.abs(t1), np.abs(t2)
    maj = 1 + 2 * np.sum(a1 * a1) + np.sum((2 * a2 + a2.transpose(1, 0, 2, 3)) * (a2 + a1[:, None, :, None] * a1[None, :, None, :]))
    return val, maj


def reported(val):
    """The engine's six outputs from the six sums: E[T], E(T), D[T], D(T), sum t_bar M3, sum (t_bar + z_bar) M3 (the majorants add the
    same way)."""
    v = np.asarray(val)
    return np.stack([v[..., 0], v[..., 0] + v[..., 1], v[..., 2], v[..., 2] + v[..., 3], v[..., 4], v[..., 4] + v[..., 5]], axis=-1)


# ------------------------------------------------------------------------------------------------------------ spin-orbital
def so_g(chem, orb, spin):
    """<pq||rs> over the spin orbitals (orb[x], spin[x]) from one full chemist array (pq|rs) of the spatial orbitals"""
    orb, spin = np.asarray(orb), np.asarray(spin)
    c = chem[np.ix_(orb, orb, orb, orb)] * (spin[:, None, None, None] == spin[None, :, None, None]) * \
        (spin[None, None, :, None] == spin[None, None, None, :])
    phys = c.transpose(0, 2, 1, 3)
    return phys - phys.transpose(0, 1, 3, 2)


def interleaved_order(n, nel):
    """init_cc_spinorb: spin orbital x of the occupied / virtual list is spatial orbital x / 2 with spin x % 2 (ccsd.f90:451-454)"""
    x = np.concatenate([np.arange(nel), nel + np.arange(2 * n - nel)])
    return x // 2, x % 2


def so_per_triple(g, lev, o, t1, t2, f_ov=None):
    """-> (val[nt], S[nt]) over so_order(o), np.longdouble"""
    g, lev, t1, t2 = (np.asarray(x, dtype=LD) for x in (g, lev, t1, t2))
    O, V = slice(0, o), slice(o, None)
    vovv, ovoo, vvoo = g[V, O, V, V], g[O, V, O, O], g[V, V, O, O]
    fo = None if f_ov is None else np.asarray(f_ov, dtype=LD)
    eo, ev = lev[:o], lev[o:]
    dv = ev[:, None, None] + ev[None, :, None] + ev[None, None, :]
    vals, majs = [], []
    for i, j, k in so_order(o):
        d = eo[i] + eo[j] + eo[k] - dv
        res = []
        for s, f in ((LD(1), lambda z: z), (LD(-1), np.abs)):
            def pp(p, q, r):    # sum_f <fp||bc> t2(q,r,a,f)
                return np.einsum("fbc,af->abc", f(vovv[:, p]), f(t2[q, r]))

            def hh(p, q, r):    # sum_m t2(m,p,c,b) <ma||qr>
                return np.einsum("mcb,ma->abc", f(t2[:, p]), f(ovoo[:, :, q, r]))

            def P(x):
                return x - s * x.transpose(1, 0, 2) - s * x.transpose(2, 1, 0)
            # value: s = 1; majorant: s = -1 turns every minus sign into a plus
            wc = pp(i, j, k) - s * pp(j, i, k) - s * pp(k, j, i) - s * hh(i, j, k) + hh(j, i, k) + hh(k, j, i)
            wd = (f(t1[i])[:, None, None] * f(vvoo[:, :, j, k])[None] - s * f(t1[j])[:, None, None] * f(vvoo[:, :, i, k])[None]
                  - s * f(t1[k])[:, None, None] * f(vvoo[:, :, j, i])[None])
            if fo is not None:
                wd = wd + (f(fo[i])[:, None, None] * f(t2[j, k])[None] - s * f(fo[j])[:, None, None] * f(t2[i, k])[None]
                           - s * f(fo[k])[:, None, None] * f(t2[j, i])[None])
            c = P(wc)
            res.append(np.sum(c * (c + P(wd)) / f(d)) / 6)
        vals.append(res[0])
        majs.append(res[1])
    return np.array(vals, dtype=LD), np.array(majs, dtype=LD)


# ------------------------------------------------------------------------------------------------------------------- cases
Case = collections.namedtuple("Case", "o v e eri t1 t2 ipp ioo val S base")
# val, S: {(i<=j<=k): the six reported quantities (reported()) of the sorted triple and their majorants}, np.longdouble, without the base term
# base:   (value, majorant) of the base term of D[T] and D(T)


@functools.lru_cache(maxsize=None)
def case(o, v, which=0):
    """The inputs and the per-triple reference of one (o, v) of CASES; which = 1: a second, independent set of amplitudes.  The completely
    renormalised intermediates are the oracle's, from the same amplitudes (I_vo and asym_t2 of an update_intermediates on them)."""
    import molecules
    import orc
    s_int, s_amp = SEEDS[(o, v)]
    n, e, eri = molecules.synthetic_system(o, v, scale=SCALE, seed=s_int)
    t1, t2 = random_amplitudes(o, v, s_amp + 1000 * which)
    vvov, oovo, oovv = slices(o, v, eri)
    cc = orc.OracleCC(o, v, eri, e, 2)
    cc.t1[...] = t1
    cc.t2[...] = t2
    cc.L.orc_cc_intermediates(cc.h)
    ipp, ioo = (x.copy() for x in cc.cr_intermediates())
    cc.close()
    val, S = spin_free_ordered(e, t1, t2, vvov, oovo, oovv, ipp, ioo)
    return Case(o, v, e, eri, t1, t2, ipp, ioo, sorted_sums(reported(val)), sorted_sums(reported(S)), base_term(t1, t2))


def expected(c, triples, with_base):
    """Sum of the reference over a list of sorted triples -> (value[6], bound[6]) as float64: the bound is tol_factor x the summed majorants."""
    val = sum((c.val[t] for t in triples), np.zeros(NQ, dtype=LD))
    S = sum((c.S[t] for t in triples), np.zeros(NQ, dtype=LD))
    if with_base:
        val[2:4] += c.base[0]
        S[2:4] += c.base[1]
    return val.astype(np.float64), (tol_factor(c.o, c.v) * S).astype(np.float64)


SOCase = collections.namedtuple("SOCase", "n na nb fock o v e eri fa fb g lev f_ov t1 t2 val S")


@functools.lru_cache(maxsize=None)
def so_case(n, na, nb, fock):
    """Closed-shell entry (init_cc_spinorb, interleaved spins, na == nb) or a Fock state (uso_init_fock on identity rotations: occupied
    alpha, occupied beta, virtual alpha, virtual beta) with diagonal oo / vv blocks and a random f_ov of order one."""
    import molecules
    import np_ucc
    o, v = na + nb, 2 * n - na - nb
    _, e, eri = molecules.synthetic_system(na, n - na, scale=SCALE, seed=601 + 10 * n + o)
    chem = unpack_eri(n, eri)
    rng = np.random.default_rng(701 + 10 * n + o)
    fa = fb = f_ov = None
    if fock:
        orb, spin = np_ucc.so_order(n, na, nb)
        eb = e.copy()
        eb[nb:na] = 0.5 + 0.125 * np.arange(na - nb)     # virtual for beta: above every occupied level
        fa, fb = np.diag(e), np.diag(eb)
        for f, no in ((fa, na), (fb, nb)):
            f[:no, no:] = rng.uniform(-0.5, 0.5, (no, n - no))
            f[no:, :no] = f[:no, no:].T
        f_so = np.where(spin[:, None] == spin[None, :], np.where(spin[:, None] == 0, fa[np.ix_(orb, orb)], fb[np.ix_(orb, orb)]), 0.0)
        f_ov = f_so[:o, o:].copy()
    else:
        assert na == nb
        orb, spin = interleaved_order(n, o)
    lev = e[orb] if not fock else np.where(spin == 0, e[orb], eb[orb])
    g = so_g(chem, orb, spin)
    t1, t2 = random_so_amplitudes(o, v, 801 + 10 * n + o)
    val, S = so_per_triple(g, lev, o, t1, t2, f_ov)
    return SOCase(n, na, nb, fock, o, v, e, eri, fa, fb, g, lev, f_ov, t1, t2, val, S)
