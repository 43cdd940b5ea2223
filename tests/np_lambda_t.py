"""Lambda-CCSD(T) in plain numpy, one value per triple: the reference of the Lambda-(T) tests.  Test infrastructure only.

Conventions of np_triples.so_per_triple.  For i<j<k and x in {t, l}:
    pp_x(p;q,r)(a,b,c) = sum_f <fp||bc> x2(q,r,a,f)
    hh_x(p;q,r)(a,b,c) = sum_m x2(m,p,c,b) <ma||qr>
    wc_x = pp_x(i;j,k) - pp_x(j;i,k) - pp_x(k;j,i) - hh_x(i;j,k) + hh_x(j;i,k) + hh_x(k;j,i)
    wd_x = x1(i,a)<jk||bc> - x1(j,a)<ik||bc> - x1(k,a)<ji||bc>  [+ f(i,a) x2(j,k,b,c) - f(j,a) x2(i,k,b,c) - f(k,a) x2(j,i,b,c)]
    P(y) = y(abc) - y(bac) - y(cba),   D = e_i + e_j + e_k - e_a - e_b - e_c
    E_LT = sum_{i<j<k} sum_abc P(wc_l + wd_l) P(wc_t) / D / 6
(Kucharski and Bartlett 1998; Crawford and Stanton 1998).  The left numerator is the derivative of the CCSDT feeds of T3 into the singles
and doubles equations contracted with Lambda -- functional() below, which test_lambda_t_cpu.py holds it to.  All of it in np.longdouble;
beside every value its majorant S as in np_triples: absolute values, every minus turned into a plus.
"""
from __future__ import annotations

import itertools

import numpy as np

from np_triples import LD, so_order


def numerators(g, o, x1, x2, f_ov, i, j, k, s=LD(1), f=lambda z: z):
    """(wc_x, wd_x) [a,b,c] of one triple from the amplitudes x1, x2; s = -1 with f = np.abs gives the majorant's terms"""
    O, V = slice(0, o), slice(o, None)
    vovv, ovoo, vvoo = g[V, O, V, V], g[O, V, O, O], g[V, V, O, O]
    fast = g.dtype == np.float64    # (float64: the products through BLAS; np.longdouble: einsum's own loops)

    def pp(p, q, r):    # sum_f <fp||bc> x2(q,r,a,f)
        return np.einsum("fbc,af->abc", f(vovv[:, p]), f(x2[q, r]), optimize=fast)

    def hh(p, q, r):    # sum_m x2(m,p,c,b) <ma||qr>
        return np.einsum("mcb,ma->abc", f(x2[:, p]), f(ovoo[:, :, q, r]), optimize=fast)

    wc = pp(i, j, k) - s * pp(j, i, k) - s * pp(k, j, i) - s * hh(i, j, k) + hh(j, i, k) + hh(k, j, i)
    wd = (f(x1[i])[:, None, None] * f(vvoo[:, :, j, k])[None] - s * f(x1[j])[:, None, None] * f(vvoo[:, :, i, k])[None]
          - s * f(x1[k])[:, None, None] * f(vvoo[:, :, j, i])[None])
    if f_ov is not None:
        wd = wd + (f(f_ov[i])[:, None, None] * f(x2[j, k])[None] - s * f(f_ov[j])[:, None, None] * f(x2[i, k])[None]
                   - s * f(f_ov[k])[:, None, None] * f(x2[j, i])[None])
    return wc, wd


def perm(x, s=LD(1)):
    """P(y) = y(abc) - y(bac) - y(cba)"""
    return x - s * x.transpose(1, 0, 2) - s * x.transpose(2, 1, 0)


def lt_per_triple(g, lev, o, t1, t2, l1, l2, f_ov=None, dtype=LD):
    """-> (val[nt], S[nt]) over so_order(o), np.longdouble (dtype=np.float64: a plain double evaluation, for shapes where that is enough)"""
    g, lev, t1, t2, l1, l2 = (np.asarray(x, dtype=dtype) for x in (g, lev, t1, t2, l1, l2))
    fo = None if f_ov is None else np.asarray(f_ov, dtype=dtype)
    eo, ev = lev[:o], lev[o:]
    dv = ev[:, None, None] + ev[None, :, None] + ev[None, None, :]
    vals, majs = [], []
    for i, j, k in so_order(o):
        d = eo[i] + eo[j] + eo[k] - dv
        res = []
        for s, f in ((dtype(1), lambda z: z), (dtype(-1), np.abs)):
            wc_t, _ = numerators(g, o, t1, t2, fo, i, j, k, s, f)
            wc_l, wd_l = numerators(g, o, l1, l2, fo, i, j, k, s, f)
            res.append(np.sum(perm(wc_l + wd_l, s) * perm(wc_t, s) / f(d)) / 6)
        vals.append(res[0])
        majs.append(res[1])
    return np.array(vals, dtype=dtype), np.array(majs, dtype=dtype)


def left_contraction(g, o, l1, l2, f_ov, X):
    """sum_{i<j<k} sum_abc P(wc_l + wd_l) X_ijkabc / 6 for any X[i,j,k,a,b,c]"""
    g, l1, l2, f_ov, X = (np.asarray(x, dtype=LD) for x in (g, l1, l2, f_ov, X))
    tot = LD(0)
    for i, j, k in so_order(o):
        wc, wd = numerators(g, o, l1, l2, f_ov, i, j, k)
        tot += np.sum(perm(wc + wd) * X[i, j, k]) / 6
    return tot


def functional(g, f_ov, l1, l2, X):
    """sum l_ia R1_ia[X] + 1/4 sum l_ijab R2_ijab[X] with the textbook CCSDT feeds of a fully antisymmetric X_ijkabc into the singles
    and doubles equations:
        R1_ia[X]   = 1/4 sum <mn||ef> X_imnaef
        R2_ijab[X] = sum f_me X_ijmabe + 1/2 P(ab) sum <bm||ef> X_ijmaef - 1/2 P(ij) sum <mn||je> X_imnabe"""
    g, f_ov, l1, l2, X = (np.asarray(x, dtype=LD) for x in (g, f_ov, l1, l2, X))
    o = l1.shape[0]
    O, V = slice(0, o), slice(o, None)
    r1 = LD(0.25) * np.einsum("mnef,imnaef->ia", g[O, O, V, V], X)
    a = np.einsum("bmef,ijmaef->ijab", g[V, O, V, V], X)
    b = np.einsum("mnje,imnabe->ijab", g[O, O, O, V], X)
    r2 = (np.einsum("me,ijmabe->ijab", f_ov, X) + LD(0.5) * (a - a.transpose(0, 1, 3, 2)) - LD(0.5) * (b - b.transpose(1, 0, 2, 3)))
    return np.sum(l1 * r1) + LD(0.25) * np.sum(l2 * r2)


def random_antisymmetric_triples(o, v, seed):
    """X[i,j,k,a,b,c], antisymmetric under every exchange within (i,j,k) and within (a,b,c)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (o, o, o, v, v, v))
    out = np.zeros_like(x)
    for p in itertools.permutations(range(3)):
        sp = np.linalg.det(np.eye(3)[list(p)])
        for q in itertools.permutations(range(3)):
            sq = np.linalg.det(np.eye(3)[list(q)])
            out += sp * sq * x.transpose(*p, *(3 + c for c in q))
    return out / 36.0


def lambda_seed(n, o):
    """seed of the Lambda amplitudes of the np_triples.SO_CASES entry with n spatial and o occupied spin orbitals (test_lambda_t_cpu.py: no
    value is cancelled away with them)"""
    return 901 + 10 * n + o
