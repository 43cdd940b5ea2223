"""Non-iterative triples correction to an EOM-EE-CCSD excitation energy in plain numpy, one value per triple: the reference of the EOM-(T)
tests.  Test infrastructure only.

Conventions of np_lambda_t.py (pp_x, hh_x, wc_x, wd_x, P, D).  For i<j<k, an excitation energy w, a left vector (l1, l2) and a right
vector (r1, r2):
    l  = wc_l[g] + wd_l                       the left numerator of Lambda-CCSD(T) with l for lambda
    m  = wc_r2[g] + wc_t2[gR]                 gR = the one-index transform of g by r1 (one_index below)
    dw = sum_{i<j<k} sum_abc P(l) P(m) / (D + w) / 6
np_fockspace.py evaluates the operator definition  m = <mu3| [H, R2] + [[H, R1], T2] |0>,  l = <0| (L1 + L2) H |mu3>  literally;
test_eom_t_cpu.py holds this file to it.  All of it in np.longdouble; beside every value its majorant S as in np_lambda_t: absolute values,
every minus turned into a plus, |D + w| in the denominator.
"""
from __future__ import annotations

import numpy as np

from np_lambda_t import numerators, perm
from np_triples import LD, EPS53, so_order


def one_index(g, o, r1, s=LD(1), f=lambda z: z):
    """The two blocks of gR = the elements of [V, R1] that m needs, as a full-size array that is zero elsewhere.  A ket-side occupied index q
    contributes + sum_d g(..d..) r(q,d), a bra-side virtual index a contributes - sum_l r(l,a) g(..l..).  In pp the integral <fp||bc> is
    the element <bc||fp> of the operator (b, c created, f and p annihilated), in hh <ma||qr> stands as written:
        gR(f,p,b,c) = sum_d <fd||bc> r(p,d) - sum_l r(l,b) <fp||lc> - sum_l r(l,c) <fp||bl>
        gR(m,a,q,r) = sum_d <ma||dr> r(q,d) + sum_d <ma||qd> r(r,d) - sum_l r(l,a) <ml||qr>
    s = -1 with f = np.abs gives the majorant's terms."""
    O, V = slice(0, o), slice(o, None)
    g, r = f(g), f(r1)
    out = np.zeros_like(g)
    out[V, O, V, V] = (np.einsum("fdbc,pd->fpbc", g[V, V, V, V], r) - s * np.einsum("lb,fplc->fpbc", r, g[V, O, O, V])
                       - s * np.einsum("lc,fpbl->fpbc", r, g[V, O, V, O]))
    out[O, V, O, O] = (np.einsum("madr,qd->maqr", g[O, V, V, O], r) + np.einsum("maqd,rd->maqr", g[O, V, O, V], r)
                       - s * np.einsum("la,mlqr->maqr", r, g[O, O, O, O]))
    return out


def eom_t_per_triple(g, lev, o, t2, omega, l1, l2, r1, r2, f_ov=None, dtype=LD):
    """-> (val[nt], S[nt]) over so_order(o)"""
    g, lev, t2, l1, l2, r1, r2 = (np.asarray(x, dtype=dtype) for x in (g, lev, t2, l1, l2, r1, r2))
    fo = None if f_ov is None else np.asarray(f_ov, dtype=dtype)
    omega = dtype(omega)
    v = len(lev) - o
    if o < 3 or v < 3:
        return np.zeros(0, dtype=dtype), np.zeros(0, dtype=dtype)
    eo, ev = lev[:o], lev[o:]
    dv = ev[:, None, None] + ev[None, :, None] + ev[None, None, :]
    zero = np.zeros_like(r1)
    gRs = [one_index(g, o, r1, s, f) for s, f in ((dtype(1), lambda z: z), (dtype(-1), np.abs))]
    vals, majs = [], []
    for i, j, k in so_order(o):
        d = eo[i] + eo[j] + eo[k] - dv + omega
        res = []
        for (s, f), gR in zip(((dtype(1), lambda z: z), (dtype(-1), np.abs)), gRs):
            wc_l, wd_l = numerators(g, o, l1, l2, fo, i, j, k, s, f)
            m = numerators(g, o, zero, r2, None, i, j, k, s, f)[0] + numerators(gR, o, zero, t2, None, i, j, k, s, f)[0]
            res.append(np.sum(perm(wc_l + wd_l, s) * perm(m, s) / f(d)) / 6)
        vals.append(res[0])
        majs.append(res[1])
    return np.array(vals, dtype=dtype), np.array(majs, dtype=dtype)


def numerator_arrays(g, o, t2, l1, l2, r1, r2, f_ov=None):
    """(P(m), P(l)) [i,j,k,a,b,c] at i<j<k (float64), for the element-wise comparison with np_fockspace.eom_t_numerators"""
    v = g.shape[0] - o
    pm, pl = np.zeros((o, o, o, v, v, v)), np.zeros((o, o, o, v, v, v))
    gR = one_index(g, o, r1)
    zero = np.zeros_like(r1)
    for i, j, k in so_order(o):
        wc_l, wd_l = numerators(g, o, l1, l2, f_ov, i, j, k)
        m = numerators(g, o, zero, r2, None, i, j, k)[0] + numerators(gR, o, zero, t2, None, i, j, k)[0]
        pm[i, j, k], pl[i, j, k] = perm(m), perm(wc_l + wd_l)
    return pm, pl


def tol_factor(o, v):
    """Per range |engine - reference| <= tol_factor * S.  As np_triples.tol_factor: two roundings per term of every nested sum against the
    majorant.  The outer sums run over the concatenated index of length 2 (v + o) (r2 against g, t2 against gR), the elements of gR are
    themselves sums of at most v + 2 o products; the reduction tree, the reciprocal and P account for the 64.  Not tuned to any kernel."""
    return (4 * (v + o) + 2 * (v + 2 * o) + 64) * EPS53


def eom_seed(n, o):
    """seed of the left / right vectors of the np_triples.SO_CASES entry with n spatial and o occupied spin orbitals (test_eom_t_cpu.py:
    no value is cancelled away with them)"""
    return 1301 + 10 * n + o


def case_vectors(c, nstates=2):
    """(omega[ns], L = [(l1, l2)], R = [(r1, r2)]) of an SO case: random antisymmetric vectors of order one, omega in (0, 1/2 min gap)"""
    from np_triples import random_so_amplitudes
    eo, ev = np.sort(c.lev[:c.o]), np.sort(c.lev[c.o:])
    gap = float(ev[:3].sum() - eo[-3:].sum())
    assert gap > 0
    seed = eom_seed(c.n, c.o)
    omega = np.array([gap * (0.15 + 0.2 * s) for s in range(nstates)])
    L = [random_so_amplitudes(c.o, c.v, seed + 100 * s) for s in range(nstates)]
    R = [random_so_amplitudes(c.o, c.v, seed + 100 * s + 50) for s in range(nstates)]
    return omega, L, R
