"""Non-iterative triples correction to an EOM-IP-CCSD or EOM-EA-CCSD root in plain numpy, one value per item: the reference of the
EOM-IP/EA-(T) tests.  Test infrastructure only.

Definition: np_eom_t's correction of the system enlarged by the ghost orbital g that defines the sectors (np_eom_ipea, np_eom_ipea_left:
embed, embed_plain) -- one more virtual for IP, one more occupied (the last) for EA, every integral, Fock element and level of g zero --
restricted to the triples that contain g.  Items: IP the triples i<j<k of np_triples.so_order(o) (3h2p: a<b beside g), EA the pairs i<j
numbered j(j-1)/2 + i (3p2h: the triple (i, j, g) of the enlarged system).  Two forms:

  * per_item_embedding: np_lambda_t.numerators / np_eom_t.one_index on the enlarged arrays, no hand-derived term;
  * per_item_explicit: the forms the device follows, with its intermediates and letters.

        IP   U_fpb = sum_l r_l <fp||bl>,  Y_mqr = sum_l r_l <ml||qr>,   S+- over (p;q,r) in {+(i;j,k), -(j;i,k), -(k;j,i)}
             conn_x(p;q,r)[a,b] = sum_f <fp||ba> x_qrf + sum_m (x_mpb <ma||qr> - x_mpa <mb||qr>)
             M[a,b] = S+- { conn_r - sum_f U_fpb t_qraf + sum_f U_fpa t_qrbf - sum_m t_mpab Y_mqr }
             L[a,b] = S+- { conn_l + l_p <qr||ab> + [f_pa l_qrb - f_pb l_qra] }
             dw     = sum_{i<j<k} sum_{a<b} L M / (e_i + e_j + e_k - e_a - e_b + w)
        EA   U_fbc = sum_d <fd||bc> r_d,  Y_mar = sum_d <ma||dr> r_d,   P(y) = y(abc) - y(bac) - y(cba)
             conn_x(i,j)[a,b,c] = sum_f <fi||bc> x_jaf - sum_f <fj||bc> x_iaf + sum_m x_mcb <ma||ji>
             m = conn_r - sum_f U_fbc t_jiaf + sum_m t_micb Y_maj - sum_m t_mjcb Y_mai
             l = conn_l + l_a <ij||bc> + [f_ia l_jbc - f_ja l_ibc]
             dw = sum_{i<j} sum_{a<b<c} P(l) P(m) / (e_i + e_j - e_a - e_b - e_c + w)

All of it in np.longdouble; beside every value its majorant S as in np_lambda_t: absolute values, every minus turned into a plus,
|D + w| in the denominator.  test_eom_ipea_t_cpu.py holds the two forms to each other and the embedding to np_fockspace.
"""
from __future__ import annotations

import itertools

import numpy as np

import np_eom_ipea as X
from np_eom_ipea_left import embed, embed_plain
from np_eom_t import one_index
from np_lambda_t import numerators, perm
from np_triples import LD, EPS53, so_order

IP, EA = X.IP, X.EA


def pair_order(o):
    """the pairs i<j in the library's triangular numbering j(j-1)/2 + i"""
    return [(i, j) for j in range(o) for i in range(j)]


def items(sector, o):
    return so_order(o) if sector == IP else pair_order(o)


def nitems(sector, o):
    return o * (o - 1) * (o - 2) // 6 if sector == IP else o * (o - 1) // 2


def admits(sector, o, v):
    return (o >= 3 and v >= 2) if sector == IP else (o >= 2 and v >= 3)


def enlarged_system(sector, g, lev, o, f_ov=None):
    """-> (g', lev', o', f_ov' or None, index of the ghost among the spin orbitals)"""
    n = len(lev)
    v = n - o
    at = n if sector == IP else o
    gg = g
    for ax in range(4):
        gg = np.insert(gg, at, 0.0, axis=ax)
    levg = np.insert(lev, at, 0.0)
    fo = None
    if f_ov is not None:
        fo = np.insert(f_ov, v, 0.0, axis=1) if sector == IP else np.insert(f_ov, o, 0.0, axis=0)
    return gg, levg, (o if sector == IP else o + 1), fo, at


_SIDES = ((LD(1), lambda z: z), (LD(-1), np.abs))


def _embedded(sector, g, lev, o, t2, l1, l2, r1, r2, f_ov, dtype):
    v = len(lev) - o
    gg, levg, og, fo, _ = enlarged_system(sector, np.asarray(g, dtype=dtype), np.asarray(lev, dtype=dtype), o,
                                          None if f_ov is None else np.asarray(f_ov, dtype=dtype))
    T2 = embed_plain(sector, o, v, np.zeros((o, v)), np.asarray(t2))[1].astype(dtype)
    L1, L2 = (a.astype(dtype) for a in embed(sector, o, v, np.asarray(l1, dtype=dtype), np.asarray(l2, dtype=dtype)))
    R1, R2 = (a.astype(dtype) for a in embed(sector, o, v, np.asarray(r1, dtype=dtype), np.asarray(r2, dtype=dtype)))
    return gg, levg, og, fo, T2, L1, L2, R1, R2


def embedding_numerators(sector, g, lev, o, t2, l1, l2, r1, r2, f_ov=None, dtype=np.float64):
    """{triple of the enlarged system: (P(l), P(m)) [a,b,c] over its v' virtuals} for EVERY triple of the enlarged system, with g or not"""
    gg, levg, og, fo, T2, L1, L2, R1, R2 = _embedded(sector, g, lev, o, t2, l1, l2, r1, r2, f_ov, dtype)
    gR = one_index(gg, og, R1)
    zero = np.zeros_like(R1)
    out = {}
    for i, j, k in so_order(og):
        wc_l, wd_l = numerators(gg, og, L1, L2, fo, i, j, k)
        m = numerators(gg, og, zero, R2, None, i, j, k)[0] + numerators(gR, og, zero, T2, None, i, j, k)[0]
        out[(i, j, k)] = (perm(wc_l + wd_l), perm(m))
    return out


def per_item_embedding(sector, g, lev, o, t2, omega, l1, l2, r1, r2, f_ov=None, dtype=LD, elements=False):
    """-> (val[nitems], S[nitems]) over items(sector, o); elements=True: also the list of the summands l m / (D + w) per item, IP [a,b] over
    the v x v tile (zero unless a < b), EA [a,b,c] (zero unless a < b < c)"""
    v = len(lev) - o
    n = nitems(sector, o)
    if not admits(sector, o, v):
        return (np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)) + (([],) if elements else ())
    gg, levg, og, fo, T2, L1, L2, R1, R2 = _embedded(sector, g, lev, o, t2, l1, l2, r1, r2, f_ov, dtype)
    omega = dtype(omega)
    eo, ev = levg[:og], levg[og:]
    dv = ev[:, None, None] + ev[None, :, None] + ev[None, None, :]
    zero = np.zeros_like(R1)
    gRs = [one_index(gg, og, R1, s, f) for s, f in _SIDES]
    vals, majs, elems = [], [], []
    for it in items(sector, o):
        i, j, k = it if sector == IP else (it[0], it[1], o)
        d = eo[i] + eo[j] + eo[k] - dv + omega
        res = []
        for (s, f), gR in zip(_SIDES, gRs):
            wc_l, wd_l = numerators(gg, og, L1, L2, fo, i, j, k, s, f)
            m = numerators(gg, og, zero, R2, None, i, j, k, s, f)[0] + numerators(gR, og, zero, T2, None, i, j, k, s, f)[0]
            x = perm(wc_l + wd_l, s) * perm(m, s) / f(d)
            if sector == IP:        # a < b beside the ghost virtual (the last one): 1/6 of the six placements of g
                x = np.triu(x[:v, :v, v], 1)
            else:
                x = x * (np.arange(v)[:, None, None] < np.arange(v)[None, :, None]) * (np.arange(v)[None, :, None] < np.arange(v)[None, None, :])
            res.append(x)
        vals.append(np.sum(res[0]))
        majs.append(np.sum(res[1]))
        elems.append(res[0])
    out = (np.array(vals, dtype=dtype), np.array(majs, dtype=dtype))
    return out + ((elems,) if elements else ())


def per_item_explicit(sector, g, lev, o, t2, omega, l1, l2, r1, r2, f_ov=None, dtype=LD, elements=False):
    """the same from the explicit forms of the module text"""
    g, lev, t2, l1, l2, r1, r2 = (np.asarray(x, dtype=dtype) for x in (g, lev, t2, l1, l2, r1, r2))
    fo = None if f_ov is None else np.asarray(f_ov, dtype=dtype)
    omega = dtype(omega)
    v = len(lev) - o
    n = nitems(sector, o)
    if not admits(sector, o, v):
        return (np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)) + (([],) if elements else ())
    O, V = slice(0, o), slice(o, None)
    eo, ev = lev[:o], lev[o:]
    E = np.einsum
    vals, majs, elems = [], [], []
    sides = []
    for s, f in _SIDES:
        G = f(g)
        vovv, ovoo, oovv = G[V, O, V, V], G[O, V, O, O], G[O, O, V, V]
        T, R1, R2, L1, L2 = f(t2), f(r1), f(r2), f(l1), f(l2)
        F = None if fo is None else f(fo)
        if sector == IP:
            U, Y = E("l,fpbl->fpb", R1, G[V, O, V, O]), E("l,mlqr->mqr", R1, G[O, O, O, O])
        else:
            U, Y = E("fdbc,d->fbc", G[V, V, V, V], R1), E("madr,d->mar", G[O, V, V, O], R1)
        sides.append((s, f, vovv, ovoo, oovv, T, R1, R2, L1, L2, F, U, Y))
    for it in items(sector, o):
        res = []
        for s, f, vovv, ovoo, oovv, T, R1, R2, L1, L2, F, U, Y in sides:
            if sector == IP:
                i, j, k = it
                d = eo[i] + eo[j] + eo[k] - ev[:, None] - ev[None, :] + omega

                def conn(x, p, q, r):
                    e = E("mb,ma->ab", x[:, p], ovoo[:, :, q, r])
                    return E("fba,f->ab", vovv[:, p], x[q, r]) + e - s * e.T

                def right(p, q, r):
                    u = E("fb,af->ab", U[:, p], T[q, r])
                    return conn(R2, p, q, r) - s * u + u.T - s * E("mab,m->ab", T[:, p], Y[:, q, r])

                def left(p, q, r):
                    x = conn(L2, p, q, r) + L1[p] * oovv[q, r]
                    if F is not None:
                        x = x + F[p][:, None] * L2[q, r][None, :] - s * F[p][None, :] * L2[q, r][:, None]
                    return x
                M = right(i, j, k) - s * right(j, i, k) - s * right(k, j, i)
                Lm = left(i, j, k) - s * left(j, i, k) - s * left(k, j, i)
                res.append(np.triu(Lm * M / f(d), 1))
            else:
                i, j = it
                d = eo[i] + eo[j] - ev[:, None, None] - ev[None, :, None] - ev[None, None, :] + omega

                def conn(x):
                    return (E("fbc,af->abc", vovv[:, i], x[j]) - s * E("fbc,af->abc", vovv[:, j], x[i])
                            + E("mcb,ma->abc", x, ovoo[:, :, j, i]))
                m = (conn(R2) - s * E("fbc,af->abc", U, T[j, i]) + E("mcb,ma->abc", T[:, i], Y[:, :, j])
                     - s * E("mcb,ma->abc", T[:, j], Y[:, :, i]))
                l = conn(L2) + L1[:, None, None] * oovv[i, j][None]
                if F is not None:
                    l = l + F[i][:, None, None] * L2[j][None] - s * F[j][:, None, None] * L2[i][None]
                x = perm(l, s) * perm(m, s) / f(d)
                ar = np.arange(v)
                res.append(x * (ar[:, None, None] < ar[None, :, None]) * (ar[None, :, None] < ar[None, None, :]))
        vals.append(np.sum(res[0]))
        majs.append(np.sum(res[1]))
        elems.append(res[0])
    out = (np.array(vals, dtype=dtype), np.array(majs, dtype=dtype))
    return out + ((elems,) if elements else ())


def tol_factor(sector, o, v):
    """Per range |engine - reference| <= tol_factor * S.  As np_eom_t.tol_factor: two roundings per term of every nested sum against the
    majorant.  The outer sums run over v + o terms on either side (left and right numerator: 4 (v + o)), the elements of U and Y are
    themselves sums of o (IP) or v (EA) products; the reduction tree, the reciprocal and P account for the 64.  Not tuned to any kernel."""
    return (4 * (v + o) + 2 * (o if sector == IP else v) + 64) * EPS53


def ipea_seed(sector, n, o):
    """seed of the left / right vectors of the np_triples.SO_CASES entry with n spatial and o occupied spin orbitals (test_eom_ipea_t_cpu.py:
    no value is cancelled away with them)"""
    return (1501 if sector == IP else 1701) + 10 * n + o


def random_vectors(sector, o, v, seed):
    """(x1, x2) of order one in the sector's layout"""
    return X.random_vector(np.random.default_rng(seed), sector, o, v, size=1.0)


def min_denominator(sector, lev, o):
    """the smallest e_a + e_b (+ e_c) - e_i - e_j (- e_k) of the sector's 3h2p / 3p2h determinants"""
    eo, ev = np.sort(lev[:o]), np.sort(lev[o:])
    return float(ev[:2].sum() - eo[-3:].sum()) if sector == IP else float(ev[:3].sum() - eo[-2:].sum())


def case_vectors(sector, lev, o, seed, nstates=2):
    """(omega[ns], L = [(l1, l2)], R = [(r1, r2)]): random vectors of order one, omega in (0, 1/2 smallest denominator)"""
    v = len(lev) - o
    gap = min_denominator(sector, np.asarray(lev, dtype=float), o)
    assert gap > 0
    omega = np.array([gap * (0.15 + 0.2 * s) for s in range(nstates)])
    L = [random_vectors(sector, o, v, seed + 100 * s) for s in range(nstates)]
    R = [random_vectors(sector, o, v, seed + 100 * s + 50) for s in range(nstates)]
    return omega, L, R


# ------------------------------------------------------------------------------------------------------------------- cases
# np_triples.so_case entries (n, na, nb, fock) beside np_triples.SO_CASES: the smallest extents that admit a sector.  A state has an even
# number of spin orbitals, so IP's o, v = 3, 2 and EA's 2, 3 themselves cannot be loaded; their two even neighbours are here -- o, v = 3, 3
# (the smallest o of IP and the smallest v of EA, a Fock state), 4, 2 (the smallest v of IP) and 2, 4 (the smallest o of EA)
MINIMAL_CASES = [(3, 2, 1, True), (3, 2, 2, False), (3, 1, 1, False)]


def cases(sector):
    """the SO_CASES and MINIMAL_CASES entries that admit the sector"""
    from np_triples import SO_CASES
    return [c for c in SO_CASES + MINIMAL_CASES if admits(sector, c[1] + c[2], 2 * c[0] - c[1] - c[2])]


_REFERENCE = {}


def reference(sector, n, na, nb, fock):
    """(omega[2], L, R, val[2][nitems], S[2][nitems]) of one case: two states and their per-item references (the embedding), computed once"""
    key = (sector, n, na, nb, fock)
    if key not in _REFERENCE:
        from np_triples import so_case
        c = so_case(n, na, nb, fock)
        omega, L, R = case_vectors(sector, c.lev, c.o, ipea_seed(sector, c.n, c.o), 2)
        per = [per_item_embedding(sector, c.g, c.lev, c.o, c.t2, omega[s], *L[s], *R[s], c.f_ov) for s in range(2)]
        _REFERENCE[key] = (omega, L, R, [p[0] for p in per], [p[1] for p in per])
    return _REFERENCE[key]
