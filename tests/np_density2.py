"""Reference for the correlation part of the two-particle density of spin-orbital CCSD (no GPU).

Gamma over all o + v spin orbitals (occupied first) is antisymmetric in p,q and in r,s, Gamma_pqrs = Gamma_rspq, and normalised so that
L = sum f D + 1/4 sum g Gamma for every (f, g), L the Lagrangian of np_lambda and D np_lambda.density.  Two independent forms:

  * gamma_fd: the defining one, a central difference of L in g with f held fixed (exact to rounding: L is linear in g);
  * gamma_explicit: term by term, the form the device code follows -- one carrier per stored block family, then the antisymmetriser
    and the (pq)<->(rs) symmetriser as sums over the images of a carrier value.

Blocks: oooo(i,j,k,l), ooov(i,j,k,a), oovv(i,j,a,b), ovov(i,a,j,b), ovvv(i,a,b,c), vvvv(a,b,c,d); every other block of Gamma is an image
of one of these (expand).  total_rdm2 adds the reference determinant's and the one-particle parts, s_squared evaluates <S^2>.
"""
from __future__ import annotations

import itertools

import numpy as np

import np_lambda
import np_rocc
from np_ucc import E

BLOCKS = ("oooo", "ooov", "oovv", "ovov", "ovvv", "vvvv")


# ---------------------------------------------------------------------------------------------------------------- definition
def perturbation(n, p, q, r, s, eps):
    """+-eps on the antisymmetric images of (pq, rs) and of (rs, pq)"""
    x = np.zeros((n,) * 4)
    for a, b, c, d in ((p, q, r, s), (r, s, p, q)):
        x[a, b, c, d] = x[b, a, d, c] = eps
        x[b, a, c, d] = x[a, b, d, c] = -eps
    return x


def gamma_fd(g, f, o, t1, t2, l1, l2, eps=2.0 ** -6):
    n = g.shape[0]
    pairs = list(itertools.combinations(range(n), 2))
    G = np.zeros((n,) * 4)
    for I, (p, q) in enumerate(pairs):
        for r, s in pairs[:I + 1]:
            x = perturbation(n, p, q, r, s, eps)
            lp = np_lambda.lagrangian(np_rocc.ROCC(g + x, f, o), t1, t2, l1, l2)
            lm = np_lambda.lagrangian(np_rocc.ROCC(g - x, f, o), t1, t2, l1, l2)
            val = (lp - lm) / (2.0 * eps) * (1.0 if (p, q) == (r, s) else 0.5)
            G += perturbation(n, p, q, r, s, val)
    return G


# ---------------------------------------------------------------------------------------------------------------- explicit
def carriers(t1, t2, l1, l2):
    """The unsymmetrised carriers of the six families, in the device's letters: Gamma = 1/8 (images of the carrier)"""
    x = E("ia,jb->ijab", t1, t1)
    tau = t2 + x - x.transpose(0, 1, 3, 2)
    Gvv = -0.5 * E("mnef,mnaf->ae", t2, l2)
    Goo = 0.5 * E("mnef,inef->mi", t2, l2)
    Y = E("ijef,klef->ijkl", tau, l2)                       # o^4 v^2
    M = E("imae,kmfe->iakf", t2, l2)                        # the o^3 v^3 ring product
    Lt = E("mnae,ie->mnia", l2, t1)
    Xoo = E("me,je->mj", l1, t1)
    Xvv = E("me,mb->eb", l1, t1)
    s1 = E("me,imae->ia", l1, t2)
    C = {}
    C["oooo"] = 0.5 * Y
    # one-body pieces times t1 (Goo t, Gvv t) are the assemble kernels' disconnected terms
    C["ooov"] = (-2.0 * E("ke,ijea->ijka", l1, tau) + E("ijkm,ma->ijka", Y, t1) - 4.0 * E("ik,ja->ijka", Goo, t1)
                 + 4.0 * E("iakf,jf->ijka", M, t1) + 2.0 * E("ijae,ke->ijka", l2, t1))
    C["ovvv"] = (2.0 * E("ma,imbc->iabc", l1, tau) + E("mnia,mnbc->iabc", Lt, tau) - 4.0 * E("ac,ib->iabc", Gvv, t1)
                 - 4.0 * E("icna,nb->iabc", M, t1) + 2.0 * E("imbc,ma->iabc", l2, t1))
    C["ovov"] = -4.0 * E("ja,ib->iajb", l1, t1) - 4.0 * E("ibja->iajb", M) + 4.0 * E("jmia,mb->iajb", Lt, t1)
    Mt = E("ibnf,jf->ibnj", M, t1)
    C["oovv"] = (tau + l2 + 4.0 * E("ia,jb->ijab", s1, t1) - 2.0 * E("mj,imab->ijab", Xoo, t2) + 2.0 * E("eb,ijea->ijab", Xvv, tau)
                 - 2.0 * E("in,njab->ijab", Goo, tau) + 2.0 * E("fb,ijaf->ijab", Gvv, tau) + 0.25 * E("ijmn,mnab->ijab", Y, tau)
                 + 2.0 * E("ibnf,njaf->ijab", M, t2) + 4.0 * E("ibnj,na->ijab", Mt, t1))
    C["vvvv"] = 0.5 * E("mnab,mncd->abcd", l2, tau)
    return C


def gamma_explicit(t1, t2, l1, l2):
    """-> dict of the six stored blocks"""
    C = carriers(t1, t2, l1, l2)

    def A01(x):
        return x - x.transpose(1, 0, 2, 3)

    def A23(x):
        return x - x.transpose(0, 1, 3, 2)
    G = {}
    y = A23(A01(C["oooo"]))
    G["oooo"] = 0.125 * (y + y.transpose(2, 3, 0, 1))
    G["ooov"] = 0.125 * A01(C["ooov"])
    G["oovv"] = 0.125 * A23(A01(C["oovv"]))
    G["ovov"] = 0.125 * (C["ovov"] + C["ovov"].transpose(2, 3, 0, 1))
    G["ovvv"] = 0.125 * A23(C["ovvv"])
    y = A23(A01(C["vvvv"]))
    G["vvvv"] = 0.125 * (y + y.transpose(2, 3, 0, 1))
    return G


def expand(G, o, v):
    """The whole (o+v)^4 Gamma from the six stored blocks"""
    n = o + v
    O, V = slice(0, o), slice(o, n)
    F = np.zeros((n,) * 4)
    F[O, O, O, O] = G["oooo"]
    F[V, V, V, V] = G["vvvv"]
    x = G["ooov"]
    F[O, O, O, V], F[O, O, V, O] = x, -x.transpose(0, 1, 3, 2)
    F[O, V, O, O], F[V, O, O, O] = x.transpose(2, 3, 0, 1), -x.transpose(3, 2, 0, 1)
    x = G["oovv"]
    F[O, O, V, V], F[V, V, O, O] = x, x.transpose(2, 3, 0, 1)
    x = G["ovov"]
    F[O, V, O, V], F[V, O, O, V] = x, -x.transpose(1, 0, 2, 3)
    F[O, V, V, O], F[V, O, V, O] = -x.transpose(0, 1, 3, 2), x.transpose(1, 0, 3, 2)
    x = G["ovvv"]
    F[O, V, V, V], F[V, O, V, V] = x, -x.transpose(1, 0, 2, 3)
    F[V, V, O, V], F[V, V, V, O] = x.transpose(2, 3, 0, 1), -x.transpose(2, 3, 1, 0)
    return F


def blocks_of(F, o):
    """the six stored blocks of a full Gamma"""
    O, V = slice(0, o), slice(o, None)
    sl = dict(o=O, v=V)
    return {k: F[tuple(sl[c] for c in k)].copy() for k in BLOCKS}


def pairs_of(x):
    """ga(ab, cd), a < b, c < d, of a vvvv block (pair index ab = a + b (b - 1) / 2, the ladder's)"""
    v = x.shape[0]
    pr = [(a, b) for b in range(v) for a in range(b)]
    if not pr:
        return np.zeros((0, 0))
    a, b = np.array(pr).T
    return x[a[:, None], b[:, None], a[None, :], b[None, :]]


def unpair(ga, v):
    x = np.zeros((v,) * 4)
    pr = [(a, b) for b in range(v) for a in range(b)]
    for I, (a, b) in enumerate(pr):
        for J, (c, d) in enumerate(pr):
            x[a, b, c, d] = x[b, a, d, c] = ga[I, J]
            x[b, a, c, d] = x[a, b, d, c] = -ga[I, J]
    return x


def family_energies(G, g, o):
    """1/4 sum g Gamma per family with all its images: oooo, ooov (4 images), oovv (2), ovov (4), ovvv (4), vvvv"""
    gb = blocks_of(g, o)
    w = dict(oooo=1.0, ooov=4.0, oovv=2.0, ovov=4.0, ovvv=4.0, vvvv=1.0)
    return np.array([0.25 * w[k] * float(np.sum(gb[k] * G[k])) for k in BLOCKS])


# ---------------------------------------------------------------------------------------------------------------- full density
def total_rdm2(d, gamma, nocc):
    """<a+_p a+_q a_s a_r> from the correlation parts d (one-particle) and gamma; the reference fills the first nocc spin orbitals"""
    n = d.shape[0]
    g0 = np.zeros((n, n))
    g0[:nocc, :nocc] = np.eye(nocc)
    ref = E("pr,qs->pqrs", g0, g0) - E("ps,qr->pqrs", g0, g0)
    one = E("pr,qs->pqrs", d, g0) + E("qs,pr->pqrs", d, g0) - E("ps,qr->pqrs", d, g0) - E("qr,ps->pqrs", d, g0)
    return ref + one + gamma


def s_squared(gtot, orb, spin, nalpha, nbeta, beta_in_alpha=None):
    """<S^2> = N/2 + Ms^2 - sum_PQ Gtot[P beta, Q alpha, Q beta, P alpha]; orb / spin: spatial index and spin (0 alpha) of every spin
    orbital; beta_in_alpha[b, a] = <beta orbital b | alpha orbital a> (the identity when both spins share one orbital set)"""
    ia, ib = np.where(spin == 0)[0], np.where(spin == 1)[0]
    n = int(max(orb)) + 1
    M = np.eye(n) if beta_in_alpha is None else beta_in_alpha
    S = M[np.ix_(orb[ib], orb[ia])]                          # (beta spin orbital, alpha spin orbital)
    x = gtot[np.ix_(ib, ia, ib, ia)]                         # [p beta, q alpha, r beta, s alpha]
    ms = 0.5 * (nalpha - nbeta)
    return 0.5 * (nalpha + nbeta) + ms * ms - float(E("pqrs,ps,rq->", x, S, S))
