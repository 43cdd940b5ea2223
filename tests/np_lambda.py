"""Reference for the spin-orbital CCSD Lambda equations and the unrelaxed one-particle density (no GPU).

Two independent forms over np_rocc.ROCC:

  * the defining one, with no hand-derived term: L(t, l) = E(t) + sum l1 R1 + 1/4 sum l2 R2 with R the CCSD residual that
    ROCC.iterate evaluates before its division; the Jacobian dR/dt and dE/dt by the complex step Im f(t + i h u) / h over the unique
    amplitudes (singles; doubles i < j, a < b as the antisymmetric four-element variation), the density by a central difference in f
    (L is linear in f);
  * the explicit one, term by term with lambda-independent one- and two-body H-bar elements plus G_vv / G_oo (Gauss and Stanton,
    J. Chem. Phys. 103, 3561 (1995)): the form the device code follows, with the same intermediates and the same letters.

Amplitudes t1(i,a), t2(i,j,a,b), l1(i,a), l2(i,j,a,b); g[p,q,r,s] = <pq||rs>, f the full Fock matrix, occupied first.
"""
from __future__ import annotations

import itertools

import numpy as np

import np_rocc
from np_ucc import E

H = 1e-30


# ---------------------------------------------------------------------------------------------------------------- definition
def residual(cc, t1, t2):
    """(E, R1, R2) of the CCSD equations at t (real or complex): R = (what ROCC.iterate divides) - D t"""
    keep = cc.t1, cc.t2
    cc.t1, cc.t2 = t1, t2
    try:
        cc.iterate()
        r1, r2 = (cc.t1 - t1) * cc.D1, (cc.t2 - t2) * cc.D2
    finally:
        cc.t1, cc.t2 = keep
    e = 0.25 * np.sum(cc.oovv * t2) + 0.5 * E("ijab,ia,jb->", cc.oovv, t1, t1) + np.sum(cc.f_ov * t1)
    return e, r1, r2


def unique(o, v):
    """the unique amplitudes: [(i, a)], [(i, j, a, b) with i < j, a < b]"""
    s = [(i, a) for i in range(o) for a in range(v)]
    d = [(i, j, a, b) for i, j in itertools.combinations(range(o), 2) for a, b in itertools.combinations(range(v), 2)]
    return s, d


def pack(x1, x2):
    s, d = unique(*x1.shape)
    return np.array([x1[k] for k in s] + [x2[k] for k in d], dtype=x1.dtype)


def unpack(x, o, v):
    s, d = unique(o, v)
    x1, x2 = np.zeros((o, v), x.dtype), np.zeros((o, o, v, v), x.dtype)
    for k, (i, a) in enumerate(s):
        x1[i, a] = x[k]
    for k, (i, j, a, b) in enumerate(d):
        y = x[len(s) + k]
        x2[i, j, a, b] = x2[j, i, b, a] = y
        x2[j, i, a, b] = x2[i, j, b, a] = -y
    return x1, x2


def jacobian(cc, t1, t2):
    """-> (dE/dt over the unique amplitudes, A[mu, nu] = dR_mu / dt_nu)"""
    o, v = cc.o, cc.v
    n = len(pack(t1, t2))
    A, dE = np.zeros((n, n)), np.zeros(n)
    for nu in range(n):
        u = np.zeros(n, complex)
        u[nu] = 1j * H
        u1, u2 = unpack(u, o, v)
        e, r1, r2 = residual(cc, t1 + u1, t2 + u2)
        dE[nu] = e.imag / H
        A[:, nu] = pack(r1, r2).imag / H
    return dE, A


def lambda_residual(cc, t1, t2, l1, l2, jac=None):
    """G1, G2 = dL/dt (G2 along the antisymmetric unit variation)"""
    dE, A = jac if jac is not None else jacobian(cc, t1, t2)
    return unpack(dE + A.T @ pack(l1, l2), cc.o, cc.v)


def lambda_solve(cc, t1, t2, jac=None):
    dE, A = jac if jac is not None else jacobian(cc, t1, t2)
    return unpack(np.linalg.solve(A.T, -dE), cc.o, cc.v)


def lagrangian(cc, t1, t2, l1, l2):
    e, r1, r2 = residual(cc, t1, t2)
    return float(np.real(e + np.sum(l1 * r1) + 0.25 * np.sum(l2 * r2)))


def density(g, f, o, t1, t2, l1, l2, eps=2.0 ** -6):
    """D_pq = 1/2 (dL/df_pq + dL/df_qp), by central difference in f (exact to rounding: L is linear in f)"""
    n = f.shape[0]
    d = np.zeros((n, n))
    for p in range(n):
        for q in range(p + 1):
            x = np.zeros((n, n))
            x[p, q] += eps
            x[q, p] += eps
            lp = lagrangian(np_rocc.ROCC(g, f + x, o), t1, t2, l1, l2)
            lm = lagrangian(np_rocc.ROCC(g, f - x, o), t1, t2, l1, l2)
            d[p, q] = d[q, p] = 0.5 * (lp - lm) / (2.0 * eps)
    return d


# ---------------------------------------------------------------------------------------------------------------- explicit
def antisym_random(rng, o, v, size=0.3):
    x1 = rng.uniform(-size, size, (o, v))
    x2 = rng.uniform(-size, size, (o, o, v, v))
    x2 = x2 - x2.transpose(1, 0, 2, 3)
    x2 = 0.5 * (x2 - x2.transpose(0, 1, 3, 2))
    return x1, np.clip(x2, -size, size)


def hbar(cc, t1, t2):
    """The T-fixed intermediates of the Lambda equations (the device builds these once, so_lambda_init); f_oo / f_vv without
    their diagonals, which are the denominators."""
    oovv, ooov, ovvv, vovv, ovvo, oovo, oooo, vvvv, ovoo = (cc.oovv, cc.ooov, cc.ovvv, cc.vovv, cc.ovvo, cc.oovo, cc.oooo, cc.vvvv,
                                                             cc.ovoo)
    x = E("ia,jb->ijab", t1, t1)
    tau = t2 + x - x.transpose(0, 1, 3, 2)
    I = {}
    I["tau"] = tau
    Hov = cc.f_ov + E("nf,mnef->me", t1, oovv)
    Hoo = (cc.f_oo + E("ie,me->mi", t1, cc.f_ov) + E("ne,mnie->mi", t1, ooov) + 0.5 * E("inef,mnef->mi", tau, oovv))
    Hvv = (cc.f_vv - E("ma,me->ae", t1, cc.f_ov) + E("mf,mafe->ae", t1, ovvv) - 0.5 * E("mnaf,mnef->ae", tau, oovv))
    y = E("je,mnie->mnij", t1, ooov)
    Hoooo = oooo + y - y.transpose(0, 1, 3, 2) + 0.5 * E("ijef,mnef->mnij", tau, oovv)
    Hvovv = vovv - E("na,nmef->amef", t1, oovv)
    Hooov = ooov - E("if,mnef->mnie", t1, oovv)
    ro = t2 + E("jf,nb->jnfb", t1, t1)
    Hovvo = ovvo + E("jf,mbef->mbej", t1, ovvv) - E("nb,mnej->mbej", t1, oovo) - E("jnfb,mnef->mbej", ro, oovv)
    # H_abei, stored (i,e,a,b).  t_if W_abef without W_abef: the bare o v^4 product, the two t1 parts through Zv(m,i,a,e) =
    # t_if <am||ef>, and the tau part together with 1/2 tau_mnab <mn||ei> as -1/2 tau_mnab H_mnie
    Zv = E("if,amef->miae", t1, vovv)
    q = ovvo - E("nibf,mnef->mbei", t2, oovv)
    p1 = -E("miaf,mbef->ieab", t2, ovvv) - E("ma,mbei->ieab", t1, q) - E("mb,miae->ieab", t1, Zv)
    Hvvvo = (E("abei->ieab", cc.vvvo) - E("me,miab->ieab", Hov, t2) + E("if,abef->ieab", t1, vvvv)
             - 0.5 * E("mnab,mnie->ieab", tau, Hooov) + p1 - p1.transpose(0, 1, 3, 2))
    # H_mbij, stored (m,b,i,j)
    p2 = E("jnbe,mnie->mbij", t2, ooov) + E("ie,mbej->mbij", t1, q)
    Hovoo = (ovoo - E("me,ijbe->mbij", Hov, t2) - E("nb,mnij->mbij", t1, Hoooo) + 0.5 * E("ijef,mbef->mbij", tau, ovvv)
             + p2 - p2.transpose(0, 1, 3, 2))
    I.update(Hov=Hov, Hoo=Hoo, Hvv=Hvv, Hoooo=Hoooo, Hvovv=Hvovv, Hooov=Hooov, Hovvo=Hovvo, Hvvvo=Hvvvo, Hovoo=Hovoo)
    return I


def lambda_rhs_explicit(cc, t1, t2, l1, l2, I=None):
    """X1, X2 with G = X - D l: what the device divides by D (the Jacobi step l <- l + G / D = X / D)"""
    I = I if I is not None else hbar(cc, t1, t2)
    tau, Hov, Hoo, Hvv = I["tau"], I["Hov"], I["Hoo"], I["Hvv"]
    Gvv = -0.5 * E("mnef,mnaf->ae", t2, l2)
    Goo = 0.5 * E("mnef,inef->mi", t2, l2)
    x1 = (Hov + E("ie,ea->ia", l1, Hvv) - E("ma,im->ia", l1, Hoo) + E("me,ieam->ia", l1, I["Hovvo"])
          + 0.5 * E("imef,maef->ia", l2, I["Hvvvo"]) - 0.5 * E("mnae,iemn->ia", l2, I["Hovoo"])
          - E("ef,eifa->ia", Gvv, I["Hvovv"]) - E("mn,mina->ia", Goo, I["Hooov"]))
    # 1/2 l_ijef H_efab as so_ladder treats 1/2 tau_ijef W_abef: bare part (the device: over antisymmetric pairs against va), the
    # t1 parts through Lt(i,j,m,e) = l_ijef t_mf, the tau part as (l . tau over ef) -> o^4, then x <mn||ab>
    Lt = E("ijef,mf->ijme", l2, t1)
    Loo = E("ijef,mnef->ijmn", l2, tau)
    lad = (0.5 * E("ijef,efab->ijab", l2, cc.vvvv) - E("ijme,emab->ijab", Lt, cc.vovv) + 0.25 * E("ijmn,mnab->ijab", Loo, cc.oovv)
           + 0.5 * E("mnab,ijmn->ijab", l2, I["Hoooo"]))
    AB = E("imae,jebm->ijab", l2, I["Hovvo"]) + E("ia,jb->ijab", l1, Hov)
    A = -E("imab,jm->ijab", l2, Hoo) + E("ie,ejab->ijab", l1, I["Hvovv"]) - E("imab,mj->ijab", cc.oovv, Goo)
    B = E("ijae,eb->ijab", l2, Hvv) - E("ma,ijmb->ijab", l1, I["Hooov"]) + E("ijae,be->ijab", cc.oovv, Gvv)
    x2 = (cc.oovv + lad + AB - AB.transpose(1, 0, 2, 3) - AB.transpose(0, 1, 3, 2) + AB.transpose(1, 0, 3, 2)
          + A - A.transpose(1, 0, 2, 3) + B - B.transpose(0, 1, 3, 2))
    return x1, x2


def lambda_residual_explicit(cc, t1, t2, l1, l2, I=None):
    x1, x2 = lambda_rhs_explicit(cc, t1, t2, l1, l2, I)
    return x1 - cc.D1 * l1, x2 - cc.D2 * l2


def pseudo_energy(cc, l1, l2):
    return float(0.25 * np.sum(cc.oovv * l2) + np.sum(cc.f_ov * l1))


def density_explicit(cc, t1, t2, l1, l2):
    """The symmetrised correlation density over all o + v spin orbitals (occupied first)"""
    o, v = cc.o, cc.v
    Gvv = -0.5 * E("mnef,mnaf->ae", t2, l2)
    Goo = 0.5 * E("mnef,inef->mi", t2, l2)
    doo = -E("ia,ma->mi", l1, t1) - Goo                                   # dL/df_mi
    dvv = E("ia,ie->ae", l1, t1) - Gvv                                    # dL/df_ae
    dov = (t1 + l1 + E("ia,imae->me", l1, t2) - E("ia,ie,ma->me", l1, t1, t1) + E("be,mb->me", Gvv, t1) - E("mj,je->me", Goo, t1))
    d = np.zeros((o + v, o + v), dov.dtype)
    d[:o, :o] = 0.5 * (doo + doo.T)
    d[o:, o:] = 0.5 * (dvv + dvv.T)
    d[:o, o:] = 0.5 * dov
    d[o:, :o] = 0.5 * dov.T
    return d


def jacobi(cc, t1, t2, maxiter=200, tol=1e-10):
    """l <- l + G / D from l = t, no DIIS -> (l1, l2, iterations)"""
    I = hbar(cc, t1, t2)
    l1, l2 = t1.copy(), t2.copy()
    for it in range(1, maxiter + 1):
        x1, x2 = lambda_rhs_explicit(cc, t1, t2, l1, l2, I)
        n1, n2 = x1 / cc.D1, x2 / cc.D2
        d = max(np.max(np.abs(n1 - l1)), np.max(np.abs(n2 - l2)))
        l1, l2 = n1, n2
        if d < tol:
            return l1, l2, it
    raise RuntimeError("Lambda Jacobi iteration did not converge")


# ---------------------------------------------------------------------------------------------------------------- models
def model(n, na, nb, seed, fov=0.15, fdiag=0.05, canonical=False):
    """A small random symmetric-positive two-electron model Hamiltonian: (pq|rs) = sum_k B[k,p,q] B[k,r,s] with symmetric B, well
    separated levels, and -- unless canonical -- a full spin Fock matrix with max |f_ov| ~ fov and off-diagonal f_oo / f_vv elements up
    to fdiag.  -> (g, f, o, dict(chem, fa, fb))"""
    import np_ucc
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n + 2, n, n)) * 0.15
    B = B + B.transpose(0, 2, 1)
    chem = np.einsum("kpq,krs->pqrs", B, B)

    def fock(no):
        lev = np.concatenate([-2.5 + 0.6 * np.arange(no), 1.0 + 0.7 * np.arange(n - no)])
        fm = np.diag(lev + 0.05 * rng.standard_normal(n))
        if not canonical:
            x = np.triu(rng.uniform(-1.0, 1.0, (n, n)), 1)
            x[:no, no:] *= fov
            x[:no, :no] *= fdiag
            x[no:, no:] *= fdiag
            fm = fm + x + x.T
        return fm
    fa, fb = fock(na), fock(nb)
    g, _, o = np_ucc.so_integrals(chem, chem, chem, np.diag(fa).copy(), np.diag(fb).copy(), na, nb)
    return g, np_rocc.so_fock(fa, fb, na, nb), o, dict(chem=chem, fa=fa, fb=fb)


def two_electron_model(n, seed):
    """One alpha and one beta electron in n orbitals that are NOT the determinant's Hartree-Fock orbitals: h, chem and the spin Fock
    matrices of the determinant that fills orbital 0 of each spin (full matrices: f_ov != 0).  CCSD is exact here."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n + 2, n, n)) * 0.1
    B = B + B.transpose(0, 2, 1)
    chem = np.einsum("kpq,krs->pqrs", B, B)
    h = 0.05 * rng.standard_normal((n, n))
    h = np.diag(-2.5 + 2.0 * np.arange(n)) + h + h.T
    fa, fb = np_rocc.fock_ro(h, chem, 1, 1)
    return h, chem, fa, fb


def fci_two_electron_density(h, chem):
    """-> (lowest electronic energy, alpha density, beta density) over |p alpha, q beta>"""
    n = h.shape[0]
    one = np.eye(n)
    Hm = (np.einsum("pr,qs->pqrs", h, one) + np.einsum("pr,qs->pqrs", one, h) + chem.transpose(0, 2, 1, 3)).reshape(n * n, n * n)
    w, vec = np.linalg.eigh(Hm)
    c = vec[:, 0].reshape(n, n)
    return float(w[0]), c @ c.T, c.T @ c
