"""Reference for the orbital-relaxed one-particle density of spin-orbital CCSD (no GPU).

With L(f, g; t, l) the Lagrangian of np_lambda, D and Gamma its derivatives (np_lambda.density, np_density2), kappa an antisymmetric matrix
over all o + v spin orbitals whose only non-zero elements are kappa_ai = -kappa_ia and U = exp(kappa):

  * gradient_fd: the defining orbital gradient, central differences of L on the rotated (f, g) with t and l held fixed -- no hand-derived
    term.  fock_response = 1 takes f as h + sum_k <pk||qk>, so that rotating the occupied space changes f;
  * gradient_explicit: w0_ai = 2 (X_ai - X_ia), X_pq = sum_r f_pr D_rq + 1/2 sum_rst <pr||st> Gamma_qrst, plus 2 sum_pq D_pq <pa||qi>;
  * gradient_blocks: the same from the stored blocks of Gamma and the state's integral slices, term by term as the device code;
  * hessian_dense / zvector / relaxed_density: A_ai,bj = delta (e_a - e_i) + <ab||ij> + <aj||ib>, A z = -w, D_rel = D + 1/2 z on ov / vo;
  * scf_model: a small spin-unrestricted SCF, so that a model's determinant is a Hartree-Fock solution of its own (h, g).

Gradients and z are (o, v) arrays laid out as t1.
"""
from __future__ import annotations

import numpy as np

import np_density2
import np_lambda
import np_rocc
import np_ucc
from np_ucc import E


# ---------------------------------------------------------------------------------------------------------------- definition
def expm_antisymmetric(kappa):
    w, v = np.linalg.eigh(1j * kappa)            # kappa = -i (i kappa): exp(kappa) = v exp(-i w) v^H
    return np.real(v @ np.diag(np.exp(-1j * w)) @ v.conj().T)


def rotate(f, g, kappa):
    """(U^T f U, g transformed by U on all four indices), U = exp(kappa)"""
    u = expm_antisymmetric(kappa)
    return u.T @ f @ u, E("pqrs,pa,qb,rc,sd->abcd", g, u, u, u, u)


def _rotated(f, g, o, a, i, x, fock_response):
    n = f.shape[0]
    k = np.zeros((n, n))
    k[o + a, i], k[i, o + a] = x, -x
    fr, gr = rotate(f, g, k)
    if fock_response:
        u = expm_antisymmetric(k)
        fr = fr + E("pkqk->pq", gr[:, :o, :, :o]) - u.T @ E("pkqk->pq", g[:, :o, :, :o]) @ u
    return fr, gr


def gradient_fd(c, t, l, fock_response, steps=(2.0 ** -7, 2.0 ** -8)):
    """-> (w from the smaller step, w from the larger): the five-point central stencil (error O(h^4)) at two step sizes; their
    disagreement measures the stencil's own error.  c: dict with g, f, o"""
    g, f, o = c["g"], c["f"], c["o"]
    v = f.shape[0] - o

    def lag(a, i, x):
        fr, gr = _rotated(f, g, o, a, i, x, fock_response)
        return np_lambda.lagrangian(np_rocc.ROCC(gr, fr, o), t[0], t[1], l[0], l[1])
    out = []
    for h in steps:
        w = np.zeros((o, v))
        for i in range(o):
            for a in range(v):
                w[i, a] = (8.0 * (lag(a, i, h) - lag(a, i, -h)) - (lag(a, i, 2 * h) - lag(a, i, -2 * h))) / (12.0 * h)
        out.append(w)
    return out[1], out[0]


# ---------------------------------------------------------------------------------------------------------------- explicit
def gradient_explicit(g, f, o, D, G, fock_response):
    """D: the (o+v)^2 density; G: the whole (o+v)^4 Gamma (np_density2.expand of the blocks)"""
    X = f @ D + 0.5 * E("prst,qrst->pq", g, G)
    w = 2.0 * (X[o:, :o] - X[:o, o:].T)                      # (a, i)
    if fock_response:
        w = w + 2.0 * E("pq,paqi->ai", D, g[:, o:, :, :o])
    return w.T.copy()


def gradient_blocks(cc, f, D, G, fock_response):
    """The same from the six stored blocks G of Gamma and the slices of cc, each term as the device builds it -> (w, terms)"""
    o = cc.o
    oooo, ooov, oovv, ovvo, ovvv, vvvv = cc.oooo, cc.ooov, cc.oovv, cc.ovvo, cc.ovvv, cc.vvvv
    xai = (-0.5 * E("klja,ijkl->ia", ooov, G["oooo"]) + E("jabk,ijkb->ia", ovvo, G["ooov"]) - 0.5 * E("jabc,ijbc->ia", ovvv, G["oovv"])
           + 0.5 * E("jkab,jkib->ia", oovv, G["ooov"]) + E("jcab,ibjc->ia", ovvv, G["ovov"]))
    pair_ai = 0.5 * E("abcd,ibcd->ia", vvvv, G["ovvv"])
    xia = (-0.5 * E("ijkl,klja->ia", oooo, G["ooov"]) - E("ijkb,jakb->ia", ooov, G["ovov"]) - 0.5 * E("ijbc,jabc->ia", oovv, G["ovvv"])
           + 0.5 * E("jkib,jkab->ia", ooov, G["oovv"]) - E("ibcj,jcab->ia", ovvo, G["ovvv"]))
    pair_ia = 0.5 * E("ibcd,abcd->ia", ovvv, G["vvvv"])
    fd = f @ D
    w = 2.0 * ((fd[o:, :o].T - fd[:o, o:]) + (xai + pair_ai) - (xia + pair_ia))
    if fock_response:
        doo, dov, dvv = D[:o, :o], D[:o, o:], D[o:, o:]
        w = w + 2.0 * (E("jk,kija->ia", doo, ooov) + E("jb,jabi->ia", dov, ovvo) + E("jb,jiba->ia", dov, oovv) + E("bc,icab->ia", dvv, ovvv))
    return w, dict(pair_ai=pair_ai, pair_ia=pair_ia)


def hessian_dense(g, lev, o):
    """A[(i,a), (j,b)] over the t1 layout, flattened with a fastest"""
    v = len(lev) - o
    A = E("abij->iajb", g[o:, o:, :o, :o]) + E("ajib->iajb", g[o:, :o, :o, o:])
    A = A.reshape(o * v, o * v).copy()
    A[np.diag_indices(o * v)] += (lev[None, o:] - lev[:o, None]).reshape(-1)
    return A


def zvector(g, lev, o, w):
    v = len(lev) - o
    return np.linalg.solve(hessian_dense(g, lev, o), -w.reshape(-1)).reshape(o, v)


def pcg(A, b, diag, tol, maxiter):
    """Conjugate gradients from x = 0 preconditioned with `diag`, as the device runs them -> (x, iterations, residual 2-norm)"""
    x, r = np.zeros_like(b), b.copy()
    zz = r / diag
    p, rz, it = zz.copy(), float(r @ zz), 0
    while np.sqrt(r @ r) >= tol and it < maxiter:
        Ap = A @ p
        alpha = rz / float(p @ Ap)
        x, r = x + alpha * p, r - alpha * Ap
        zz = r / diag
        rz, old = float(r @ zz), rz
        p = zz + (rz / old) * p
        it += 1
    return x, it, float(np.sqrt(r @ r))


def relaxed_density(D, z, o):
    d = D.copy()
    d[:o, o:] += 0.5 * z
    d[o:, :o] += 0.5 * z.T
    return d


def relaxed_reference(cc, g, f, t, l, fock_response=1):
    """-> dict(D, G (blocks), w, z, D_rel) of a state at given t and l, all through the explicit forms"""
    o = cc.o
    D = np_lambda.density_explicit(cc, t[0], t[1], l[0], l[1])
    G = np_density2.gamma_explicit(t[0], t[1], l[0], l[1])
    w, _ = gradient_blocks(cc, f, D, G, fock_response)
    lev = np.diag(f).copy()
    z = zvector(g, lev, o, w)
    return dict(D=D, G=G, w=w, z=z, D_rel=relaxed_density(D, z, o))


# ---------------------------------------------------------------------------------------------------------------- models
def scf_model(h, chem, na, nb, maxiter=500, tol=1e-13):
    """Spin-unrestricted SCF on (h, chem) from the core guess with DIIS on the commutators -> dict(ca, cb (MO x AO), ea, eb, e_ref)"""
    n = h.shape[0]

    def fock(da, db):
        j = E("pqrs,rs->pq", chem, da + db)
        return h + j - E("prqs,rs->pq", chem, da), h + j - E("prqs,rs->pq", chem, db)
    _, c = np.linalg.eigh(h)
    ca = cb = c
    focks, errs = [], []
    for _ in range(maxiter):
        da, db = ca[:, :na] @ ca[:, :na].T, cb[:, :nb] @ cb[:, :nb].T
        fa, fb = fock(da, db)
        ev = np.concatenate([(fa @ da - da @ fa).ravel(), (fb @ db - db @ fb).ravel()])
        if np.max(np.abs(ev)) < tol:
            ea, ca = np.linalg.eigh(fa)
            eb, cb = np.linalg.eigh(fb)
            break
        focks, errs = (focks + [np.stack([fa, fb])])[-8:], (errs + [ev])[-8:]   # DIIS on the commutators
        m = len(focks)
        if m > 1:
            Bm = -np.ones((m + 1, m + 1))
            Bm[m, m] = 0.0
            Bm[:m, :m] = np.array(errs) @ np.array(errs).T
            rhs = np.zeros(m + 1)
            rhs[m] = -1.0
            cf = np.linalg.lstsq(Bm, rhs, rcond=None)[0][:m]
            fa, fb = sum(x * y for x, y in zip(cf, focks))
        ea, ca = np.linalg.eigh(fa)
        eb, cb = np.linalg.eigh(fb)
    else:
        raise RuntimeError("scf_model did not converge")
    da, db = ca[:, :na] @ ca[:, :na].T, cb[:, :nb] @ cb[:, :nb].T
    fa, fb = fock(da, db)
    e_ref = 0.5 * float(np.sum((h + fa) * da) + np.sum((h + fb) * db))
    return dict(ca=ca.T.copy(), cb=cb.T.copy(), ea=ea, eb=eb, e_ref=e_ref)


def scf_case(h, chem, na, nb):
    """The spin-orbital CCSD problem on the SCF orbitals of (h, chem) -> dict(cc, g, f, o, e_ref, orb, spin, ca, cb)"""
    s = scf_model(h, chem, na, nb)
    ca, cb = s["ca"], s["cb"]

    def mo(c1, c2):
        return E("pi,qj,rk,sl,ijkl->pqrs", c1, c1, c2, c2, chem)
    g, lev, o = np_ucc.so_integrals(mo(ca, ca), mo(ca, cb), mo(cb, cb), s["ea"], s["eb"], na, nb)
    f = np.diag(lev)
    orb, spin = np_ucc.so_order(h.shape[0], na, nb)
    return dict(cc=np_rocc.ROCC(g, f, o), g=g, f=f, o=o, e_ref=s["e_ref"], orb=orb, spin=spin, ca=ca, cb=cb)


def so_operator(V, c):
    """A spin-free one-electron operator (AO basis) over the spin orbitals of an scf_case"""
    va, vb = c["ca"] @ V @ c["ca"].T, c["cb"] @ V @ c["cb"].T
    orb, spin = c["orb"], c["spin"]
    same = spin[:, None] == spin[None, :]
    return np.where(same, np.where(spin[:, None] == 0, va[np.ix_(orb, orb)], vb[np.ix_(orb, orb)]), 0.0)


def ccsd_and_lambda(cc, tol=1e-13, maxiter=300):
    """converged (E_CCSD, t, l) of a ROCC problem"""
    _, e = cc.solve(maxiter, tol, tol)
    t1, t2 = cc.t1.copy(), cc.t2.copy()
    l1, l2 = np_lambda.lambda_solve(cc, t1, t2)
    return e, (t1, t2), (l1, l2)
