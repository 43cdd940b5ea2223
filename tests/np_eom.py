"""Reference for EOM-EE-CCSD on the spin-orbital CCSD state (no GPU).

The right-hand EOM matrix in the singles and doubles space is the Jacobian A = dR/dt of the CCSD residual (np_lambda.jacobian): for an
antisymmetric r = [r1; r2], sigma(r) = A r is the directional derivative Im R(t + i h r) / h, at any t.  Two forms:

  * sigma_definition: that complex step, with no hand-derived term;
  * sigma_explicit: term by term over the lambda-independent H-bar elements of np_lambda.hbar -- the form the device code follows,
    with the same intermediates and the same letters.

On full (i,j,a,b) storage the inner product is <x, y> = sum x1 y1 + 1/4 sum x2 y2; with it the matrix in the unique basis is A itself.
davidson() is the block Davidson iteration of the device code, rule by rule (guess, two projection passes, clamp, collapse).
"""
from __future__ import annotations

import numpy as np

import np_lambda
from np_ucc import E

DROP, CLAMP = 1e-10, 1e-4


# ---------------------------------------------------------------------------------------------------------------- sigma
def sigma_definition(cc, t1, t2, r1, r2):
    _, s1, s2 = np_lambda.residual(cc, t1 + 1j * np_lambda.H * r1, t2 + 1j * np_lambda.H * r2)
    return s1.imag / np_lambda.H, s2.imag / np_lambda.H


def sigma_explicit(cc, t1, t2, r1, r2, I=None):
    I = I if I is not None else np_lambda.hbar(cc, t1, t2)
    tau, Hov, Hoo, Hvv = I["tau"], I["Hov"], I["Hoo"], I["Hvv"]
    oovv = cc.oovv
    s1 = (E("ae,ie->ia", Hvv, r1) - E("mi,ma->ia", Hoo, r1) + E("me,imae->ia", Hov, r2) + E("maei,me->ia", I["Hovvo"], r1)
          - 0.5 * E("mnie,mnae->ia", I["Hooov"], r2) + 0.5 * E("amef,imef->ia", I["Hvovv"], r2) - cc.D1 * r1)
    Yvv = E("bmef,mf->be", I["Hvovv"], r1) - 0.5 * E("mnef,mnbf->be", oovv, r2)
    Yoo = E("mnje,ne->mj", I["Hooov"], r1) + 0.5 * E("mnef,jnef->mj", oovv, r2)
    # 1/2 r_ijef W_abef without W_abef, as the T iteration's ladder: the bare part, the t1 parts through Z(i,j,a,m), the tau part as
    # (r . <mn||ef> over ef) -> o^4, then x tau;  + 1/2 H_mnij r_mnab
    Z = 0.5 * E("ijef,amef->ijam", r2, cc.vovv)
    Roo = E("ijef,mnef->ijmn", r2, oovv)
    lad = (0.5 * E("ijef,abef->ijab", r2, cc.vvvv) - E("mb,ijam->ijab", t1, Z) + E("ma,ijbm->ijab", t1, Z)
           + 0.25 * E("ijmn,mnab->ijab", Roo, tau) + 0.5 * E("mnij,mnab->ijab", I["Hoooo"], r2))
    AB = E("mbej,imae->ijab", I["Hovvo"], r2)
    A = -E("mj,imab->ijab", Hoo, r2) + E("jeab,ie->ijab", I["Hvvvo"], r1) - E("mj,imab->ijab", Yoo, t2)
    B = E("be,ijae->ijab", Hvv, r2) - E("mbij,ma->ijab", I["Hovoo"], r1) + E("be,ijae->ijab", Yvv, t2)
    s2 = (lad + AB - AB.transpose(1, 0, 2, 3) - AB.transpose(0, 1, 3, 2) + AB.transpose(1, 0, 3, 2)
          + A - A.transpose(1, 0, 2, 3) + B - B.transpose(0, 1, 3, 2) - cc.D2 * r2)
    return s1, s2


def dot(x1, x2, y1, y2):
    return float(np.sum(x1 * y1) + 0.25 * np.sum(x2 * y2))


# ---------------------------------------------------------------------------------------------------------------- Davidson
def guess_order(cc):
    """the unique amplitudes by ascending -D (the diagonal guess of A), ties by flat index in the device's (Fortran) storage order:
    singles i + o a first, then doubles i + o (j + o (a + v b)) -> list of ("s", i, a) / ("d", i, j, a, b)"""
    o, v = cc.o, cc.v
    s, d = np_lambda.unique(o, v)
    items = [(-cc.D1[i, a], i + o * a, ("s", i, a)) for i, a in s]
    items += [(-cc.D2[i, j, a, b], o * v + i + o * (j + o * (a + v * b)), ("d", i, j, a, b)) for i, j, a, b in d]
    items.sort(key=lambda x: (x[0], x[1]))
    return [x[2] for x in items]


def unit_vector(o, v, key):
    x1, x2 = np.zeros((o, v)), np.zeros((o, o, v, v))
    if key[0] == "s":
        x1[key[1], key[2]] = 1.0
    else:
        _, i, j, a, b = key
        x2[i, j, a, b] = x2[j, i, b, a] = 1.0
        x2[j, i, a, b] = x2[i, j, b, a] = -1.0
    return x1, x2


def sort_roots(w):
    """order by real part, ties by index"""
    return sorted(range(len(w)), key=lambda k: (w[k].real, k))


def davidson(sigma, D1, D2, guesses, nroots, tol=1e-8, max_space=None, maxiter=100):
    """Block Davidson for the lowest nroots eigenvalues of the non-symmetric A.  sigma(r1, r2) -> (s1, s2); vectors are held as packed
    unique amplitudes, where the (1, 1/4) inner product is the plain dot product.
    -> (omega, [packed Ritz vectors], dict(iterations, nsigma, collapses, resnorm))"""
    o, v = D1.shape
    pk, up = np_lambda.pack, lambda x: np_lambda.unpack(x, o, v)
    Dp = pk(D1, D2)
    max_space = max_space if max_space is not None else max(2 * nroots, min(len(Dp), 8 * nroots))
    B, S = [], []
    pending = [pk(*g) for g in guesses]
    nsigma = collapses = 0

    def orthonormalise(x, basis):
        for _ in range(2):
            for b in basis:
                x = x - np.dot(b, x) * b
        nrm = np.sqrt(np.dot(x, x))
        return None if nrm < DROP else x / nrm

    for it in range(1, maxiter + 1):
        if len(B) + len(pending) > max_space:                  # collapse: restart from the Ritz vectors, sigma by the same combination
            nb, ns = [], []
            Y = np.array(B).T @ yk
            SY = np.array(S).T @ yk
            # orthonormalise the Ritz vectors (Gram-Schmidt as a triangular transformation, applied to both)
            for k in range(Y.shape[1]):
                x, sx = Y[:, k].copy(), SY[:, k].copy()
                for _ in range(2):
                    for b, sb in zip(nb, ns):
                        c = np.dot(b, x)
                        x, sx = x - c * b, sx - c * sb
                nrm = np.sqrt(np.dot(x, x))
                if nrm >= DROP:
                    nb.append(x / nrm)
                    ns.append(sx / nrm)
            B, S = nb, ns
            collapses += 1
        for x in pending:
            x = orthonormalise(x, B)
            if x is None:
                continue
            s1, s2 = sigma(*up(x))
            nsigma += 1
            B.append(x)
            S.append(pk(s1, s2))
        Bm, Sm = np.array(B).T, np.array(S).T
        w, y = np.linalg.eig(Bm.T @ Sm)
        order = sort_roots(w)[:nroots]
        omega, yk = w[order].real, y[:, order].real
        X = Bm @ yk
        nx = np.sqrt(np.sum(X * X, axis=0))
        yk, X = yk / nx, X / nx
        R = Sm @ yk - X * omega
        res = np.sqrt(np.sum(R * R, axis=0))
        if np.all(res < tol):
            return omega, [X[:, k] for k in range(nroots)], dict(iterations=it, nsigma=nsigma, collapses=collapses, resnorm=res)
        pending = []
        for k in range(nroots):
            if res[k] >= tol:
                den = omega[k] + Dp
                den = np.where(np.abs(den) < CLAMP, np.where(den < 0.0, -CLAMP, CLAMP), den)
                pending.append(R[:, k] / den)
    raise RuntimeError("Davidson did not converge")


MODELS = {   # name: (n, nalpha, nbeta, seed, canonical) of np_lambda.model -- the eight lowest eigenvalues of A are real in all four
    "o4v6": (5, 2, 2, 1, False),
    "o3v7": (5, 2, 1, 2, False),
    "o4v6_canonical": (5, 2, 2, 4, True),
    "o4v8": (6, 2, 2, 5, False),
}
_CONVERGED = {}


def converged_model(name):
    """A model of MODELS at its converged amplitudes, made once: cc, t1, t2, the Jacobian A and its eigenvalues in Davidson's order"""
    if name not in _CONVERGED:
        import np_rocc
        n, na, nb, seed, canonical = MODELS[name]
        g, f, o, blocks = np_lambda.model(n, na, nb, seed, canonical=canonical)
        cc = np_rocc.ROCC(g, f, o)
        cc.solve(300, 1e-13, 1e-13)
        t1, t2 = cc.t1.copy(), cc.t2.copy()
        _, A = np_lambda.jacobian(cc, t1, t2)
        w = np.linalg.eigvals(A)
        w = w[sort_roots(w)]
        _CONVERGED[name] = dict(n=n, na=na, nb=nb, o=o, v=cc.v, cc=cc, t1=t1, t2=t2, A=A, w=w, blocks=blocks, g=g, f=f)
    return _CONVERGED[name]


def fci_two_electron_spectrum(h, chem):
    """every eigenvalue of the two-electron Hamiltonian over |p alpha, q beta> (Ms = 0: singlets and the Ms = 0 triplet components)"""
    n = h.shape[0]
    one = np.eye(n)
    Hm = (np.einsum("pr,qs->pqrs", h, one) + np.einsum("pr,qs->pqrs", one, h) + chem.transpose(0, 2, 1, 3)).reshape(n * n, n * n)
    return np.linalg.eigvalsh(Hm)
