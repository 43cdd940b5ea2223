"""Reference for EOM-IP-CCSD and EOM-EA-CCSD on the spin-orbital CCSD state (no GPU).

IP sector (1h + 2h1p): r1(i), r2(i,j,a) antisymmetric in i,j.  EA sector (1p + 2p1h): r1(a), r2(i,a,b) antisymmetric in a,b.  On full
storage <x, y> = sum x1 y1 + 1/2 sum x2 y2; the unique amplitudes are i, then (i < j, a) / a, then (i, a < b).  Two forms of sigma:

  * ip_sigma_definition / ea_sigma_definition, with no hand-derived term: EOM-EE (np_eom.sigma_definition, the complex step) into a
    ghost orbital g that interacts with nothing -- every integral and Fock element of g zero, its level included.  IP: g is one more
    virtual, r1'[i,g] = r_i, r2'[i,j,a,g] = -r2'[i,j,g,a] = r_ija.  EA: g is one more occupied, the last one, r1'[g,a] = r_a,
    r2'[i,g,a,b] = -r2'[g,i,a,b] = r_iab.  sigma is read from the same components; every component without g vanishes identically
    (the `leak` the functions return);
  * ip_sigma_explicit / ea_sigma_explicit: term by term over the H-bar elements of np_lambda.hbar -- the form the device code follows,
    with the same intermediates and the same letters.

davidson() is the block Davidson iteration of the device code, rule by rule, on packed vectors (where the inner product is the plain
dot product); np_eom.davidson packs with the EE sector's own layout and cannot serve here.
"""
from __future__ import annotations

import itertools

import numpy as np

import np_eom
import np_lambda
import np_rocc
from np_ucc import E

IP, EA = 1, 2
DROP, CLAMP = np_eom.DROP, np_eom.CLAMP


def levels(cc):
    return np.asarray(cc.eo, dtype=float), np.asarray(cc.ev, dtype=float)


def shapes(sector, o, v):
    return ((o,), (o, o, v)) if sector == IP else ((v,), (o, v, v))


def random_vector(rng, sector, o, v, size=0.3):
    s1, s2 = shapes(sector, o, v)
    r1, r2 = rng.uniform(-size, size, s1), rng.uniform(-size, size, s2)
    r2 = 0.5 * (r2 - (r2.transpose(1, 0, 2) if sector == IP else r2.transpose(0, 2, 1)))
    return r1, r2


def dot(x1, x2, y1, y2):
    return float(np.sum(x1 * y1) + 0.5 * np.sum(x2 * y2))


# ---------------------------------------------------------------------------------------------------------------- definition
def _ghost(cc_g, cc_f, o, at):
    """g and f with one more spin orbital at index `at`, all of whose elements are zero"""
    g = cc_g
    for ax in range(4):
        g = np.insert(g, at, 0.0, axis=ax)
    f = np.insert(np.insert(cc_f, at, 0.0, axis=0), at, 0.0, axis=1)
    return g, f


def ip_sigma_definition(g, f, o, t1, t2, r1, r2):
    """-> (sigma1 (o), sigma2 (o,o,v), leak: the largest |component without g| of the enlarged sigma)"""
    n = f.shape[0]
    v = n - o
    gg, fg = _ghost(g, f, o, n)
    cc = np_rocc.ROCC(gg, fg, o)
    T1, T2 = np.zeros((o, v + 1), t1.dtype), np.zeros((o, o, v + 1, v + 1), t2.dtype)
    T1[:, :v], T2[:, :, :v, :v] = t1, t2
    R1, R2 = np.zeros((o, v + 1)), np.zeros((o, o, v + 1, v + 1))
    R1[:, v] = r1
    R2[:, :, :v, v] = r2
    R2[:, :, v, :v] = -r2
    S1, S2 = np_eom.sigma_definition(cc, T1, T2, R1, R2)
    leak = max(np.max(np.abs(S1[:, :v])), np.max(np.abs(S2[:, :, :v, :v])), np.max(np.abs(S2[:, :, v, v])))
    return S1[:, v].copy(), S2[:, :, :v, v].copy(), float(leak)


def ea_sigma_definition(g, f, o, t1, t2, r1, r2):
    """-> (sigma1 (v), sigma2 (o,v,v), leak)"""
    n = f.shape[0]
    v = n - o
    gg, fg = _ghost(g, f, o, o)
    cc = np_rocc.ROCC(gg, fg, o + 1)
    T1, T2 = np.zeros((o + 1, v), t1.dtype), np.zeros((o + 1, o + 1, v, v), t2.dtype)
    T1[:o], T2[:o, :o] = t1, t2
    R1, R2 = np.zeros((o + 1, v)), np.zeros((o + 1, o + 1, v, v))
    R1[o] = r1
    R2[:o, o] = r2
    R2[o, :o] = -r2
    S1, S2 = np_eom.sigma_definition(cc, T1, T2, R1, R2)
    leak = max(np.max(np.abs(S1[:o])), np.max(np.abs(S2[:o, :o])), np.max(np.abs(S2[o, o])))
    return S1[o].copy(), S2[:o, o].copy(), float(leak)


def sigma_definition(sector, g, f, o, t1, t2, r1, r2):
    return (ip_sigma_definition if sector == IP else ea_sigma_definition)(g, f, o, t1, t2, r1, r2)


# ---------------------------------------------------------------------------------------------------------------- explicit
def ip_sigma_explicit(cc, t1, t2, r1, r2, I=None):
    I = I if I is not None else np_lambda.hbar(cc, t1, t2)
    eo, ev = levels(cc)
    Hov, Hoo, Hvv = I["Hov"], I["Hoo"], I["Hvv"]
    s1 = -E("mi,m->i", Hoo, r1) - E("me,ime->i", Hov, r2) + 0.5 * E("mnie,mne->i", I["Hooov"], r2) - eo * r1
    y = 0.5 * E("mnef,mnf->e", cc.oovv, r2)
    W = (0.5 * E("mnij,mna->ija", I["Hoooo"], r2) + E("ae,ije->ija", Hvv, r2) + E("maij,m->ija", I["Hovoo"], r1)
         + E("e,ijae->ija", y, t2))
    A = E("maej,ime->ija", I["Hovvo"], r2) - E("mj,ima->ija", Hoo, r2)
    d = eo[:, None, None] + eo[None, :, None] - ev[None, None, :]
    return s1, W + A - A.transpose(1, 0, 2) - d * r2


def ea_sigma_explicit(cc, t1, t2, r1, r2, I=None):
    I = I if I is not None else np_lambda.hbar(cc, t1, t2)
    eo, ev = levels(cc)
    Hov, Hoo, Hvv = I["Hov"], I["Hoo"], I["Hvv"]
    s1 = E("ae,e->a", Hvv, r1) - E("me,mae->a", Hov, r2) - 0.5 * E("amef,mef->a", I["Hvovv"], r2) + ev * r1
    y = 0.5 * E("mnef,nef->m", cc.oovv, r2)
    Z = 0.5 * E("ief,amef->iam", r2, cc.vovv)
    Q = E("ief,mnef->imn", r2, cc.oovv)
    W = (0.5 * E("abef,ief->iab", cc.vvvv, r2) + 0.25 * E("imn,mnab->iab", Q, I["tau"]) + E("m,imab->iab", y, t2)
         - E("mi,mab->iab", Hoo, r2) - E("ieab,e->iab", I["Hvvvo"], r1))
    B = -E("mb,iam->iab", t1, Z) + E("mbei,mae->iab", I["Hovvo"], r2) + E("be,iae->iab", Hvv, r2)
    d = eo[:, None, None] - ev[None, :, None] - ev[None, None, :]
    return s1, W + B - B.transpose(0, 2, 1) - d * r2


def sigma_explicit(sector, cc, t1, t2, r1, r2, I=None):
    return (ip_sigma_explicit if sector == IP else ea_sigma_explicit)(cc, t1, t2, r1, r2, I)


def diagonal(sector, cc):
    """the diagonal guess of the sector's matrix (what the device keeps resident): -> (d1, d2) on full storage"""
    eo, ev = levels(cc)
    if sector == IP:
        return -eo, -(eo[:, None, None] + eo[None, :, None] - ev[None, None, :])
    return ev.copy(), -(eo[:, None, None] - ev[None, :, None] - ev[None, None, :])


# ---------------------------------------------------------------------------------------------------------------- packing
def unique(sector, o, v):
    """[(p,)] and [(i, j, a) with i < j] / [(i, a, b) with a < b]"""
    if sector == IP:
        return [(i,) for i in range(o)], [(i, j, a) for i, j in itertools.combinations(range(o), 2) for a in range(v)]
    return [(a,) for a in range(v)], [(i, a, b) for i in range(o) for a, b in itertools.combinations(range(v), 2)]


def _image(sector, k):
    return (k[1], k[0], k[2]) if sector == IP else (k[0], k[2], k[1])


def pack(sector, x1, x2):
    o, v = (x2.shape[0], x2.shape[2])
    s, d = unique(sector, o, v)
    return np.array([x1[k] for k in s] + [x2[k] for k in d], dtype=np.result_type(x1, x2))


def unpack(sector, x, o, v):
    s, d = unique(sector, o, v)
    s1, s2 = shapes(sector, o, v)
    x1, x2 = np.zeros(s1, x.dtype), np.zeros(s2, x.dtype)
    for k, p in enumerate(s):
        x1[p] = x[k]
    for k, p in enumerate(d):
        x2[p] = x[len(s) + k]
        x2[_image(sector, p)] = -x[len(s) + k]
    return x1, x2


def guess_order(sector, cc):
    """the unique amplitudes by ascending diagonal, ties by flat index in the device's (Fortran) storage order -> list of index tuples
    (length 1: a single; length 3: a double)"""
    o, v = cc.o, cc.v
    d1, d2 = diagonal(sector, cc)
    s, d = unique(sector, o, v)
    n1 = len(s)
    if sector == IP:
        flat = lambda k: n1 + k[0] + o * (k[1] + o * k[2])
    else:
        flat = lambda k: n1 + k[0] + o * (k[1] + v * k[2])
    items = [(d1[k], k[0], k) for k in s] + [(d2[k], flat(k), k) for k in d]
    items.sort(key=lambda x: (x[0], x[1]))
    return [x[2] for x in items]


def unit_vector(sector, o, v, key):
    s1, s2 = shapes(sector, o, v)
    x1, x2 = np.zeros(s1), np.zeros(s2)
    if len(key) == 1:
        x1[key] = 1.0
    else:
        x2[key] = 1.0
        x2[_image(sector, key)] = -1.0
    return x1, x2


SEED, PHI = 1e-3, 0.6180339887498949


def seed_vector(sector, o, v):
    """what every guess of the device carries beside its unit vector: SEED (frac((q + 1) PHI) - 1/2) on every unique amplitude, q the
    smaller flat index of its two images in the device's (Fortran) storage, the other image with the opposite sign"""
    s1, s2 = shapes(sector, o, v)
    n1, y = s1[0], np.arange(int(np.prod(s2)), dtype=np.int64)
    if sector == IP:
        z = (y // o) % o + o * (y % o + (y // (o * o)) * o)
    else:
        z = y % o + o * (y // (o * v) + v * ((y // o) % v))
    frac = lambda q: (q + 1) * PHI - np.floor((q + 1) * PHI) - 0.5
    sign = np.where(z == y, 0.0, np.where(y < z, 1.0, -1.0))
    return SEED * frac(np.arange(n1, dtype=np.int64).astype(float)), (SEED * sign * frac((n1 + np.minimum(y, z)).astype(float))).reshape(s2, order="F")


def guess_vector(sector, o, v, key):
    """a guess of the device: the unit vector on `key` plus seed_vector -- sigma couples neither Ms blocks nor irreducible
    representations, and a unit vector alone sees one block of each"""
    x1, x2 = unit_vector(sector, o, v, key)
    y1, y2 = seed_vector(sector, o, v)
    return x1 + y1, x2 + y2


def matrix(sector, cc, t1, t2, I=None):
    """the sector's matrix over the unique amplitudes, column by column from sigma_explicit of the unit vectors"""
    o, v = cc.o, cc.v
    I = I if I is not None else np_lambda.hbar(cc, t1, t2)
    s, d = unique(sector, o, v)
    n = len(s) + len(d)
    A = np.zeros((n, n))
    for nu in range(n):
        e = np.zeros(n)
        e[nu] = 1.0
        A[:, nu] = pack(sector, *sigma_explicit(sector, cc, t1, t2, *unpack(sector, e, o, v), I))
    return A


# ---------------------------------------------------------------------------------------------------------------- Davidson
def davidson(sigma, Dp, guesses, nroots, tol=1e-8, max_space=None, maxiter=100):
    """np_eom.davidson on packed vectors: sigma(x) -> packed sigma, Dp the packed diagonal of the matrix (the correction is
    rho / (omega - Dp)), guesses packed.  -> (omega, [packed Ritz vectors], dict(iterations, nsigma, collapses, resnorm))"""
    max_space = max_space if max_space is not None else max(2 * nroots, min(len(Dp), 8 * nroots))
    B, S = [], []
    pending = [np.asarray(g, dtype=float) for g in guesses]
    nsigma = collapses = 0
    yk = None
    for it in range(1, maxiter + 1):
        if len(B) + len(pending) > max_space:
            nb, ns = [], []
            Y, SY = np.array(B).T @ yk, np.array(S).T @ yk
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
            if len(B) >= max_space:
                break
            for _ in range(2):
                for b in B:
                    x = x - np.dot(b, x) * b
            nrm = np.sqrt(np.dot(x, x))
            if nrm < DROP:
                continue
            x = x / nrm
            B.append(x)
            S.append(sigma(x))
            nsigma += 1
        Bm, Sm = np.array(B).T, np.array(S).T
        w, y = np.linalg.eig(Bm.T @ Sm)
        order = np_eom.sort_roots(w)[:nroots]
        omega, yk = w[order].real, y[:, order].real
        X = Bm @ yk
        nx = np.sqrt(np.sum(X * X, axis=0))
        yk, X = yk / nx, X / nx
        R = Sm @ yk - X * omega
        res = np.sqrt(np.sum(R * R, axis=0))
        if len(order) == nroots and np.all(res < tol):
            return omega, [X[:, k] for k in range(nroots)], dict(iterations=it, nsigma=nsigma, collapses=collapses, resnorm=res)
        pending = []
        for k in range(len(order)):
            if res[k] >= tol:
                den = omega[k] - Dp
                den = np.where(np.abs(den) < CLAMP, np.where(den < 0.0, -CLAMP, CLAMP), den)
                pending.append(R[:, k] / den)
    raise RuntimeError("Davidson did not converge")


_SECTOR = {}


def converged_sector(name, sector):
    """np_eom.converged_model(name) with the sector's matrix and its eigenvalues in Davidson's order, made once"""
    if (name, sector) not in _SECTOR:
        c = np_eom.converged_model(name)
        A = matrix(sector, c["cc"], c["t1"], c["t2"])
        w = np.linalg.eigvals(A)
        _SECTOR[name, sector] = dict(c, A=A, w=w[np_eom.sort_roots(w)])
    return _SECTOR[name, sector]


def davidson_case(name, sector, nroots):
    """what the Davidson tests (CPU and GPU) run on a model of np_eom.MODELS: -> (max_space, collapses)
    max_space is four vectors per root, at most every unique amplitude; `collapses` says whether the space is too small for the iteration to
    end before it restarts from the Ritz vectors (the one case where it is not: IP at o3v7 with 6 roots, 24 unique amplitudes)."""
    n, na, nb, _, _ = np_eom.MODELS[name]
    o, v = na + nb, 2 * n - na - nb
    nunique = len(unique(sector, o, v)[0]) + len(unique(sector, o, v)[1])
    return min(4 * nroots, nunique), 4 * nroots < nunique
