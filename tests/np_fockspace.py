"""Occupation-number-basis toolkit: second-quantised operators applied literally to state vectors of length 2^n.  Test infrastructure only.

Spin orbital p is bit p of a basis state's index; the first o spin orbitals are occupied in the reference |0>.  Creation and annihilation
carry the Jordan-Wigner sign (-1)^(number of occupied spin orbitals below p).  No matrices: every operator is a function on vectors.

    H  = sum h(p,q) p+ q + 1/4 sum <pq||rs> p+ q+ s r,     h = f - sum_i <pi||qi>
    T2 = 1/4 sum t(ijab) a+ b+ j i,   R1 = sum r(l,d) d+ l,   R2 as T2,   L1 = sum l(ia) i+ a,   L2 = 1/4 sum l(ijab) i+ j+ b a

Used by test_eom_t_cpu.py at n <= 10 spin orbitals as the oracle of np_eom_t.py:
    m(mu3) = <mu3| [H, R2] + [[H, R1], T2] |0>,     l(mu3) = <0| (L1 + L2) H |mu3>,     |mu3> = a+ b+ c+ k j i |0>  (i<j<k, a<b<c)
"""
from __future__ import annotations

import itertools

import numpy as np


class Fock:
    def __init__(self, n, o):
        self.n, self.o, self.dim = n, o, 1 << n
        idx = np.arange(self.dim)
        self.free, self.sign = [], []
        for p in range(n):
            below = np.zeros(self.dim, dtype=np.int64)
            for q in range(p):
                below += (idx >> q) & 1
            self.free.append(((idx >> p) & 1) == 0)
            self.sign.append(1.0 - 2.0 * (below & 1))
        self.idx = idx

    def vac(self):
        x = np.zeros(self.dim)
        x[(1 << self.o) - 1] = 1.0
        return x

    def cre(self, p, x):
        out = np.zeros_like(x)
        src = self.idx[self.free[p]]
        out[src | (1 << p)] = self.sign[p][src] * x[src]
        return out

    def ann(self, p, x):
        out = np.zeros_like(x)
        src = self.idx[~self.free[p]]
        out[src & ~(1 << p)] = self.sign[p][src] * x[src]
        return out

    def one_body(self, h, x):
        """sum h(p,q) p+ q x"""
        out = np.zeros_like(x)
        for q in range(self.n):
            y = self.ann(q, x)
            if not y.any():
                continue
            for p in range(self.n):
                if h[p, q] != 0.0:
                    out += h[p, q] * self.cre(p, y)
        return out

    def two_body(self, g, x):
        """1/4 sum <pq||rs> p+ q+ s r x = sum_{p<q, r<s} <pq||rs> p+ q+ s r x for an antisymmetrised g"""
        out = np.zeros_like(x)
        for r, s in itertools.combinations(range(self.n), 2):
            y = self.ann(s, self.ann(r, x))
            if not y.any():
                continue
            for p, q in itertools.combinations(range(self.n), 2):
                if g[p, q, r, s] != 0.0:
                    out += g[p, q, r, s] * self.cre(p, self.cre(q, y))
        return out

    def hamiltonian(self, f, g):
        o = self.o
        h = f - np.einsum("piqi->pq", g[:, :o, :, :o])
        return lambda x: self.one_body(h, x) + self.two_body(g, x)

    # excitation (up=True: a+ i, a+ b+ j i) and de-excitation (i+ a, i+ j+ b a) operators of amplitudes laid out as t1 / t2
    def singles(self, x1, up=True):
        n, o = self.n, self.o
        h = np.zeros((n, n))
        if up:
            h[o:, :o] = x1.T
        else:
            h[:o, o:] = x1
        return lambda x: self.one_body(h, x)

    def doubles(self, x2, up=True):
        n, o = self.n, self.o
        g = np.zeros((n, n, n, n))
        if up:
            g[o:, o:, :o, :o] = x2.transpose(2, 3, 0, 1)
        else:
            g[:o, :o, o:, o:] = x2
        return lambda x: self.two_body(g, x)

    def triples(self):
        """[(i,j,k), (a,b,c) (virtual counts from 0), |mu3>] over i<j<k, a<b<c"""
        o, v = self.o, self.n - self.o
        out = []
        for i, j, k in itertools.combinations(range(o), 3):
            for a, b, c in itertools.combinations(range(v), 3):
                x = self.ann(i, self.vac())
                x = self.ann(j, x)
                x = self.ann(k, x)
                x = self.cre(o + c, x)
                x = self.cre(o + b, x)
                x = self.cre(o + a, x)
                out.append(((i, j, k), (a, b, c), x))
        return out


def eom_t_numerators(f, g, o, t2, l1, l2, r1, r2):
    """-> (m[i,j,k,a,b,c], l[i,j,k,a,b,c]) filled at i<j<k, a<b<c, from the operator definitions in the module text"""
    n = f.shape[0]
    v = n - o
    F = Fock(n, o)
    H = F.hamiltonian(f, g)
    T2, R1, R2 = F.doubles(t2), F.singles(r1), F.doubles(r2)
    L1d, L2d = F.singles(l1), F.doubles(l2)     # (L1)^+ and (L2)^+: H is symmetric, so <0| L H |mu3> = <mu3| H L^+ |0>
    vac = F.vac()
    h0 = H(vac)
    right = H(R2(vac)) - R2(h0)
    # [[H, R1], T2] = H R1 T2 - R1 H T2 - T2 H R1 + T2 R1 H
    right += H(R1(T2(vac))) - R1(H(T2(vac))) - T2(H(R1(vac))) + T2(R1(h0))
    left = H(L1d(vac) + L2d(vac))
    m = np.zeros((o, o, o, v, v, v))
    ell = np.zeros_like(m)
    for (i, j, k), (a, b, c), x in F.triples():
        m[i, j, k, a, b, c] = x @ right
        ell[i, j, k, a, b, c] = x @ left
    return m, ell


def fci_spectrum(f, g, o, nroots=None):
    """eigenvalues of H in the o-electron sector (dense; n <= 10 spin orbitals)"""
    n = f.shape[0]
    F = Fock(n, o)
    H = F.hamiltonian(f, g)
    dets = [d for d in range(F.dim) if bin(d).count("1") == o]
    mat = np.zeros((len(dets), len(dets)))
    for c, d in enumerate(dets):
        x = np.zeros(F.dim)
        x[d] = 1.0
        mat[:, c] = H(x)[dets]
    w = np.linalg.eigvalsh(0.5 * (mat + mat.T))
    return w if nroots is None else w[:nroots]
