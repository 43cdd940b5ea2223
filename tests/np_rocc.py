"""Dense numpy restatement of the non-HF spin-orbital path (restricted open-shell references): np_ucc.UCC with a full Fock matrix
(Stanton, Gauss, Watts, Bartlett 1991, Eqs. 1-5 with their f terms), the ROHF-CCSD(T) disconnected triples with f_ia t_jk^bc (Watts,
Gauss, Bartlett 1993), the ROHF-MBPT(2) energy, the two spin Fock operators of a restricted determinant and semicanonical orbitals.

Spin-orbital order, amplitudes and integrals as np_ucc's."""
from __future__ import annotations

import itertools

import numpy as np

import np_ucc
from np_ucc import E


def fock_ro(h, chem, na, nb):
    """F_a, F_b of the restricted determinant that fills the first na / nb orbitals; chem[p,q,r,s] = (pq|rs) over ONE orbital set."""
    def jk(o):
        return np.einsum("pqii->pq", chem[:, :, :o, :o]), np.einsum("piqi->pq", chem[:, :o, :, :o])
    (ja, ka), (jb, kb) = jk(na), jk(nb)
    return h + ja + jb - ka, h + ja + jb - kb


def e_ref_elec(h, fa, fb, na, nb):
    return 0.5 * float(np.trace((h + fa)[:na, :na])) + 0.5 * float(np.trace((h + fb)[:nb, :nb]))


def block_rotation(f, o):
    n = f.shape[0]
    u = np.zeros((n, n))
    for lo, hi in ((0, o), (o, n)):
        if hi > lo:
            _, vec = np.linalg.eigh(0.5 * (f[lo:hi, lo:hi] + f[lo:hi, lo:hi].T))
            for c in range(hi - lo):
                if vec[np.argmax(np.abs(vec[:, c])), c] < 0.0:
                    vec[:, c] = -vec[:, c]
            u[lo:hi, lo:hi] = vec.T
    return u


def semicanonical(fa, fb, na, nb):
    """-> (u_a, u_b, fa', fb'), u[new, old]; the occupied and the virtual block of every f' are diagonal"""
    res = []
    for f, o in ((fa, na), (fb, nb)):
        n = f.shape[0]
        u = block_rotation(f, o)
        g = u @ f @ u.T
        g = 0.5 * (g + g.T)
        for lo, hi in ((0, o), (o, n)):
            g[lo:hi, lo:hi] = np.diag(np.diag(g)[lo:hi].copy())
        res.append((u, g))
    return res[0][0], res[1][0], res[0][1], res[1][1]


def so_fock(fa, fb, na, nb):
    """The spin-orbital Fock matrix in the engine's order (zero between the spins)."""
    n = fa.shape[0]
    orb, spin = np_ucc.so_order(n, na, nb)
    f = np.where(spin[:, None] == spin[None, :], np.where(spin[:, None] == 0, fa[np.ix_(orb, orb)], fb[np.ix_(orb, orb)]), 0.0)
    return f


class ROCC(np_ucc.UCC):
    """Spin-orbital CCSD with a full Fock matrix f (all spin orbitals, occupied first): the levels are its diagonal."""

    def __init__(self, g, f, o):
        super().__init__(g, np.diag(f).copy(), o)
        self.f_ov = f[:o, o:].copy()
        self.f_oo = f[:o, :o] - np.diag(np.diag(f)[:o])
        self.f_vv = f[o:, o:] - np.diag(np.diag(f)[o:])
        self.t1 = self.f_ov / self.D1

    def e_mp2(self):
        return float(np.sum(self.f_ov ** 2 / self.D1) + 0.25 * np.sum(self.oovv ** 2 / self.D2))

    def energy_step(self):
        e, r = super().energy_step()
        self.energy = e + float(np.sum(self.f_ov * self.t1))
        return self.energy, r

    def intermediates(self):
        I = super().intermediates()
        t1 = self.t1
        I["F_vv"] = I["F_vv"] + self.f_vv - 0.5 * E("me,ma->ae", self.f_ov, t1)
        I["F_oo"] = I["F_oo"] + self.f_oo + 0.5 * E("ie,me->mi", t1, self.f_ov)
        I["F_ov"] = I["F_ov"] + self.f_ov
        return I

    def iterate(self):
        super().iterate()                       # (r1 without f_ia) / D1
        self.t1 = self.t1 + self.f_ov / self.D1

    def triples(self):
        o, t1, t2, eo, ev, f = self.o, self.t1, self.t2, self.eo, self.ev, self.f_ov
        vovv, ovoo, vvoo = self.vovv, self.ovoo, self.vvoo
        dv = ev[:, None, None] + ev[None, :, None] + ev[None, None, :]

        def P(x):
            return x - x.transpose(1, 0, 2) - x.transpose(2, 1, 0)
        e_t = 0.0
        for i, j, k in itertools.combinations(range(o), 3):
            wc = (E("fbc,af->abc", vovv[:, i], t2[j, k]) - E("fbc,af->abc", vovv[:, j], t2[i, k])
                  - E("fbc,af->abc", vovv[:, k], t2[j, i])
                  - E("mcb,ma->abc", t2[:, i], ovoo[:, :, j, k]) + E("mcb,ma->abc", t2[:, j], ovoo[:, :, i, k])
                  + E("mcb,ma->abc", t2[:, k], ovoo[:, :, j, i]))
            wd = (t1[i][:, None, None] * vvoo[:, :, j, k][None] - t1[j][:, None, None] * vvoo[:, :, i, k][None]
                  - t1[k][:, None, None] * vvoo[:, :, j, i][None]
                  + f[i][:, None, None] * t2[j, k][None] - f[j][:, None, None] * t2[i, k][None] - f[k][:, None, None] * t2[j, i][None])
            d = eo[i] + eo[j] + eo[k] - dv
            c = P(wc)
            e_t += np.sum(c * (c / d + P(wd) / d)) / 6.0
        return float(e_t)


def rocc_from_blocks(aa, ab, bb, fa, fb, na, nb):
    """ROCC over the three chemist blocks (np_ucc.mo_blocks) and the spin Fock matrices of the same orbitals"""
    g, _, o = np_ucc.so_integrals(aa, ab, bb, np.diag(fa).copy(), np.diag(fb).copy(), na, nb)
    return ROCC(g, so_fock(fa, fb, na, nb), o)


def random_orthogonal(rng, m, size):
    """exp of a random antisymmetric matrix of the given norm scale (m x m)"""
    if m == 0:
        return np.zeros((0, 0))
    k = rng.standard_normal((m, m))
    k = size * (k - k.T)
    w, v = np.linalg.eigh(1j * k)            # k = -i (i k): exp(k) = v exp(-i w) v^H
    return np.real(v @ np.diag(np.exp(-1j * w)) @ v.conj().T)


def block_diag(a, b):
    n = a.shape[0] + b.shape[0]
    u = np.zeros((n, n))
    u[:a.shape[0], :a.shape[0]] = a
    u[a.shape[0]:, a.shape[0]:] = b
    return u


def triplet_rotation(n, angle):
    """The occupied-virtual rotation of the two-electron triplet case: orbital 0 with 2 by `angle`, orbital 1 with 3 by -angle / 2.
    With angle = 0.05 the H2O(8+) triplet has max |f_ov| above 1 Eh and the restatement converges well within 60 iterations (both
    asserted in test_rohf_cpu.py)."""
    k = np.zeros((n, n))
    k[0, 2], k[2, 0], k[1, 3], k[3, 1] = angle, -angle, -0.5 * angle, 0.5 * angle
    w, v = np.linalg.eigh(1j * k)
    return np.real(v @ np.diag(np.exp(-1j * w)) @ v.conj().T)


def invariance_rotations(n, na, nb, seed=7, size=1e-3):
    """One occupied-occupied and one virtual-virtual rotation per spin.  With seed 7 and size 1e-3 the off-diagonal Fock elements of H2O+
    exceed 1e-2 Eh (occupied) and 1e-3 Eh (virtual), and np_ucc.UCC.solve with 20 DIIS vectors converges to 1e-11 within 60
    iterations (asserted in test_rohf_cpu.py); with its default 8 vectors it needs more than 60."""
    rng = np.random.default_rng(seed)
    ra = block_diag(random_orthogonal(rng, na, size), random_orthogonal(rng, n - na, size))
    rb = block_diag(random_orthogonal(rng, nb, size), random_orthogonal(rng, n - nb, size))
    return ra, rb
