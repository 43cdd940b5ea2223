"""Reference for the left-hand side of EOM-EE-CCSD on the spin-orbital CCSD state (no GPU): the left sigma build, and the one-particle
density as a bilinear form of a left and a right vector.

Left sigma.  sigma_L(l) = A^T l in the unique basis, with A = dR/dt of np_lambda.jacobian and np_eom's metric.  Two forms:

  * lsigma_definition: A^T pack(l), with no hand-derived term;
  * lsigma_explicit: lambda_rhs_explicit(l) - lambda_rhs_explicit(0) - D l -- the Lambda iteration's X without its two inhomogeneous
    terms and without the division: the form the device code follows.

Density.  With a left pair (l0, l) and a right pair (r0, r)

    F(f) = l0 r0 E(t) + l0 dE(t).r + r0 <l, R(t)> + <l, sigma(r)> + E(t) <l, r> + sum_ijab l_ijab r_ia R1_jb
    D_pq = 1/2 (dF/df_pq + dF/df_qp)

is <0| (l0 + L) H-bar (r0 + R) |0> differentiated by the Fock matrix (its diagonal included, as in np_lambda.density); the last term is
the disconnected <L2| R1 H-bar |0>.  Two forms:

  * density_definition: central difference in f over np_rocc.ROCC(g, f +- x, o), as np_lambda.density (exact to rounding: F is linear in f);
  * density_explicit: the form the device follows, with the same letters.  Every f in F sits in E (f_me t_me) or in R, and sigma(r) is
    the derivative of R along r, so with P(t, l) = d<l, R(t)>/df -- np_lambda.density_explicit without its lone t_me --
        D = (l0 r0 + <l, r>) [t_me]  +  l0 [r_me]  +  P(t, (r0 l1 + y, r0 l2))  +  dP(t, l)/dt . r,      y_jb = sum_ia l_ijab r_ia
    where y carries the disconnected term (it multiplies R1 as a lambda_1 does).

The cases above the library: ground state (1, lambda; 1, 0), excited state k (0, L_k; r0_k, R_k) with <L_k, R_k> = 1, gamma^0k
(1, lambda; r0_k, R_k), gamma^k0 (0, L_k; 1, 0); r0_k = (sum H_ia r_ia + 1/4 sum <ij||ab> r_ijab) / omega_k (ref_coupling).
"""
from __future__ import annotations

import numpy as np

import np_eom
import np_lambda
import np_rocc
from np_ucc import E


# ---------------------------------------------------------------------------------------------------------------- left sigma
def lsigma_definition(cc, t1, t2, l1, l2, A=None):
    A = A if A is not None else np_lambda.jacobian(cc, t1, t2)[1]
    return np_lambda.unpack(A.T @ np_lambda.pack(l1, l2), cc.o, cc.v)


def lsigma_explicit(cc, t1, t2, l1, l2, I=None):
    I = I if I is not None else np_lambda.hbar(cc, t1, t2)
    x1, x2 = np_lambda.lambda_rhs_explicit(cc, t1, t2, l1, l2, I)
    z1, z2 = np_lambda.lambda_rhs_explicit(cc, t1, t2, 0.0 * l1, 0.0 * l2, I)
    return x1 - z1 - cc.D1 * l1, x2 - z2 - cc.D2 * l2


def ref_coupling(cc, t1, t2, r1, r2, I=None):
    """<0| H-bar R |0> = sum H_ia r_ia + 1/4 sum <ij||ab> r_ijab (= dE.r); r0 = this / omega"""
    I = I if I is not None else np_lambda.hbar(cc, t1, t2)
    return float(np.sum(I["Hov"] * r1) + 0.25 * np.sum(cc.oovv * r2))


# ---------------------------------------------------------------------------------------------------------------- density
def _zero(cc):
    return np.zeros((cc.o, cc.v)), np.zeros((cc.o, cc.o, cc.v, cc.v))


def F(cc, t1, t2, l0, l, r0, r):
    """The bilinear form at the Fock matrix cc was made with.  l, r: (x1, x2) or None (zero)"""
    l1, l2 = l if l is not None else _zero(cc)
    r1, r2 = r if r is not None else _zero(cc)
    h = np_lambda.H
    e, R1, R2 = np_lambda.residual(cc, t1 + 1j * h * r1, t2 + 1j * h * r2)     # real parts: E, R; imaginary parts / h: dE.r, sigma(r)
    dEr, s1, s2 = e.imag / h, R1.imag / h, R2.imag / h
    e, R1, R2 = e.real, R1.real, R2.real
    return float(l0 * r0 * e + l0 * dEr + r0 * np_eom.dot(l1, l2, R1, R2) + np_eom.dot(l1, l2, s1, s2) + e * np_eom.dot(l1, l2, r1, r2)
                 + E("ijab,ia,jb->", l2, r1, R1))


def density_definition(g, f, o, t1, t2, l0, l, r0, r, eps=2.0 ** -6):
    n = f.shape[0]
    d = np.zeros((n, n))
    for p in range(n):
        for q in range(p + 1):
            x = np.zeros((n, n))
            x[p, q] += eps
            x[q, p] += eps
            fp = F(np_rocc.ROCC(g, f + x, o), t1, t2, l0, l, r0, r)
            fm = F(np_rocc.ROCC(g, f - x, o), t1, t2, l0, l, r0, r)
            d[p, q] = d[q, p] = 0.5 * (fp - fm) / (2.0 * eps)
    return d


def density_explicit(cc, t1, t2, l0, l, r0, r):
    """Block by block as the device builds it:
      w [t_me]                  the lone t_me term, w = l0 r0 + <l, r>
      l0 [r_me]                 l0 . r1 in the ov block
      the lambda part           np_lambda's formulas with lambda -> (L1, r0 l2), L1 = r0 l1 + y -- y_jb = l_ijab r_ia: the disconnected term
      the sigma part            oo and vv blocks from l1.r1 and l2.r2 (GooR, GvvR), and ov-block chains through t1 / t2"""
    o, v = cc.o, cc.v
    l1, l2 = l if l is not None else _zero(cc)
    r1, r2 = r if r is not None else _zero(cc)
    w = l0 * r0 + np_eom.dot(l1, l2, r1, r2)
    GvvT, GooT = -0.5 * E("mnef,mnaf->ae", t2, l2), 0.5 * E("mnef,inef->mi", t2, l2)
    GvvR, GooR = -0.5 * E("mnef,mnaf->ae", r2, l2), 0.5 * E("mnef,inef->mi", r2, l2)
    y = E("ijab,ia->jb", l2, r1)
    L1 = r0 * l1 + y
    doo = -E("ia,ma->mi", L1, t1) - E("ia,ma->mi", l1, r1) - r0 * GooT - GooR
    dvv = E("ia,ie->ae", L1, t1) + E("ia,ie->ae", l1, r1) - r0 * GvvT - GvvR
    dvvT = E("ia,ie->ae", l1, t1) - GvvT                                  # (what r1 meets: the vv block of the lambda part at r0 = 1, y = 0)
    dov =(w * t1 + l0 * r1 + L1 + E("ia,imae->me", L1, t2) + E("ia,imae->me", l1, r2)
           - E("mb,be->me", t1, dvv) - E("mb,be->me", r1, dvvT)
           - r0 * E("mj,je->me", GooT, t1) - E("mj,je->me", GooR, t1) - E("mj,je->me", GooT, r1))
    d = np.zeros((o + v, o + v))
    d[:o, :o] = 0.5 * (doo + doo.T)
    d[o:, o:] = 0.5 * (dvv + dvv.T)
    d[:o, o:] = 0.5 * dov
    d[o:, :o] = 0.5 * dov.T
    return d


# ---------------------------------------------------------------------------------------------------------------- FCI, two electrons
def fci_two_electron_states(h, chem):
    """-> (energies ascending, [c_k (n,n)] over |p alpha, q beta>): c symmetric for a singlet, antisymmetric for the Ms = 0 triplet component"""
    n = h.shape[0]
    one = np.eye(n)
    Hm = (np.einsum("pr,qs->pqrs", h, one) + np.einsum("pr,qs->pqrs", one, h) + chem.transpose(0, 2, 1, 3)).reshape(n * n, n * n)
    w, vec = np.linalg.eigh(Hm)
    return w, [vec[:, k].reshape(n, n) for k in range(n * n)]


def fci_is_singlet(c):
    return bool(np.linalg.norm(c - c.T) < 1e-6 * np.linalg.norm(c))


def fci_density(ck, cl=None):
    """the symmetrised alpha and beta (transition) density matrices <k| p+ q |l> (l = k by default)"""
    cl = ck if cl is None else cl
    a, b = ck @ cl.T, ck.T @ cl
    return 0.5 * (a + a.T), 0.5 * (b + b.T)


def so_matrix(ma, mb, orb, spin):
    """a spin-diagonal operator (alpha and beta n x n matrices) over spin orbitals in a state's order (afesp_amd.density.so_spin_order)"""
    out = np.where(spin[:, None] == 0, ma[np.ix_(orb, orb)], mb[np.ix_(orb, orb)])
    return out * (spin[:, None] == spin[None, :])
