"""Reference for EOM-CCSD linear response at complex frequencies z = omega + i gamma (no GPU): dense complex solves, the
response function, the FCI sum over states and the complex linear mode of the block Davidson unit, rule by rule.

Conventions are those of np_response.  A and xi are real, R = P + i Q:

    (A - z) R^X(z) = -xi^X      <=>      (A - omega) P + gamma Q = -xi,   (A - omega) Q - gamma P = 0
    <<X;Y>>_z      = Phi[X, R^Y(z)] + Phi[Y, R^X(-z)],     Phi[X, P + i Q] = Phi[X, P] + i Phi[X, Q]     (Phi is linear in R)
    alpha_XY(z)    = -<<X;Y>>_z,        R(conj z) = conj R(z)

the analytic continuation of np_response's function; np_response itself is untouched.
"""
from __future__ import annotations

import numpy as np

import np_eom
import np_eom_left
import np_lambda
import np_response

DROP, CLAMP, POLE = np_response.DROP, np_response.CLAMP, np_response.POLE
Pole = np_response.Pole


# ---------------------------------------------------------------------------------------------------------------- response
def solve_dense(A, o, v, xi, z):
    """R(z) = -(A - z)^-1 xi over the unique amplitudes -> (r1, r2), complex"""
    x = np.linalg.solve(A - complex(z) * np.eye(A.shape[0]), -np_lambda.pack(*xi).astype(complex))
    p, q = np_lambda.unpack(x.real.copy(), o, v), np_lambda.unpack(x.imag.copy(), o, v)
    return p[0] + 1j * q[0], p[1] + 1j * q[1]


def phi(cc, t1, t2, lam, X, R, D=None):
    """Phi[X, P + i Q] = Phi[X, P] + i Phi[X, Q]"""
    D = D if D is not None else np_lambda.density_explicit(cc, t1, t2, *lam)
    re = np_response.phi(cc, t1, t2, lam, X, (R[0].real.copy(), R[1].real.copy()), D)
    im = np_response.phi(cc, t1, t2, lam, X, (R[0].imag.copy(), R[1].imag.copy()), D)
    return complex(re, im)


def response_from_vectors(cc, t1, t2, lam, ops, Rp, Rm, D=None):
    """<<X_a;X_b>>_z from given R^X(z) and R^X(-z) -> complex (nop, nop)"""
    D = D if D is not None else np_lambda.density_explicit(cc, t1, t2, *lam)
    n = len(ops)
    out = np.zeros((n, n), dtype=complex)
    for a in range(n):
        for b in range(n):
            out[a, b] = phi(cc, t1, t2, lam, ops[a], Rp[b], D) + phi(cc, t1, t2, lam, ops[b], Rm[a], D)
    return out


def response_dense(cc, t1, t2, lam, A, ops, z):
    """<<X_a;X_b>>_z for every pair of ops, by dense complex solves at z and at -z -> complex (nop, nop)"""
    o, v = cc.o, cc.v
    xis = [np_response.xi_explicit(t1, t2, X) for X in ops]
    Rp = [solve_dense(A, o, v, xi, z) for xi in xis]
    Rm = [solve_dense(A, o, v, xi, -complex(z)) for xi in xis]
    return response_from_vectors(cc, t1, t2, lam, ops, Rp, Rm)


def fci_response(w, c, X, Y, z):
    """np_response.fci_response with a complex frequency: <<X;Y>>_z of the two-electron FCI states"""
    z = complex(z)
    out = 0.0j
    for k in range(1, len(w)):
        ta, tb = np_eom_left.fci_density(c[0], c[k])
        x, y, gap = float(np.sum(X * (ta + tb))), float(np.sum(Y * (ta + tb))), w[k] - w[0]
        out -= x * y / (gap - z) + y * x / (gap + z)
    return out


def fci_strengths(w, c, ops):
    """(gaps omega_k, f_k) with alpha-bar(z) = sum_k f_k / (omega_k^2 - z^2): f_k = (2 omega_k / 3) sum_X <0|X|k>^2 over the three
    operators `ops` (spin-free, symmetric)"""
    gaps, f = [], []
    for k in range(1, len(w)):
        ta, tb = np_eom_left.fci_density(c[0], c[k])
        gaps.append(w[k] - w[0])
        f.append(2.0 * (w[k] - w[0]) / 3.0 * sum(float(np.sum(X * (ta + tb))) ** 2 for X in ops))
    return np.array(gaps), np.array(f)


def c6_closed_form(gaps, f):
    """C6 = (3 / 2) sum_kl f_k f_l / (omega_k omega_l (omega_k + omega_l)) of alpha-bar(iu) = sum_k f_k / (omega_k^2 + u^2), from
    int_0^inf du / ((a^2 + u^2)(b^2 + u^2)) = pi / (2 a b (a + b))"""
    g, h = np.meshgrid(gaps, gaps, indexing="ij")
    return float(1.5 * np.sum(np.outer(f, f) / (g * h * (g + h))))


# ---------------------------------------------------------------------------------------------------------------- linear solver
def lu_solve_complex(a, b, floor=0.0):
    """np_response.lu_solve for a complex matrix, as the device's host code has it: pivoting on |pivot| -> x, or None where |pivot| is
    not above `floor`"""
    a, b = np.array(a, dtype=complex), np.array(b, dtype=complex)
    n = a.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if not abs(a[p, k]) > floor:
            return None
        if p != k:
            a[[k, p]] = a[[p, k]]
            b[[k, p]] = b[[p, k]]
        for i in range(k + 1, n):
            l = a[i, k] / a[k, k]
            a[i, k:] -= l * a[k, k:]
            b[i] -= l * b[k]
    for k in range(n - 1, -1, -1):
        b[k] = (b[k] - np.dot(a[k, k + 1:], b[k + 1:])) / a[k, k]
    return b


def cden(z, diag):
    """the guarded denominator z - diag: inside CLAMP of zero it is the real +-CLAMP with the sign of its real part (+ for zero)"""
    den = complex(z) - np.asarray(diag, dtype=float)
    small = np.abs(den) < CLAMP
    return np.where(small, np.where(den.real < 0.0, -CLAMP, CLAMP) + 0.0j, den)


class ComplexLinear:
    """The complex linear mode of the block Davidson unit (csrc/davidson_so.h) on whole vectors: (A - z_j) x_j = -rhs[j % nrhs] with
    `apply` the real matrix, `diag` the preconditioner diagonal and the metric <x, y> = sum w x y.  One real orthonormal basis B with
    S = A B.  The rules: the first pending vectors are Re and Im of rhs_j / (z_j - diag), in that order per system; two projection passes,
    vectors below DROP are dropped (the exactly zero imaginary vectors of a system with gamma_j = 0 among them); (G - z_j) y_j = -B^T W
    rhs_j by complex LU, Pole where |pivot| <= POLE max(|G|_max, |z_j|); x = B y, rho = rhs + S y - z x; the next pending vectors are Re
    and Im of rho_j / (z_j - diag) / |rho_j| of the systems with |rho_j| >= tol; a full space collapses onto Re x_j, Im x_j of every
    system, in that order, with S x carried."""

    def __init__(self, apply, diag, w, rhs, zs, max_space):
        self.apply, self.diag, self.w = apply, np.asarray(diag, dtype=float), np.asarray(w, dtype=float)
        self.rhs = np.asarray(rhs, dtype=float)                              # (nvec, nrhs)
        self.z = np.asarray(zs, dtype=complex)
        self.ns, self.ms = len(self.z), max_space
        assert 4 * self.ns <= max_space and self.rhs.shape[1] <= self.ns
        self.B, self.S = [], []
        self.nsigma = self.ncollapse = self.dropped = 0
        self.pend = []
        for j in range(self.ns):
            p = self.rhs[:, j % self.rhs.shape[1]] / cden(self.z[j], self.diag)
            self.pend += [p.real.copy(), p.imag.copy()]
        self.x = self.sx = None
        self.resnorm = np.full(self.ns, np.inf)

    def counts(self):
        return dict(nsigma=self.nsigma, ncollapse=self.ncollapse, nb=len(self.B), npend=len(self.pend))

    def _orthonormalise(self, x, sx=None):
        w = self.w
        if self.B:
            Bm = np.array(self.B).T
            Sm = np.array(self.S).T
            for _ in range(2):
                c = (Bm * w[:, None]).T @ x
                x = x - Bm @ c
                if sx is not None:
                    sx = sx - Sm @ c
        nrm = np.sqrt(np.sum(w * x * x))
        if not nrm >= DROP:
            self.dropped += 1
            return None
        return x / nrm, (None if sx is None else sx / nrm)

    def step(self, tol):
        """-> converged; raises Pole"""
        ns, w = self.ns, self.w
        if len(self.B) + len(self.pend) > self.ms:
            cols = [(c.copy(), sc.copy()) for j in range(ns) for c, sc in ((self.x[:, j].real, self.sx[:, j].real), (self.x[:, j].imag, self.sx[:, j].imag))]
            self.B, self.S = [], []
            for x, sx in cols:
                got = self._orthonormalise(x, sx)
                if got is not None:
                    self.B.append(got[0])
                    self.S.append(got[1])
            self.ncollapse += 1
        for x in self.pend:
            if len(self.B) >= self.ms:
                break
            got = self._orthonormalise(x)
            if got is None:
                continue
            self.B.append(got[0])
            self.S.append(self.apply(got[0]))
            self.nsigma += 1
        self.pend = []
        if not self.B:
            raise RuntimeError("every right-hand side vanished")
        Bm, Sm = np.array(self.B).T, np.array(self.S).T
        G = (Bm * w[:, None]).T @ Sm
        prhs = (Bm * w[:, None]).T @ self.rhs
        nb = Bm.shape[1]
        Y = np.zeros((nb, ns), dtype=complex)
        for j in range(ns):
            y = lu_solve_complex(G - self.z[j] * np.eye(nb), -prhs[:, j % self.rhs.shape[1]], POLE * max(float(np.max(np.abs(G))), abs(self.z[j])))
            if y is None:
                raise Pole(f"system {j}: z = {self.z[j]} is at a root of the projected matrix")
            Y[:, j] = y
        self.y = Y
        self.x, self.sx = Bm @ Y, Sm @ Y
        rho = self.rhs[:, np.arange(ns) % self.rhs.shape[1]] + self.sx - self.x * self.z[None, :]
        self.rho = rho
        self.resnorm = np.sqrt(np.sum(w[:, None] * (rho.real ** 2 + rho.imag ** 2), axis=0))
        self.corr = np.stack([rho[:, j] / cden(self.z[j], self.diag) for j in range(ns)], axis=1)
        for j in range(ns):
            if not self.resnorm[j] < tol:
                c = self.corr[:, j] / self.resnorm[j]
                self.pend += [c.real.copy(), c.imag.copy()]
        return not self.pend


def linear_davidson_complex(sigma, D1, D2, rhs, zs, tol=1e-8, max_space=None, maxiter=100):
    """np_response.linear_davidson at complex shifts: (A - z_j) x_j = -xi_j for every system j = (rhs[j], zs[j]) over the unique amplitudes
    (the plain dot product), by ComplexLinear.  -> ([packed complex x_j], dict(iterations, nsigma, collapses, resnorm, dropped)); raises Pole"""
    o, v = D1.shape
    pk, up = np_lambda.pack, lambda x: np_lambda.unpack(x, o, v)
    Dp = pk(D1, D2)
    xi = np.array([pk(*r) for r in rhs]).T
    ns = xi.shape[1]
    max_space = max_space if max_space is not None else max(4 * ns, min(len(Dp) + 2 * ns, 16 * ns))
    st = ComplexLinear(lambda x: pk(*sigma(*up(x))), -Dp, np.ones(len(Dp)), xi, zs, max_space)
    for it in range(1, maxiter + 1):
        if st.step(tol):
            return [st.x[:, j] for j in range(ns)], dict(iterations=it, nsigma=st.nsigma, collapses=st.ncollapse, resnorm=st.resnorm,
                                                         dropped=st.dropped)
    raise RuntimeError("the complex linear Davidson iteration did not converge")
