"""Reference for EOM-CCSD linear response on the spin-orbital CCSD state (no GPU): the operator vector xi^X, the perturbed amplitudes
R^X(omega), the response function <<X;Y>>_omega and the shared-basis linear solver of the device code, rule by rule.

Conventions (np_lambda / np_eom / np_eom_left: the state's spin-orbital order, <x, y> = sum x1 y1 + 1/4 sum x2 y2 on full storage, the
plain dot product over the unique amplitudes).  X is a real symmetric one-body operator over the o + v spin orbitals, X-bar =
exp(-T) X_N exp(T):

    xi^X_mu          = <mu| X-bar |0> = residual(f + X) - residual(f) at fixed t (the residual is linear in f)
    (A - omega) R^X(omega) = -xi^X                       A = dR/dt, the matrix of np_eom.sigma_explicit
    <<X;Y>>_omega    = Phi[X, R^Y(omega)] + Phi[Y, R^X(-omega)]
    Phi[X, R]        = <0| (1 + Lambda) (X-bar - <X-bar>) R |0> = Tr(X gamma(1, lambda; 0, R)) - Tr(X D) <lambda, R>
    alpha_XY(omega)  = -<<X;Y>>_omega

with gamma np_eom_left.density_explicit and D np_lambda.density_explicit.  This is the EOM-CC response function of Stanton and Bartlett
(J. Chem. Phys. 99, 5178 (1993)), not the LR-CC one: the term quadratic in the perturbed amplitudes is absent by definition, and
alpha_XY(omega) != alpha_YX(omega) in general at omega != 0 (<<X;Y>>_omega = <<Y;X>>_-omega always).  For two electrons it is exact.

At the converged t and lambda, an eigenpair (omega_k, R_k) of A has r0_k = <0| H-bar R_k |0> / omega_k = -<lambda, R_k>, hence
Phi[X, R_k] = Tr(X gamma(1, lambda; r0_k, R_k)) = Tr(X gamma^0k): the sum over states

    <<X;Y>>_omega = -sum_k [ Tr(X gamma^0k) (L_k . xi^Y) / (omega_k - omega) + Tr(Y gamma^0k) (L_k . xi^X) / (omega_k + omega) ]

with L the rows of the inverse of the matrix of right eigenvectors.
"""
from __future__ import annotations

import numpy as np

import np_eom
import np_eom_left
import np_lambda
import np_rocc
from np_ucc import E

DROP, CLAMP, POLE = np_eom.DROP, np_eom.CLAMP, 1e-10


# ---------------------------------------------------------------------------------------------------------------- xi
def xi_definition(g, f, o, t1, t2, X):
    """residual(f + X) - residual(f) at fixed t, with no hand-derived term"""
    _, a1, a2 = np_lambda.residual(np_rocc.ROCC(g, f + X, o), t1, t2)
    _, b1, b2 = np_lambda.residual(np_rocc.ROCC(g, f, o), t1, t2)
    return a1 - b1, a2 - b2


def xi_explicit(t1, t2, X):
    """The form the device follows, with the same letters: the dressed X~_oo / X~_vv, xi1, and xi2 as two permuted products with t2"""
    o = t1.shape[0]
    Xoo, Xov, Xvv = X[:o, :o], X[:o, o:], X[o:, o:]
    Xtoo = Xoo + E("kc,jc->kj", Xov, t1)
    Xtvv = Xvv - E("kb,kc->bc", t1, Xov)
    xi1 = (Xov + E("ab,ib->ia", Xvv, t1) - E("ja,ji->ia", t1, Xoo) + E("jb,ijab->ia", Xov, t2)
           - E("jb,ib,ja->ia", Xov, t1, t1))
    pv = E("bc,ijac->ijab", Xtvv, t2)
    po = E("kj,ikab->ijab", Xtoo, t2)
    # each part is antisymmetric in its own pair by construction and in the other through t2, up to the order of its sums: the mean with
    # the exchanged image makes both exact (the device computes a unique element once and writes its four images)
    u, w = pv - pv.transpose(0, 1, 3, 2), po.transpose(1, 0, 2, 3) - po
    xi2 = 0.5 * (u - u.transpose(1, 0, 2, 3)) + 0.5 * (w - w.transpose(0, 1, 3, 2))
    return xi1, xi2


# ---------------------------------------------------------------------------------------------------------------- response
def phi(cc, t1, t2, lam, X, R, D=None):
    """Phi[X, R] = Tr(X gamma(1, lambda; 0, R)) - Tr(X D) <lambda, R>"""
    D = D if D is not None else np_lambda.density_explicit(cc, t1, t2, *lam)
    gam = np_eom_left.density_explicit(cc, t1, t2, 1.0, lam, 0.0, R)
    return float(np.sum(X * gam) - np.sum(X * D) * np_eom.dot(*lam, *R))


def solve_dense(A, o, v, xi, omega):
    """R(omega) = -(A - omega)^-1 xi over the unique amplitudes -> (r1, r2)"""
    x = np.linalg.solve(A - omega * np.eye(A.shape[0]), -np_lambda.pack(*xi))
    return np_lambda.unpack(x, o, v)


def response_dense(cc, t1, t2, lam, A, ops, omega):
    """<<X_a;X_b>>_omega for every pair of ops, by dense solves -> (nop, nop)"""
    o, v = cc.o, cc.v
    D = np_lambda.density_explicit(cc, t1, t2, *lam)
    xis = [xi_explicit(t1, t2, X) for X in ops]
    Rp = [solve_dense(A, o, v, xi, omega) for xi in xis]
    Rm = [solve_dense(A, o, v, xi, -omega) for xi in xis]
    return response_from_vectors(cc, t1, t2, lam, ops, Rp, Rm, D)


def response_from_vectors(cc, t1, t2, lam, ops, Rp, Rm, D=None):
    """the same from given R^X(+omega) / R^X(-omega) (the device's, for instance)"""
    D = D if D is not None else np_lambda.density_explicit(cc, t1, t2, *lam)
    n = len(ops)
    out = np.zeros((n, n))
    for a in range(n):
        for b in range(n):
            out[a, b] = phi(cc, t1, t2, lam, ops[a], Rp[b], D) + phi(cc, t1, t2, lam, ops[b], Rm[a], D)
    return out


def eigen_decomposition(A):
    """-> (w, V, L, residual): A V = V w with L = V^-1 (rows: biorthonormal left vectors) and the figure |A V - V w|_max"""
    w, V = np.linalg.eig(A)
    return w, V, np.linalg.inv(V), float(np.max(np.abs(A @ V - V * w)))


def response_sum_over_states(cc, t1, t2, lam, A, ops, omega, eig=None):
    """The sum over the eigenpairs of the dense Jacobian, at converged t and lambda (module docstring) -> (nop, nop)"""
    o, v = cc.o, cc.v
    w, V, L, _ = eig if eig is not None else eigen_decomposition(A)
    if np.max(np.abs(w.imag)) > 0.0:
        raise ValueError("the Jacobian has complex eigenvalues: pick another seed")
    w, V, L = w.real, V.real, L.real
    I = np_lambda.hbar(cc, t1, t2)
    xis = [np_lambda.pack(*xi_explicit(t1, t2, X)) for X in ops]
    n = len(ops)
    m = np.zeros((n, len(w)))
    for k in range(len(w)):
        Rk = np_lambda.unpack(V[:, k], o, v)
        r0 = np_eom_left.ref_coupling(cc, t1, t2, *Rk, I) / w[k]
        g0k = np_eom_left.density_explicit(cc, t1, t2, 1.0, lam, r0, Rk)
        for a in range(n):
            m[a, k] = np.sum(ops[a] * g0k)
    c = np.array([L @ x for x in xis])                                       # c[a, k] = L_k . xi^a
    out = np.zeros((n, n))
    for a in range(n):
        for b in range(n):
            out[a, b] = -np.sum(m[a] * c[b] / (w - omega)) - np.sum(m[b] * c[a] / (w + omega))
    return out


def fci_response(w, c, X, Y, omega):
    """<<X;Y>>_omega of the two-electron FCI states (np_eom_left.fci_two_electron_states) for spin-free symmetric n x n X, Y"""
    out = 0.0
    for k in range(1, len(w)):
        ta, tb = np_eom_left.fci_density(c[0], c[k])
        x, y, gap = float(np.sum(X * (ta + tb))), float(np.sum(Y * (ta + tb))), w[k] - w[0]
        out -= x * y / (gap - omega) + y * x / (gap + omega)
    return out


# ---------------------------------------------------------------------------------------------------------------- linear solver
class Pole(RuntimeError):
    """the projected system of a frequency is singular: omega is at a root of the projected matrix"""


def lu_solve(a, b, floor=0.0):
    """Partial-pivot LU of the small dense a, as the device's host code has it -> x, or None where a pivot is not above `floor`.  The
    solver passes POLE times the scale of the projected matrix and the shift, max(|G|_max, |omega|): omega is then within 1e-10
    (relative) of a root of G, closer than any tolerance the solver is run at can tell from the root itself."""
    a, b = np.array(a, dtype=float), np.array(b, dtype=float)
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


def linear_davidson(sigma, D1, D2, rhs, omegas, tol=1e-8, max_space=None, maxiter=100):
    """(A - omega_j) x_j = -xi_j for every system j = (rhs[j], omegas[j]) on ONE orthonormal basis B with S = A B: every pending correction
    costs one sigma build that serves every system.  The device's rules: the first pending vectors are the preconditioned right-hand
    sides xi_j / (omega_j + D), later ones the corrections rho_j / (omega_j + D) / |rho_j| (scaled: DROP is absolute), two projection
    passes, vectors below DROP are dropped, the denominator is clamped at CLAMP, and a full space collapses onto the current x_j.  -> ([packed x_j], dict(iterations, nsigma, collapses, resnorm)); raises Pole"""
    o, v = D1.shape
    pk, up = np_lambda.pack, lambda x: np_lambda.unpack(x, o, v)
    Dp = pk(D1, D2)
    xi = [pk(*r) for r in rhs]
    ns = len(xi)
    max_space = max_space if max_space is not None else max(2 * ns, min(len(Dp), 8 * ns))

    def precondition(r, om):
        den = om + Dp
        den = np.where(np.abs(den) < CLAMP, np.where(den < 0.0, -CLAMP, CLAMP), den)
        return r / den

    B, S = [], []
    pending = [precondition(xi[j], omegas[j]) for j in range(ns)]
    nsigma = collapses = 0
    X = SX = None
    for it in range(1, maxiter + 1):
        if len(B) + len(pending) > max_space:
            nb, nsg = [], []
            for k in range(ns):
                x, sx = X[:, k].copy(), SX[:, k].copy()
                for _ in range(2):
                    for b, sb in zip(nb, nsg):
                        c = np.dot(b, x)
                        x, sx = x - c * b, sx - c * sb
                nrm = np.sqrt(np.dot(x, x))
                if nrm >= DROP:
                    nb.append(x / nrm)
                    nsg.append(sx / nrm)
            B, S = nb, nsg
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
            S.append(pk(*sigma(*up(x))))
            nsigma += 1
        Bm, Sm = np.array(B).T, np.array(S).T
        G = Bm.T @ Sm
        Y = np.zeros((len(B), ns))
        for j in range(ns):
            y = lu_solve(G - omegas[j] * np.eye(len(B)), -(Bm.T @ xi[j]), POLE * max(float(np.max(np.abs(G))), abs(omegas[j])))
            if y is None:
                raise Pole(f"system {j}: omega = {omegas[j]} is at a root of the projected matrix")
            Y[:, j] = y
        X, SX = Bm @ Y, Sm @ Y
        rho = np.array(xi).T + SX - X * np.asarray(omegas)
        res = np.sqrt(np.sum(rho * rho, axis=0))
        if np.all(res < tol):
            return [X[:, j] for j in range(ns)], dict(iterations=it, nsigma=nsigma, collapses=collapses, resnorm=res)
        pending = [precondition(rho[:, j], omegas[j]) / res[j] for j in range(ns) if res[j] >= tol]
    raise RuntimeError("the linear Davidson iteration did not converge")
