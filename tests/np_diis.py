"""update_diis_cc (src/ccsd.f90:617-676) in plain numpy: the reference of the DIIS tests.  Test infrastructure only.

A ring of nerr slots holds amplitude vectors t_k and error vectors e_k = t_k - s (s: the amplitudes at the top of the iteration,
ccsd.f90:342-343).  The overlaps B_ij = e_i . e_j are accumulated in np.longdouble, [B -1; -1 0] c = (0,...,0,-1) is solved in
np.longdouble by Gaussian elimination with partial pivoting, and the new amplitudes are sum_k c_k t_k.  eliminate_f64 is the same
elimination in binary64 with multipliers formed by DIVISION (the engine's host solver, csrc/ccsd.hip diis_update, and the oracle's
orc_linsolve): it returns None when a pivot is exactly zero, which is what `singular` means in the tests."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

Step = namedtuple("Step", "t c cond c64 n slot tmax")
# t     sum_k c_k t_k as float64 (None when the longdouble elimination meets a zero pivot)
# c     the n coefficients (longdouble), cond: numpy.linalg.cond of the augmented (n+1) x (n+1) matrix
# c64   coefficients of the binary64 elimination by division, None when it meets a pivot that is exactly zero
# n     active vectors, slot: the ring slot (0-based) this push wrote, tmax: max |t_k| over the active history vectors


def augmented(B):
    """[B -1; -1 0] and the right-hand side (0,...,0,-1) (ccsd.f90:653-656)."""
    n = B.shape[0]
    A = np.zeros((n + 1, n + 1), dtype=B.dtype)
    A[:n, :n] = B
    A[n, :n] = A[:n, n] = -1
    rhs = np.zeros(n + 1, dtype=B.dtype)
    rhs[n] = -1
    return A, rhs


def _eliminate(A, rhs):
    """Gaussian elimination with partial pivoting in the dtype of A, multipliers by division; None at a pivot that is exactly zero."""
    A = A.copy()
    b = rhs.copy()
    N = A.shape[0]
    for k in range(N):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if A[p, k] == 0:
            return None
        if p != k:
            A[[k, p]] = A[[p, k]]
            b[[k, p]] = b[[p, k]]
        for i in range(k + 1, N):
            f = A[i, k] / A[k, k]
            A[i, k:] = A[i, k:] - f * A[k, k:]
            b[i] = b[i] - f * b[k]
    x = np.zeros(N, dtype=A.dtype)
    for k in range(N - 1, -1, -1):
        x[k] = (b[k] - np.dot(A[k, k + 1:], x[k + 1:])) / A[k, k]
    return x


def eliminate_f64(B):
    """The n DIIS coefficients of the overlap matrix B from the binary64 elimination, or None (singular)."""
    A, rhs = augmented(np.asarray(B, dtype=np.float64))
    x = _eliminate(A, rhs)
    return None if x is None else x[:-1]


def eliminate_ld(B):
    A, rhs = augmented(np.asarray(B, dtype=LD))
    x = _eliminate(A, rhs)
    return None if x is None else x[:-1]


def flat(t1, t2):
    """[t1 ; t2] as one vector in the engine's (column-major) order."""
    return np.concatenate([np.asarray(t1).ravel(order="F"), np.asarray(t2).ravel(order="F")])


def unflat(x, o, v):
    return x[:o * v].reshape((o, v), order="F"), x[o * v:].reshape((o, o, v, v), order="F")


class Diis:
    def __init__(self, nerr):
        self.nerr, self.nact, self.it = int(nerr), 0, 0
        self.t = [None] * self.nerr
        self.e = [None] * self.nerr
        self.B = np.zeros((self.nerr, self.nerr), dtype=LD)

    def push(self, t, s) -> Step:
        """One update_diis_cc with the current amplitudes t and the saved ones s (flat float64 vectors)."""
        t = np.asarray(t, dtype=np.float64)
        if self.nerr < 2:   # ccsd.f90:593-595: DIIS switched off
            return Step(t.copy(), None, 1.0, None, 0, 0, float(np.max(np.abs(t))))
        self.it += 1
        if self.it > self.nerr:
            self.it -= self.nerr
        if self.nact < self.nerr:
            self.nact += 1
        slot, n = self.it - 1, self.nact
        self.t[slot] = t.copy()
        self.e[slot] = t - np.asarray(s, dtype=np.float64)   # (the subtraction the engine does, in binary64)
        el = self.e[slot].astype(LD)
        for j in range(n):
            self.B[slot, j] = self.B[j, slot] = np.dot(el, self.e[j].astype(LD))
        B = self.B[:n, :n]
        A64, _ = augmented(B.astype(np.float64))
        cond = float(np.linalg.cond(A64))
        c = eliminate_ld(B)
        c64 = eliminate_f64(B)
        tn = None
        if c is not None:
            acc = np.zeros(t.size, dtype=LD)
            for k in range(n):
                acc += c[k] * self.t[k].astype(LD)
            tn = acc.astype(np.float64)
        tmax = max(float(np.max(np.abs(self.t[k]))) for k in range(n))
        return Step(tn, c, cond, c64, n, slot, tmax)


def tolerance(step: Step) -> float:
    """64 eps cond max|t| (t: the history vectors that are combined): the factor covers another elimination order."""
    return 64.0 * EPS * step.cond * step.tmax


# ---- inputs of the injection tests (tests/test_gpu_diis.py; their conditioning is pinned without a GPU in tests/test_diis_cpu.py)
INJECT_NERR = (2, 3, 4, 5, 7, 8, 9, 12, 15)
SPATIAL_EXTENTS = ((3, 5), (7, 21))          # (o, v): 240 elements (less than one block) and 21756 (no multiple of 256)
SPINORB_EXTENTS = ((6, 4), (9, 6))           # (n, nel) of init_cc_spinorb: (o, v) = (4, 8) and (6, 12)


def perturbations(kind, o, v, count, seed):
    """`count` seeded random vectors d_k as (t1, t2) with the solver's own symmetry -- kind "spatial": t2(i,j,a,b) = t2(j,i,b,a),
    kind "spinorb": t2 antisymmetric in ij and in ab -- and norms 1e-2 * 2^u, u uniform in [-1, 1]: spread over a factor of 4
    around 1e-2, so that random directions in >= 100 dimensions give a well conditioned overlap matrix."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        t1 = rng.standard_normal((o, v))
        t2 = rng.standard_normal((o, o, v, v))
        if kind == "spatial":
            t2 = t2 + t2.transpose(1, 0, 3, 2)
        else:
            t2 = t2 - t2.transpose(1, 0, 2, 3)
            t2 = t2 - t2.transpose(0, 1, 3, 2)
        nrm = np.sqrt(np.sum(t1 * t1) + np.sum(t2 * t2))
        f = 1e-2 * 2.0 ** rng.uniform(-1.0, 1.0) / nrm
        out.append((t1 * f, t2 * f))
    return out


def duplicate_vector(o, v):
    """(t1, t2) with exactly 49 entries equal to 1.0 and the rest 0: t1 entries first, then t2(i,i,a,a), which both symmetries of
    `perturbations` map to themselves resp. leave at zero -- so spin-orbital extents need o v >= 49."""
    t1 = np.zeros((o, v))
    t2 = np.zeros((o, o, v, v))
    left = 49
    for a in range(v):
        for i in range(o):
            if left:
                t1[i, a] = 1.0
                left -= 1
    for a in range(v):
        for i in range(o):
            if left:
                t2[i, i, a, a] = 1.0
                left -= 1
    assert left == 0
    return t1, t2


def dyadic(x):
    """x rounded to multiples of 2^-40: for |x| < 1 the sums x + 1 and the differences (x + 1) - x are then exact in binary64."""
    return np.round(np.asarray(x) * 2.0 ** 40) / 2.0 ** 40
