"""The block Davidson unit (csrc/davidson_so.hip) restated rule by rule in numpy, for both of its modes and any metric, on matrices given as
data: A = diag(d) + U V^T.  Generalised from np_eom.davidson and np_response.linear_davidson (which stay as they are).

Three layers:
  * `Operator` and the seeded generators of the test matrices (`generate`, `dense_operator`, `rotation_block_matrix`);
  * `Restatement`: the iteration step by step in float64 with the unit's rules -- what tests/test_davidson_cpu.py holds to dense
    numpy.linalg.eig / solve and what tests/test_gpu_davidson.py takes the counts of every step from;
  * the one-step evaluators in numpy.longdouble (`ld_*`): each takes what the device held before an operation and returns what the operation
    must give, with a majorant M per returned element -- the same expression over absolute values, with the propagated part of a few-stage
    operation added (derivations at each function) -- so that |device - reference| <= (L + 64) 2^-53 M, L being the rounded additions on the
    element's path (the form of np_triples.tol_factor).

The unit's rules (davidson_so.hip):
  metric      <x, y> = sum_{e < n1} x y + w2 sum_{e >= n1} x y
  projection  two passes of classical Gram-Schmidt against the stored columns: all coefficients of a pass from the vector as the pass finds
              it, then x -= sum_p c_p b_p; then x / |x|.  |x| < DROP = 1e-10 (or NaN): the vector is dropped
  collapse    when nb + npend > max_space: the basis becomes the orthonormalised Ritz vectors (linear mode: the solutions) x_k, and their
              sigma the same combination of the stored sigma
  roots       eigenvalues of G = B^T W S ordered by real part (a complex pair adjacent, wi > 0 first); the lowest nr = min(nroots, nb),
              or, for a following state started from the caller's guesses, at each later step with nb > nr the root nearest to each
              target (the Ritz values of the guess step) in the targets' order, each root once, then in ascending order
  complex     flag 2; omega is the real part; the vector is the real part of the vector of the pair's wi > 0 member, scaled to sum y^2 = 1
  correction  rho / (omega - diag), |omega - diag| < CLAMP = 1e-4 replaced by +-CLAMP with its sign; only roots with |rho| >= tol
  linear      pending_j = rhs_(j % nrhs) / (shift_j - diag); (G - shift_j) y_j = -B^T W rhs_j by partial-pivot LU with a pole where a pivot is
              not above POLE max(|G|_max, |shift_j|); rho_j = rhs_j + (S - shift_j B) y_j; corrections scaled by 1 / |rho_j|
"""
import numpy as np

DROP, CLAMP, POLE = 1e-10, 1e-4, 1e-10
EPS53 = 2.0 ** -53
FLAG_CONVERGED, FLAG_COMPLEX = 1, 2
LD = np.longdouble


class Pole(RuntimeError):
    """a shift is at a root of the projected matrix"""


class Vanished(RuntimeError):
    """every guess vector (right-hand side) vanished"""


def tol_factor(L):
    """|device - reference| <= tol_factor(L) * M: L rounded additions on the element's path, each within 2^-53 of the running majorant; 64
    for the reduction tree over lanes, waves and blocks, the products, a division or square root.  Not tuned to any kernel."""
    return (L + 64) * EPS53


def weights(n1, nvec, w2):
    w = np.full(nvec, float(w2))
    w[:n1] = 1.0
    return w


# ---------------------------------------------------------------------------------------------------------------- the matrices
class Operator:
    """A = diag(d) + U V^T (U, V: (nvec, r), or None); `diag` is the preconditioner diagonal"""

    def __init__(self, d, U=None, V=None, diag=None):
        self.d = np.asarray(d, dtype=float)
        self.nvec = self.d.size
        self.U = None if U is None else np.asarray(U, dtype=float)
        self.V = None if V is None else np.asarray(V, dtype=float)
        self.r = 0 if U is None else self.U.shape[1]
        self.diag = self.d.copy() if diag is None else np.asarray(diag, dtype=float)

    def apply(self, x):
        s = self.d * x
        return s if self.r == 0 else s + self.U @ (self.V.T @ x)

    def dense(self):
        a = np.diag(self.d)
        return a if self.r == 0 else a + self.U @ self.V.T


NLOW = 24   # the lowest diagonal elements of a generated matrix are 0.5, 0.6, ... (well separated); the rest lie in [3.2, 4]


def generate(nvec, r=4, seed=0, coupling=0.2):
    """The seeded test matrix: d spread over [0.5, 4] -- its lowest min(NLOW, nvec) values 0.5 + 0.1 k at scattered places, the lowest at the LAST
    element and the next at the first, so that the lowest vectors have an entry of unit magnitude where a lost tail would show -- and
    U, V with normal entries of size coupling / sqrt(nvec) (|U V^T|_2 ~ coupling^2: real, well separated lowest roots).  U != V: not symmetric.
    -> (Operator, places of the ascending lowest diagonal elements)"""
    rng = np.random.default_rng(1000003 * seed + nvec)
    nlow = min(NLOW, nvec)
    d = 3.2 + 0.8 * rng.random(nvec)
    rest = rng.permutation(np.arange(1, nvec - 1))[:max(nlow - 2, 0)] if nvec > 2 else np.zeros(0, dtype=int)
    places = np.concatenate([[nvec - 1], [0] if nvec > 1 else [], rest]).astype(int)[:nlow]
    d[places] = 0.5 + 0.1 * np.arange(places.size)
    U = V = None
    if r:
        U = coupling / np.sqrt(nvec) * rng.standard_normal((nvec, r))
        V = coupling / np.sqrt(nvec) * rng.standard_normal((nvec, r))
        U[places[:4], 0] += 0.15          # (a coupling among the lowest vectors that does not fade with nvec)
        V[places[:4], 0] += 0.1
    return Operator(d, U, V), places


def dense_operator(a, diag=None):
    """a dense m x m matrix as d = 0, U = A, V = 1"""
    a = np.asarray(a, dtype=float)
    return Operator(np.zeros(a.shape[0]), a, np.eye(a.shape[0]), np.diag(a).copy() if diag is None else diag)


def rotation_block_matrix(m=24, seed=0, a=0.3, b=0.2, coupling=0.05):
    """A dense m x m matrix whose two lowest roots are the complex pair ~ a +- i b of a 2 x 2 rotation block, below a real rest spread over
    [1, 4], with a small non-symmetric coupling all over"""
    rng = np.random.default_rng(77 + seed)
    A = np.diag(np.concatenate([[a, a], np.linspace(1.0, 4.0, m - 2)]))
    A[0, 1], A[1, 0] = b, -b
    return A + coupling * rng.standard_normal((m, m)) / np.sqrt(m)


def unit_guesses(nvec, places, k):
    g = np.zeros((nvec, k))
    g[places[:k], np.arange(k)] = 1.0
    return g


# ---------------------------------------------------------------------------------------------------------------- host rules
def numpy_eig(g):
    """numpy.linalg.eig in the unit's order: by real part, ties by LAPACK's order (a pair adjacent, wi > 0 first) -> (wr, wi, vectors as the
    unit stores them: a real root's column; a pair's real part under its wi > 0 member and imaginary part under the other)"""
    w, v = np.linalg.eig(np.asarray(g, dtype=float))
    order = sorted(range(len(w)), key=lambda k: (w[k].real, k))
    w, v = w[order], v[:, order]
    vr = np.where(w.imag[None, :] < 0.0, -v.imag, v.real) if np.iscomplexobj(v) else v
    return w.real.copy(), (w.imag.copy() if np.iscomplexobj(w) else np.zeros(len(w))), np.asarray(vr, dtype=float)


def select_roots(wr, nr, target, guess_step):
    """-> the columns taken (ascending).  target: the list kept by a following state, or empty"""
    nb = len(wr)
    sel = list(range(nr))
    if not guess_step and len(target) and nb > nr:
        used, sel = [False] * nb, []
        nt = min(nr, len(target))
        for k in range(nr):
            best = -1
            for c in range(nb):
                if used[c]:
                    continue
                if best < 0 or (k < nt and abs(wr[c] - target[k]) < abs(wr[best] - target[k])):
                    best = c
            used[best] = True
            sel.append(best)
        sel.sort()
    return sel


def ritz_coefficients(wr, wi, vr, sel):
    """-> (y (nb, nr), omega, flags) of the columns `sel`"""
    nb = len(wr)
    y, om, fl = np.zeros((nb, len(sel))), np.zeros(len(sel)), np.zeros(len(sel), dtype=int)
    for k, c in enumerate(sel):
        col = vr[:, c - 1 if (wi[c] < 0.0 and c > 0) else c]
        n2 = 0.0
        for v in col:                     # (in the unit's order: one running sum)
            n2 += float(v) * float(v)
        y[:, k] = (1.0 / np.sqrt(n2) if n2 > 0.0 else 0.0) * col
        om[k] = wr[c]
        fl[k] = FLAG_COMPLEX if wi[c] != 0.0 else 0
    return y, om, fl


def lu_solve(a, b, floor=0.0):
    """partial-pivot LU as the unit's host code has it (np_response.lu_solve) -> x, or None at a pivot not above `floor`"""
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


def linear_coefficients(G, prhs, shifts):
    """y_j of (G - shift_j) y_j = -prhs_(j % nrhs) -> (nb, nsys); raises Pole"""
    nb, nrhs = prhs.shape
    gmax = float(np.max(np.abs(G))) if nb else 0.0
    Y = np.zeros((nb, len(shifts)))
    for j, om in enumerate(shifts):
        y = lu_solve(G - om * np.eye(nb), -prhs[:, j % nrhs], POLE * max(gmax, abs(om)))
        if y is None:
            raise Pole(f"system {j}: shift {om} is at a root of the projected matrix of {nb} vectors")
        Y[:, j] = y
    return Y


def clamp(den):
    return np.where(np.abs(den) < CLAMP, np.where(den < 0.0, -CLAMP, CLAMP), den)


def project_normalise(Bm, x, w, Sm=None, sx=None):
    """The unit's orthonormalisation of x (with its companion sx) against the columns of Bm (float64, or long double if the inputs are)
    -> (b, s) or None when the vector is dropped"""
    one = x.dtype.type(1.0)
    if Bm.shape[1]:
        for _ in range(2):
            c = (Bm * w[:, None]).T @ x
            x = x - Bm @ c
            if sx is not None:
                sx = sx - Sm @ c
    nrm = np.sqrt(np.sum(w * x * x))
    if not nrm >= DROP:
        return None
    sc = one / nrm
    return sc * x, (None if sx is None else sc * sx)


# ---------------------------------------------------------------------------------------------------------------- the iteration, float64
class Restatement:
    """One state of the unit.  B, S: lists of columns; pend: list of pending vectors; x, sx, corr: (nvec, nroots) of the last step."""

    def __init__(self, op, n1, w2, nroots, max_space, follow=False, eig=numpy_eig):
        assert nroots >= 1 and max_space >= 2 * nroots
        self.op, self.w = op, weights(n1, op.nvec, w2)
        self.nroots, self.ms, self.follow, self.eig = nroots, max_space, bool(follow), eig
        self.restart()
        self.linear = False
        self.user_guess = False

    def restart(self):
        self.B, self.S, self.pend = [], [], []
        self.G = np.zeros((0, 0))
        self.prhs = np.zeros((0, 0))
        self.target = []
        self.ritz = False
        self.nsigma = self.ncollapse = 0
        self.features = dict(clamp_pos=0, clamp_neg=0, dropped=0, complex=0, selected_not_lowest=0)

    @property
    def nb(self):
        return len(self.B)

    def counts(self):
        return dict(nsigma=self.nsigma, ncollapse=self.ncollapse, nb=self.nb, npend=len(self.pend))

    def set_guess(self, k, x):
        if self.nb > 0 or not self.user_guess:
            self.restart()
            self.pend = []
            self.user_guess = True
        while len(self.pend) <= k:
            self.pend.append(np.zeros(self.op.nvec))
        self.pend[k] = np.array(x, dtype=float)
        self.linear = False

    def _mat(self, cols):
        return np.array(cols).T if cols else np.zeros((self.op.nvec, 0))

    def _extend(self, b, s):
        self.B.append(b)
        self.S.append(s)
        Bm, Sm, w = self._mat(self.B), self._mat(self.S), self.w
        q = self.nb - 1
        G = np.zeros((q + 1, q + 1))
        G[:q, :q] = self.G
        G[:, q] = (Bm * w[:, None]).T @ s
        G[q, :q] = (Sm[:, :q] * w[:, None]).T @ b
        self.G = G
        if self.linear:
            self.prhs = np.vstack([self.prhs, ((self.rhs * w[:, None]).T @ b)[None, :]])

    def _basis_step(self, nkeep):
        """collapse where needed, then the pending vectors"""
        if self.nb + len(self.pend) > self.ms:
            xs, sxs = self.x[:, :nkeep].copy(), self.sx[:, :nkeep].copy()
            self.B, self.S, self.G = [], [], np.zeros((0, 0))
            if self.linear:
                self.prhs = np.zeros((0, self.rhs.shape[1]))
            for k in range(nkeep):
                got = project_normalise(self._mat(self.B), xs[:, k], self.w, self._mat(self.S), sxs[:, k])
                if got is None:
                    self.features["dropped"] += 1
                    continue
                self._extend(*got)
            self.ncollapse += 1
        for x in self.pend:
            if self.nb >= self.ms:
                break
            got = project_normalise(self._mat(self.B), x, self.w)
            if got is None:
                self.features["dropped"] += 1
                continue
            self.nsigma += 1
            self._extend(got[0], self.op.apply(got[0]))
        self.pend = []
        if self.nb == 0:
            raise Vanished("every guess vector vanished")

    def _ritz_pass(self, y, om, rhs_cols):
        """x, sx, rho, corr, resnorm of the coefficient columns y with the values om (and rho += rhs where given)"""
        Bm, Sm = self._mat(self.B), self._mat(self.S)
        nr = y.shape[1]
        self.x, self.sx = np.zeros((self.op.nvec, self.nroots)), np.zeros((self.op.nvec, self.nroots))
        self.corr = np.zeros((self.op.nvec, self.nroots))
        self.x[:, :nr], self.sx[:, :nr] = Bm @ y, Sm @ y
        rho = self.sx[:, :nr] - self.x[:, :nr] * om
        if rhs_cols is not None:
            rho = rhs_cols + rho
        den = om[None, :] - self.op.diag[:, None]
        self.features["clamp_pos"] += int(np.sum((np.abs(den) < CLAMP) & (den >= 0.0)))
        self.features["clamp_neg"] += int(np.sum((np.abs(den) < CLAMP) & (den < 0.0)))
        self.corr[:, :nr] = rho / clamp(den)
        self.rho = rho
        return np.sqrt(np.sum(self.w[:, None] * rho * rho, axis=0))

    def step(self, tol):
        """-> converged.  omega, resnorm, flags, sel are those of the step"""
        assert not self.linear
        if self.nb == 0 and not self.pend:
            raise RuntimeError("no guess vectors")
        guess_step = self.nb == 0
        self._basis_step(min(self.nroots, self.nb))
        nb, nr = self.nb, min(self.nroots, self.nb)
        wr, wi, vr = self.eig(self.G)
        if guess_step and self.follow and self.user_guess:
            self.target = list(wr[:nr])
        self.sel = select_roots(wr, nr, self.target, guess_step)
        if self.sel != list(range(nr)):
            self.features["selected_not_lowest"] += 1
        self.y, om, fl = ritz_coefficients(wr, wi, vr, self.sel)
        self.features["complex"] += int(np.sum(fl != 0))
        res = self._ritz_pass(self.y, om, None)
        self.ritz = True
        self.omega, self.resnorm, self.flags = np.zeros(self.nroots), np.full(self.nroots, np.inf), np.zeros(self.nroots, dtype=int)
        self.omega[:nr], self.resnorm[:nr], self.flags[:nr] = om, res, fl
        conv = nr == self.nroots
        for k in range(nr):
            if res[k] < tol:
                self.flags[k] |= FLAG_CONVERGED
            else:
                conv = False
                self.pend.append(self.corr[:, k].copy())
        return conv

    def linear_start(self, rhs, shifts):
        rhs = np.asarray(rhs, dtype=float)
        assert 1 <= rhs.shape[1] <= self.nroots and len(shifts) == self.nroots
        self.restart()
        self.linear, self.user_guess = True, False
        self.rhs, self.shifts = rhs, np.asarray(shifts, dtype=float)
        self.prhs = np.zeros((0, rhs.shape[1]))
        self.resnorm = np.full(self.nroots, np.inf)
        den = clamp(self.shifts[None, :] - self.op.diag[:, None])
        self.pend = [rhs[:, j % rhs.shape[1]] / den[:, j] for j in range(self.nroots)]

    def linear_step(self, tol):
        assert self.linear
        if self.nb == 0 and not self.pend:
            raise RuntimeError("no right-hand sides")
        self._basis_step(self.nroots)
        self.y = linear_coefficients(self.G, self.prhs, self.shifts)       # raises Pole: the basis stays, nothing is pending
        nrhs = self.rhs.shape[1]
        res = self._ritz_pass(self.y, self.shifts, self.rhs[:, np.arange(self.nroots) % nrhs])
        self.ritz = True
        self.omega, self.resnorm = self.shifts.copy(), res
        self.flags = np.where(res < tol, FLAG_CONVERGED, 0)
        self.pend = [(1.0 / res[j]) * self.corr[:, j] for j in range(self.nroots) if not res[j] < tol]
        return not self.pend


def run(st, tol, maxiter=100, linear=False):
    """iterate to convergence -> number of steps; raises when maxiter is not enough"""
    for it in range(1, maxiter + 1):
        if (st.linear_step(tol) if linear else st.step(tol)):
            return it
    raise RuntimeError("the Davidson restatement did not converge")


# ---------------------------------------------------------------------------------------------------------------- one-step evaluators
def _ld(a):
    return np.asarray(a, dtype=LD)


def ld_wdots(Bm, x, w):
    """<b_p, x>_W for the columns of Bm -> (values (long double), majorants sum w |b_p| |x|).  L = nvec"""
    wx = _ld(w) * _ld(x)
    return _ld(Bm).T @ wx, np.abs(Bm).T @ (w * np.abs(x))


def ld_project_normalise(Bm, x, w, Sm=None, sx=None):
    """What project_normalise must give, in long double, with majorants for (L + 64) 2^-53 M, L = nvec + 2 nb (a dot, then a combination
    over nb columns, for each of the two passes the longest single path is one dot and one combination; the passes add).
    Derivation, with e = (L + 64) 2^-53.  Pass 1: c_p = <b_p, x> has |dc_p| <= e Mc_p, Mc_p = sum w |b_p| |x| >= |c_p|; x1 = x - sum c_p b_p
    has |dx1| <= e (|x| + sum (|c_p| + Mc_p) |b_p|) <= e M1, M1 = |x| + 2 sum_p Mc_p |b_p|.  Pass 2 from x1: its coefficients carry their own
    dot rounding (Mc2_p from |x1|) and what dx1 feeds into them, sum w |b_p| M1 =: Mp_p; M2 = M1 + sum_p (2 Mc2_p + Mp_p) |b_p|.  The norm:
    n^2 = sum w x2^2 has |d n^2| <= e n^2 + 2 e sum w |x2| M2, so |dn| / n <= e (1/2 + sum w |x2| M2 / n^2), and b = x2 / n has
    |db| <= e (M2 / n + |b| (1 + sum w |x2| M2 / n^2)).  The companion sx goes the same way with |s_p| in the place of |b_p| in the combinations
    (the coefficients, and so their errors, are the same).
    -> None (dropped), or (b, s, Mb, Ms, n, ctot): b, s long double; Mb, Ms float64 majorants (s, Ms None without a companion); n the norm
    before scaling; ctot the |coefficients| of both passes added"""
    Bl, xl, wl = _ld(Bm), _ld(x), _ld(w)
    Ba = np.abs(Bm)
    Mx = np.abs(np.asarray(x, dtype=float))
    have_s = sx is not None
    ctot = np.zeros(Bm.shape[1])
    if have_s:
        Sl, sl, Sa = _ld(Sm), _ld(sx), np.abs(Sm)
        Ms = np.abs(np.asarray(sx, dtype=float))
    if Bm.shape[1]:
        for pas in range(2):
            c = Bl.T @ (wl * xl)
            ctot += np.abs(c).astype(float)
            xabs = np.abs(xl).astype(float)
            Mc = Ba.T @ (w * xabs)                       # own dot rounding (>= |c|)
            Mp = Ba.T @ (w * Mx) if pas else np.zeros_like(Mc)   # what the error of the vector so far feeds into the coefficients
            grow = 2.0 * Mc + Mp
            xl = xl - Bl @ c
            Mx = Mx + Ba @ grow
            if have_s:
                sl = sl - Sl @ c
                Ms = Ms + Sa @ grow
    n2 = np.sum(wl * xl * xl)
    n = np.sqrt(n2)
    if not n >= DROP:
        return None
    nf = float(n)
    xabs = np.abs(xl).astype(float)
    rel = 1.0 + float(np.sum(w * xabs * Mx)) / (nf * nf)
    b = xl / n
    Mb = Mx / nf + np.abs(b).astype(float) * rel
    if not have_s:
        return b, None, Mb, None, n, ctot
    s = sl / n
    return b, s, Mb, Ms / nf + np.abs(s).astype(float) * rel, n, ctot


def ld_sigma(op, b):
    """A b in long double -> (s, M) for (L + 64) 2^-53 M with L = nvec + r: t_j = <V_j, b> with |dt_j| <= e Mt_j, Mt_j = sum |V_j| |b|; then
    s = d b + sum_j U_j t_j with |ds| <= e (|d b| + sum_j |U_j| (|t_j| + Mt_j)) <= e (|d b| + 2 sum_j |U_j| Mt_j)"""
    bl = _ld(b)
    s = _ld(op.d) * bl
    M = np.abs(op.d * np.asarray(b, dtype=float))
    if op.r:
        t = _ld(op.V).T @ bl
        Mt = np.abs(op.V).T @ np.abs(np.asarray(b, dtype=float))
        s = s + _ld(op.U) @ t
        M = M + 2.0 * (np.abs(op.U) @ Mt)
    return s, M


def abs_apply(op, v):
    """a majorant of |A| v for v >= 0, the one ld_sigma uses: |d| v + 2 |U| (|V|^T v)"""
    return np.abs(op.d) * v + (2.0 * (np.abs(op.U) @ (np.abs(op.V).T @ v)) if op.r else 0.0)


def ld_combine(Bm, y):
    """B y in long double -> (values, M = |B| |y|); L = nb"""
    return _ld(Bm) @ _ld(y), np.abs(Bm) @ np.abs(y)


def ld_correction(x, sx, om, diag, rhs=None):
    """From the x and sx the device holds: rho = [rhs +] (sx - om x) and corr = rho / clamp(om - diag), column by column, in long double
    -> (rho, corr, Mrho, Mcorr) with Mrho = |sx| + |om x| [+ |rhs|], Mcorr = Mrho / |den|; L = 3 (a fused multiply-add, an addition, a division)"""
    xl, sl, oml = _ld(x), _ld(sx), _ld(om)[None, :]
    rho = sl - oml * xl
    Mrho = np.abs(sx) + np.abs(om)[None, :] * np.abs(x)
    if rhs is not None:
        rho = _ld(rhs) + rho
        Mrho = Mrho + np.abs(rhs)
    den = clamp(np.asarray(om, dtype=float)[None, :] - np.asarray(diag, dtype=float)[:, None])   # (the device forms it in float64 too)
    return rho, rho / _ld(den), Mrho, Mrho / np.abs(den)


def ld_precondition(rhs, shifts, diag):
    """the first pending vectors of the linear mode, pend_j = rhs_(j % nrhs) / clamp(shift_j - diag), in long double -> (pend, M = |pend|); the
    denominator is formed in float64 as the device forms it, so L = 1: one division"""
    den = clamp(np.asarray(shifts, dtype=float)[None, :] - np.asarray(diag, dtype=float)[:, None])
    cols = np.asarray(rhs, dtype=float)[:, np.arange(len(shifts)) % rhs.shape[1]]
    pend = _ld(cols) / _ld(den)
    return pend, np.abs(cols / den)


def ld_resnorm(rho, Mrho, w):
    """sqrt(rho^T W rho) per column -> (values, bound on |device - value| / ((nvec + 68) 2^-53)): the device sums w rho'^2 of its own rho' with
    |rho' - rho| <= 2 2^-53 Mrho, so |d n^2| <= (nvec + 64) 2^-53 sum w rho^2 + 4 2^-53 sum w |rho| Mrho <= (nvec + 68) 2^-53 sum w Mrho^2, and
    |dn| = |d n^2| / (n + n')"""
    n2 = np.sum(_ld(w)[:, None] * rho * rho, axis=0)
    return np.sqrt(n2), np.sum(w[:, None] * Mrho * Mrho, axis=0)


# ---------------------------------------------------------------------------------------------------------------- the cases of the two test files
NVECS = (7, 255, 256, 257, 600, 32768, 32769, 70001)   # below a wave, the block edges, 128 blocks in one trip, one element into the second, three ragged trips


def metrics(nvec):
    return ((0, 0.25), (3, 0.5), (nvec, 1.0), (nvec // 3, 0.25))


class Case:
    """one eigenvalue run: the operator, the metric, the state's extents, the guesses (columns; a None column is left out) and tol"""

    def __init__(self, op, n1, w2, nroots, ms, guesses, follow=False, tol=1e-9, name=""):
        self.op, self.n1, self.w2, self.nroots, self.ms, self.guesses, self.follow, self.tol, self.name = op, n1, w2, nroots, ms, guesses, follow, tol, name

    def restatement(self, eig=numpy_eig):
        st = Restatement(self.op, self.n1, self.w2, self.nroots, self.ms, self.follow, eig)
        for k, g in enumerate(self.guesses):
            if g is not None:
                st.set_guess(k, g)
        return st


def grid_case(nvec, n1, w2):
    """the vector-length grid: three roots in a space of six (a collapse at the third step)"""
    op, places = generate(nvec, r=4, seed=1)
    nroots = min(3, nvec // 2)
    return Case(op, n1, w2, nroots, 2 * nroots, list(unit_guesses(nvec, places, nroots).T), name=f"grid-{nvec}-{n1}-{w2}")


def roots_case(nvec, nroots, ms):
    """the root-count grid: Ritz chunks of 8 roots, k0 = 0, 8, 16, and a last chunk of one root"""
    op, places = generate(nvec, r=6, seed=10, coupling=0.35)
    return Case(op, nvec // 3, 0.25, nroots, ms, list(unit_guesses(nvec, places, nroots).T), name=f"roots-{nvec}-{nroots}-{ms}")


def complex_case():
    A = rotation_block_matrix()
    g = np.zeros((24, 2))
    g[0, 0] = g[1, 1] = 1.0
    g[2:, :] = 0.01
    return Case(dense_operator(A), 5, 0.5, 2, 40, list(g.T), tol=1e-10, name="complex")


def follow_case(follow):
    """guesses near the interior eigenvectors 5 and 6 of a 255-vector matrix, with a part of the two lowest mixed in: the lower roots enter
    the basis at once, and only the targets keep a following state away from them"""
    op, places = generate(255, r=4, seed=3)
    w, v = np.linalg.eig(op.dense())
    order = np.argsort(w.real)
    v = v[:, order].real
    g = [v[:, 5] + 0.05 * v[:, 0] + 0.02 * v[:, 1], v[:, 6] - 0.04 * v[:, 0] + 0.03 * v[:, 1]]
    return Case(op, 85, 0.25, 2, 16, g, follow=follow, name=f"follow-{int(follow)}")


def follow_drop_case():
    """follow_case's two guesses as the first and the third of THREE roots, the second column left out (zero: dropped at the guess step).
    The state then has two targets for three roots: at every later step the two nearest roots are taken target by target, and the third
    place goes to the lowest root not yet taken"""
    base = follow_case(True)
    return Case(base.op, base.n1, base.w2, 3, 16, [base.guesses[0], None, base.guesses[1]], follow=True, name="follow-drop")


def clamp_case():
    """the preconditioner diagonal set 5e-5 below the first root's guess-step value at one element and 5e-5 above it at another: the
    denominators omega - diag there are +5e-5 and -5e-5, inside +-CLAMP with each sign"""
    base = grid_case(600, 200, 0.25)
    st = base.restatement()
    st.step(base.tol)
    om0 = st.omega[0]
    diag = base.op.d.copy()
    e_pos, e_neg = 100, 411
    diag[e_pos], diag[e_neg] = om0 - 5e-5, om0 + 5e-5
    op = Operator(base.op.d, base.op.U, base.op.V, diag)
    c = Case(op, base.n1, base.w2, base.nroots, 12, base.guesses, name="clamp")
    c.e_pos, c.e_neg = e_pos, e_neg
    return c


def drop_case():
    """the second guess is a multiple of the first (in the span of B: dropped), the third is left out (zero: dropped)"""
    op, places = generate(257, r=4, seed=4)
    g = unit_guesses(257, places, 4)
    g0 = g[:, 0] + 0.1 * g[:, 1]
    return Case(op, 3, 0.5, 4, 8, [g0, -2.5 * g0, None, g[:, 3]], name="drop")


class LinearCase:
    def __init__(self, nvec, nrhs, nroots, ms=None, seed=5, clamp=False):
        self.op, places = generate(nvec, r=4, seed=seed)
        rng = np.random.default_rng(900 + 7 * nrhs + nroots)
        self.rhs = 0.05 * rng.standard_normal((nvec, nrhs))
        self.rhs[places[:nrhs], np.arange(nrhs)] += 1.0
        self.rhs[-1, :] += 0.5
        self.shifts = np.linspace(-0.3, 0.38, nroots) * np.where(np.arange(nroots) % 2, 1.0, -1.0)   # signed, below the spectrum (>= 0.49)
        if clamp:
            # the preconditioner diagonal 5e-5 below the first shift at one element and 5e-5 above the last shift at another: the start's
            # denominators shift - diag there are inside +-CLAMP with each sign (the clamp of davidson_precondition_kernel)
            self.e_pos, self.e_neg = 7, 11
            diag = self.op.d.copy()
            diag[self.e_pos], diag[self.e_neg] = self.shifts[0] - 5e-5, self.shifts[-1] + 5e-5
            self.op = Operator(self.op.d, self.op.U, self.op.V, diag)
        self.n1, self.w2, self.nroots, self.ms, self.tol = nvec // 3, 0.25, nroots, ms or 2 * nroots, 1e-9
        self.name = f"linear-{nvec}-{nrhs}-{nroots}" + ("-clamp" if clamp else "")

    def restatement(self):
        st = Restatement(self.op, self.n1, self.w2, self.nroots, self.ms)
        st.linear_start(self.rhs, self.shifts)
        return st

    @classmethod
    def of(cls, op, n1, w2, nroots, ms, rhs, shifts, tol, name):
        """a linear run on a given operator and state"""
        c = cls.__new__(cls)
        c.op, c.n1, c.w2, c.nroots, c.ms, c.rhs, c.shifts, c.tol, c.name = op, n1, w2, nroots, ms, np.asarray(rhs), np.asarray(shifts, dtype=float), tol, name
        return c


# ---------------------------------------------------------------------------------------------------------------- the step checker
def library_eig(g):
    """the unit's own host eigensolver (afesp_eig_general; no device needed) in the layout of numpy_eig"""
    from afesp_amd import capi
    lib = capi.load_library()
    n = g.shape[0]
    wr, wi, vr = np.zeros(n), np.zeros(n), np.zeros(n * n)
    rc = lib.afesp_eig_general(n, np.ascontiguousarray(np.asarray(g, dtype=float).ravel(order="F")), n, wr, wi, vr)
    if rc:
        raise RuntimeError(f"afesp_eig_general: status {rc}")
    return wr, wi, vr.reshape(n, n, order="F")


class Snapshot:
    """what a state holds between two steps: B, S, pend, x, sx, corr (columns), G, prhs, y, yom (the values the Ritz pass was given), omega,
    resnorm, flags, target, counts"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def snapshot_restatement(st):
    z = np.zeros((st.op.nvec, st.nroots))
    ritz = st.ritz
    return Snapshot(B=st._mat(st.B), S=st._mat(st.S), pend=st._mat(st.pend), x=st.x if ritz else z, sx=st.sx if ritz else z,
                    corr=st.corr if ritz else z, G=st.G.copy(), prhs=st.prhs.copy() if st.linear else None, y=st.y if ritz else None,
                    yom=(st.shifts if st.linear else st.omega[:st.y.shape[1]]) if ritz else None, omega=st.omega if ritz else None,
                    resnorm=st.resnorm if ritz else None, flags=st.flags if ritz else None, target=list(st.target), counts=st.counts())


def _plu_abs(a):
    """|L| |U| of the partial-pivot LU of a, rows in the pivoted order -> (|L||U|, row order)"""
    a = np.array(a, dtype=float)
    n = a.shape[0]
    perm = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if p != k:
            a[[k, p]] = a[[p, k]]
            perm[[k, p]] = perm[[p, k]]
        if a[k, k] != 0.0:
            a[k + 1:, k] /= a[k, k]
            a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k, k + 1:])
    L, U = np.tril(a, -1) + np.eye(n), np.triu(a)
    return np.abs(L) @ np.abs(U), perm


class StepChecker:
    """Checks (a) - (e) of one step from the snapshots before and after it.  `ratios` collects the largest error / bound per check name; a
    ratio above 1 raises.  `sbound` carries, column by column, the bound on |s_p - A b_p| the earlier checks established (a collapse
    combines the stored sigma, and with it their errors)."""

    def __init__(self, op, n1, w2, nroots, ms, eig=numpy_eig, log=None):
        self.op, self.w, self.nroots, self.ms, self.eig, self.log = op, weights(n1, op.nvec, w2), nroots, ms, eig, log
        self.ratios = {}
        self.sbound = np.zeros((op.nvec, 0))
        # backward error of the small host eigensolvers: p(nb) 2^-53 |G|_F.  p = 64 nb is an ASSUMPTION, not a derivation: the proven
        # bounds of the QR algorithm are O(nb^2) or worse and never attained, O(nb) is what is observed; 64 is tol_factor's constant
        self.host_p = lambda nb: 64 * nb

    def _put(self, name, err, bound):
        err, bound = np.asarray(err, dtype=float), np.asarray(bound, dtype=float)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / bound)
        r = float(np.max(ratio)) if ratio.size else 0.0
        self.ratios[name] = max(self.ratios.get(name, 0.0), r)
        if self.log is not None:
            self.log(f"    {name:<22s} error / bound = {r:.3e}   (largest error {float(np.max(err)) if err.size else 0.0:.3e})")
        assert r <= 1.0, f"{name}: error / bound = {r:.3e} (largest error {float(np.max(err)):.3e})"

    def _cmp(self, name, dev, ref, M, L):
        self._put(name, np.abs(_ld(dev) - ref).astype(float), tol_factor(L) * M)

    def basis(self, pre, post, linear):
        """(a), (b): the columns of B and S after the step; -> index of the first new (or rewritten) column"""
        op, w, ms = self.op, self.w, self.ms
        nvec, nbp, npend = op.nvec, pre.B.shape[1], pre.pend.shape[1]
        collapsed = nbp + npend > ms
        sb = []
        j = 0
        if collapsed:
            nkeep = self.nroots if linear else min(self.nroots, nbp)
            for k in range(nkeep):
                got = ld_project_normalise(post.B[:, :j], pre.x[:, k], w, post.S[:, :j], pre.sx[:, k])
                if got is None:
                    continue
                assert j < post.B.shape[1], "collapse: the device kept fewer vectors than the rule"
                b, s, Mb, Ms, n, ctot = got
                L = nvec + 2 * j
                self._cmp("a collapse B", post.B[:, j], b, Mb, L)
                self._cmp("b collapse S", post.S[:, j], s, Ms, L)
                # ... and A b.  What the device held: sx_k - A x_k = sum_p y_pk (s_p - A b_p) and the rounding of the two combinations,
                # |.| <= sbound |y_k| + e_nb (|S| |y_k| + |A| |B| |y_k|); the projection subtracts the new columns with the coefficients
                # ctot, and their own departures with them; all of it is divided by the norm n; the roundings of the projection itself
                # are e_L (Ms + |A| Mb).
                ya = np.abs(pre.y[:, k])
                dx = self.sbound @ ya + tol_factor(nbp) * (np.abs(pre.S) @ ya + abs_apply(op, np.abs(pre.B) @ ya))
                prev = np.array(sb).T @ ctot if sb else 0.0
                bound = (dx + prev) / float(n) + tol_factor(L + op.r) * (Ms + abs_apply(op, Mb))
                sA = ld_sigma(op, post.B[:, j])[0]
                self._put("b collapse S = A B", np.abs(_ld(post.S[:, j]) - sA).astype(float), bound)
                sb.append(bound)
                j += 1
        else:
            assert post.B.shape[1] >= nbp and np.array_equal(post.B[:, :nbp], pre.B) and np.array_equal(post.S[:, :nbp], pre.S), \
                "stored columns changed without a collapse"
            sb = [self.sbound[:, p] for p in range(nbp)]
            j = nbp
        first_new = 0 if collapsed else nbp
        for k in range(npend):
            if j >= ms:
                break
            got = ld_project_normalise(post.B[:, :j], pre.pend[:, k], w)
            if got is None:
                continue
            assert j < post.B.shape[1], "the device dropped a pending vector the rule keeps"
            b, _, Mb, _, _, _ = got
            self._cmp("a new B", post.B[:, j], b, Mb, nvec + 2 * j)
            s, Ms = ld_sigma(op, post.B[:, j])
            self._cmp("b new S = A b", post.S[:, j], s, Ms, nvec + op.r)
            sb.append(tol_factor(nvec + op.r) * Ms)
            j += 1
        assert j == post.B.shape[1], f"the device holds {post.B.shape[1]} columns, the rule gives {j}"
        self.sbound = np.array(sb).T if sb else np.zeros((nvec, 0))
        # |B^T W B - 1|: two operations deep.  The bound is the departure of the float64 restatement of the same operation on the same
        # inputs (its own rounding through the two passes) plus the bound of the one dot that measures it.
        if post.B.shape[1]:
            Bn = post.B
            dev = np.abs(np.asarray(_ld(Bn * w[:, None]).T @ _ld(Bn) - np.eye(Bn.shape[1]), dtype=float))
            ref = self._restated_departure(pre, post, linear, collapsed)
            Mdot = (np.abs(Bn) * w[:, None]).T @ np.abs(Bn)
            self._put("a |B^T W B - 1|", dev, ref + tol_factor(nvec) * Mdot)
        return first_new

    def _restated_departure(self, pre, post, linear, collapsed):
        """max |B^T W B - 1| of the float64 restatement of the step's orthonormalisations, from the same inputs"""
        w = self.w
        cols = [] if collapsed else [pre.B[:, p] for p in range(pre.B.shape[1])]
        mat = lambda: np.array(cols).T if cols else np.zeros((self.op.nvec, 0))
        if collapsed:
            for k in range(self.nroots if linear else min(self.nroots, pre.B.shape[1])):
                got = project_normalise(mat(), pre.x[:, k].copy(), w)
                if got is not None:
                    cols.append(got[0])
        for k in range(pre.pend.shape[1]):
            if len(cols) >= self.ms:
                break
            got = project_normalise(mat(), pre.pend[:, k].copy(), w)
            if got is not None:
                cols.append(got[0])
        Bm = mat()
        return float(np.max(np.abs((Bm * w[:, None]).T @ Bm - np.eye(Bm.shape[1])))) if cols else 0.0

    def linear_start(self, pend, rhs, shifts):
        """the pending vectors a linear start leaves: the preconditioned right-hand sides, system j with column j % nrhs"""
        assert pend.shape == (self.op.nvec, len(shifts))
        ref, M = ld_precondition(rhs, shifts, self.op.diag)
        self._cmp("start pend", pend, ref, M, 1)

    def projected(self, pre, post, first_new, rhs=None):
        """(c): G = B^T W S (and prhs = B^T W rhs); what is older than the step is bit-identical"""
        w, nvec, nb = self.w, self.op.nvec, post.B.shape[1]
        assert post.G.shape == (nb, nb)
        if first_new:
            assert np.array_equal(post.G[:first_new, :first_new], pre.G[:first_new, :first_new]), "older elements of G changed"
        new = np.arange(first_new, nb)
        if new.size:
            Bw, Ba = _ld(post.B * w[:, None]), np.abs(post.B) * w[:, None]
            cols, Mc = Bw.T @ _ld(post.S[:, new]), Ba.T @ np.abs(post.S[:, new])
            self._cmp("c G columns", post.G[:, new], cols, Mc, nvec)
            rows, Mr = Bw[:, new].T @ _ld(post.S), Ba[:, new].T @ np.abs(post.S)
            self._cmp("c G rows", post.G[new, :], rows, Mr, nvec)
        if rhs is not None:
            assert post.prhs.shape == (nb, rhs.shape[1])
            if first_new:
                assert np.array_equal(post.prhs[:first_new], pre.prhs[:first_new]), "older rows of prhs changed"
            ref, M = _ld(post.B * w[:, None]).T @ _ld(rhs), (np.abs(post.B) * w[:, None]).T @ np.abs(rhs)
            self._cmp("c prhs", post.prhs, ref, M, nvec)

    def host_eigen(self, pre, post, guess_step, follow_user):
        """(d): omega, flags, the selection and y from the fetched G"""
        G = post.G
        nb = G.shape[0]
        nr = min(self.nroots, nb)
        wr, wi, vr = self.eig(G)
        target = list(wr[:nr]) if (guess_step and follow_user) else pre.target
        assert list(post.target) == list(target), "the targets changed"
        sel = select_roots(wr, nr, target, guess_step)
        y, om, fl = ritz_coefficients(wr, wi, vr, sel)
        assert np.array_equal(post.yom, om) and np.array_equal(post.omega[:nr], om), (post.yom, om)
        assert np.array_equal(post.flags[:nr] & FLAG_COMPLEX, fl), (post.flags, fl)
        assert np.array_equal(post.y, y), "y is not the rule applied to the host eigenvectors of the fetched G"
        # ... and against numpy.linalg.eig of the same G: the same roots are taken, and every (omega, y) is an eigenpair of G within the
        # backward error of a QR eigensolver, p(nb) 2^-53 |G|_F (both solvers have it: twice)
        nwr, nwi, nvr = numpy_eig(G)
        nsel = select_roots(nwr, nr, target, guess_step)
        gF = float(np.linalg.norm(G))
        e = self.host_p(nb) * EPS53 * gF
        kappa = float(np.linalg.cond(np.linalg.eig(G)[1]))
        self._put("d omega vs numpy", np.abs(post.yom - nwr[nsel]), np.full(nr, 2.0 * kappa * e))
        assert np.array_equal(fl != 0, nwi[nsel] != 0.0), "complex flags differ from numpy's roots"
        for k in range(nr):
            yk, a, b = post.y[:, k], om[k], nwi[nsel[k]]
            if fl[k]:
                Ga = G - a * np.eye(nb)
                self._put("d pair subspace", np.linalg.norm(Ga @ (Ga @ yk) + b * b * yk), 4.0 * kappa * e * (gF + abs(a) + abs(b)))
            else:
                self._put("d eigenpair", np.linalg.norm(G @ yk - a * yk), 2.0 * kappa * e)
            self._put("d sum y^2", abs(float(np.sum(yk * yk)) - 1.0), tol_factor(nb))

    def host_linear(self, post, shifts):
        """(d), linear mode: (G - shift_j) y_j = -prhs_j within the backward error of partial-pivot LU, 3 nb roundings on |L| |U| |y|"""
        G, nb, nrhs = post.G, post.G.shape[0], post.prhs.shape[1]
        assert np.array_equal(post.yom, shifts)
        for j, om in enumerate(shifts):
            m = G - om * np.eye(nb)
            LU, perm = _plu_abs(m)
            yj, b = post.y[:, j], -post.prhs[:, j % nrhs]
            r = np.abs(np.asarray(_ld(m) @ _ld(yj) - _ld(b), dtype=float))[perm]
            self._put("d LU residual", r, tol_factor(3 * nb) * (LU @ np.abs(yj) + np.abs(b[perm])))

    def ritz(self, post, tol, linear, rhs=None):
        """(e): x, sx from B, S, y; corr and resnorm from the x, sx held; the next pending vectors and the flags"""
        op, w = self.op, self.w
        nb, nr = post.B.shape[1], post.y.shape[1]
        x, Mx = ld_combine(post.B, post.y)
        self._cmp("e x = B y", post.x[:, :nr], x, Mx, nb)
        sx, Ms = ld_combine(post.S, post.y)
        self._cmp("e sx = S y", post.sx[:, :nr], sx, Ms, nb)
        rcols = None if rhs is None else rhs[:, np.arange(nr) % rhs.shape[1]]
        rho, corr, Mrho, Mcorr = ld_correction(post.x[:, :nr], post.sx[:, :nr], post.yom, op.diag, rcols)
        self._cmp("e corr", post.corr[:, :nr], corr, Mcorr, 3)
        res, M2 = ld_resnorm(rho, Mrho, w)
        dev = post.resnorm[:nr]
        self._put("e resnorm", np.abs(_ld(dev) - res).astype(float) * (dev + res.astype(float)), (op.nvec + 68 + 64) * EPS53 * M2)
        assert np.all(post.resnorm[nr:] == np.inf) and np.all(post.omega[nr:] == 0.0)
        conv = dev < tol
        assert np.array_equal((post.flags[:nr] & FLAG_CONVERGED) != 0, conv), (post.flags, dev, tol)
        want = [(1.0 / dev[k]) * post.corr[:, k] if linear else post.corr[:, k] for k in range(nr) if not conv[k]]
        assert post.pend.shape[1] == len(want), (post.pend.shape, len(want))
        for k, c in enumerate(want):
            assert np.array_equal(post.pend[:, k], c), f"pending vector {k} is not the correction of its root"
        return bool(np.all(conv)) and nr == self.nroots

    def step(self, pre, post, tol, linear=False, rhs=None, shifts=None, follow_user=False):
        """every check of one step -> converged, as the checks give it"""
        guess_step = pre.B.shape[1] == 0
        first_new = self.basis(pre, post, linear)
        self.projected(pre, post, first_new, rhs if linear else None)
        if linear:
            self.host_linear(post, shifts)
        else:
            self.host_eigen(pre, post, guess_step, follow_user)
        return self.ritz(post, tol, linear, rhs if linear else None)


def pole_case():
    """seven elements, two roots in a space of eight: the eigenvalue run ends with the whole space as its basis and the lowest root to rounding;
    the linear run that follows on the same state has that root as its first shift, and meets the pole once its basis is the whole space"""
    op, places = generate(7, r=2, seed=6)
    c = Case(op, 3, 0.5, 2, 8, list(unit_guesses(7, places, 2).T), tol=1e-12, name="pole")
    rng = np.random.default_rng(61)
    c.rhs = rng.standard_normal((7, 1))
    c.other_shift = -0.2
    return c
