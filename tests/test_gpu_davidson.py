"""The block Davidson unit (csrc/davidson_so.hip) run directly, through the test entry afesp_test_davidson_*, on matrices given as data
(A = diag(d) + U V^T, np_davidson.generate), and compared after EVERY step with the long-double one-step evaluators of np_davidson applied
to what the device held before the step.

What is checked per step (np_davidson.StepChecker):
  a  the new columns of B are the two-pass projection of the pending vectors against the columns before them, scaled to unit norm, in order,
     vectors below DROP absent; |B^T W B - 1|
  b  every new column of S is A b element by element; after a collapse every column of B and S is the stated combination of the Ritz vectors
     and their sigma, and S = A B within the bound carried through that combination
  c  G = B^T W S (linear mode: prhs = B^T W rhs); what is older than the step is bit-identical to the previous fetch
  d  omega, flags, the selection and y are bit for bit the unit's rules applied to the host eigenvectors (afesp_eig_general) of the FETCHED
     G, the same roots as numpy.linalg.eig of it gives, and eigenpairs of it; linear mode: y_j solves the fetched G - shift_j
  e  x = B y, sx = S y; corr = rho / clamp(omega - diag) and resnorm = sqrt(rho^T W rho) from the x and sx held; the next pending vectors
     bit for bit the corrections of the unconverged roots, in order (linear mode: times 1 / |rho|)
  f  nsigma, ncollapse, nb, npend are those of the float64 restatement (np_davidson.Restatement) of the same run

Bounds.  Every check is one operation deep from fetched inputs: |device - reference| <= (L + 64) 2^-53 M, with L the number of rounded
additions on the element's path (nvec for a dot product, nb for a combination, their sum where an operation is a dot followed by a
combination) and M the evaluator's majorant: the same expression over absolute values, with the part that the error of a first stage
feeds into a second added (derived at each np_davidson.ld_* function; the form of np_triples.tol_factor).  64 covers the reduction tree
over lanes, waves and blocks, the products, a division or a square root.  The host solvers: an eigenpair of the fetched G holds within
2 kappa(V) p(nb) 2^-53 |G|_F with p = 64 nb, the backward error of a QR eigensolver (twice: numpy's and the unit's), and an LU solution
within 3 nb roundings on |L| |U| |y|.  p = 64 nb is an assumption (what QR eigensolvers are observed to do), not a derivation; and the
bit-for-bit part of (d) takes its eigenvectors from afesp_eig_general, the solver the unit itself calls, so it checks the unit's RULES on
those vectors -- the solver is held to numpy by that cross-check and by tests/test_eom_cpu.py.  End to end, |omega_k - w_k| <= kappa(V)
resnorm_k with the device's own resnorm_k, plus the dense reference's own kappa(V) (nvec + 64) 2^-53 |A|_2.  |B^T W B - 1| is two operations deep: its bound is the departure that the float64 restatement of the
same orthonormalisation has on the same fetched inputs plus the bound of the one dot product that measures it -- the restatement's own
rounding stands for the first stage because no majorant of a projection's loss of orthogonality is sharper than running it.
Nothing here is tuned to what the device gave; `-s` prints error / bound of every check.

Largest error / bound seen on an MI355X, per group of cases (every check of every step):
  vector-length grid, nvec = 7 / 255 / 256 / 257 / 600 (4 metrics each)   0.060 / 0.060 / 0.057 / 0.068 / 0.059
  vector-length grid, nvec = 32768 / 32769 / 70001                         0.072 / 0.071 / 0.072
  root-count grid at nvec = 600,   nroots = 1 / 8 / 9 / 17                 0.040 / 0.083 / 0.089 / 0.108
  root-count grid at nvec = 32769, nroots = 1 / 8 / 9 / 17                 0.047 / 0.110 / 0.118 / 0.115
  complex pair 0.050, following 0.054, not following 0.079, following with a dropped guess 0.081, clamp 0.067, drop 0.061,
  pole (both modes) 0.048; the preconditioned start of the linear mode (with its clamp) 0.015
  linear mode at nvec = 600 (nrhs, nroots) = (1,3) / (1,12) / (3,3) / (3,12)     0.060 / 0.100 / 0.061 / 0.102
  linear mode at nvec = 32769                                                   0.069 / 0.121 / 0.069 / 0.121
The largest ratios are those of x = B y and sx = S y (a combination of nb terms against its majorant) and of sum y^2 = 1; the dot
products of nvec terms stay below 1e-3 of their bounds at nvec >= 32768 (the partial sums over blocks and the tree within a block add far
fewer roundings in a row than the nvec the bound allows).  The same tests on four deliberately wrong builds of davidson_so.hip: weight 1
behind n1 in the panel kernel -- every case with w2 != 1 fails (first at the norm of check a); the partial index without blockIdx.x --
every case with nvec >= 257 fails; the Ritz chunk offset at 0 -- every case with nroots >= 9 fails (check e); `c - 1` as `c` -- the
complex case fails (check d).
"""
import numpy as np
import pytest

import np_davidson as nd
from afesp_amd.capi import AfespError, Engine

pytestmark = pytest.mark.gpu

LARGE_STEPS = 4        # steps of a run above nvec = 600: a guess step, an extension, a collapse, one more
SMALL_STEPS = 30


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def snapshot(eng, linear, out):
    """what the device holds; out: what the last iterate call returned (None before the first step)"""
    f = eng.davidson_test_fetch
    n1, nvec, nroots, ms = eng.davidson_test_shape
    s = nd.Snapshot(B=f("B"), S=f("S"), pend=f("pend"), x=f("x"), sx=f("sx"), corr=f("corr"), G=f("G"), prhs=f("prhs") if linear else None,
                    target=list(f("target")), counts=f("counts"), y=None, yom=None, omega=None, resnorm=None, flags=None)
    if out is not None:
        s.y, s.yom = f("y")
        s.omega, s.resnorm, s.flags = out
    return s


def start(eng, case, follow=None):
    eng.davidson_test_create(case.n1, case.op.nvec, case.w2, case.follow if follow is None else follow, case.nroots, case.ms, case.op.d, case.op.U,
                             case.op.V, case.op.diag)
    for k, g in enumerate(case.guesses):
        if g is not None:
            eng.davidson_test_set_guess(k, g)


def device_step(eng, tol, linear):
    if linear:
        res, fl, counts, conv = eng.davidson_test_linear_iterate(tol)
        return (np.array(eng.davidson_test_fetch("y")[1]), res, fl), counts, conv
    om, res, fl, counts, conv = eng.davidson_test_iterate(tol)
    return (om, res, fl), counts, conv


def run_checked(eng, case, maxsteps, linear=False, st=None, quiet=False):
    """the device and the float64 restatement side by side, every step checked -> (restatement, checker, last snapshot, converged)"""
    st = st or (case.restatement() if linear else case.restatement(nd.library_eig))
    log = None if quiet else print
    ck = nd.StepChecker(case.op, case.n1, case.w2, case.nroots, case.ms, nd.library_eig, log)
    pre = snapshot(eng, linear, None)
    assert pre.counts == st.counts()
    if linear and pre.counts["nb"] == 0:
        ck.linear_start(pre.pend, case.rhs, case.shifts)                                     # what davidson_linear_start left
    conv = False
    for it in range(1, maxsteps + 1):
        conv_ref = st.linear_step(case.tol) if linear else st.step(case.tol)
        res = st.resnorm[np.isfinite(st.resnorm)]
        assert not np.any((res > case.tol / 1.05) & (res < case.tol * 1.05)), "the case is too close to tol: re-seed it in test_davidson_cpu.py"
        out, counts, conv = device_step(eng, case.tol, linear)
        post = snapshot(eng, linear, out)
        if log:
            log(f"  {case.name} step {it}: counts {counts}")
        got = ck.step(pre, post, case.tol, linear, case.rhs if linear else None, case.shifts if linear else None,
                      False if linear else bool(st.follow and st.user_guess))
        assert got == conv == conv_ref
        assert counts == post.counts == st.counts(), (counts, st.counts())                       # (f)
        pre = post
        if conv:
            break
    print(f"{case.name}: {it} steps, largest error / bound {max(ck.ratios.values()):.3e} in '{max(ck.ratios, key=ck.ratios.get)}'")
    return st, ck, pre, conv


def residual_certificate(eng, case, ck, post, shifts=None, rhs=None):
    """The residual recomputed in long double from the device's x: |[rhs +] A x - omega x|_W <= resnorm + its bound.  The bound: sx - A x =
    sum_p y_p (s_p - A b_p) and the rounding of the two combinations, |.| <= sbound |y| + e_nb (|S| |y| + |A| |B| |y|) =: E; then
    |rho_true|_W <= |rho_dev|_W + |E|_W, and resnorm is |rho_dev|_W within the bound of check (e)."""
    op, w = case.op, ck.w
    nr = post.y.shape[1]
    out = []
    for k in range(nr):
        x = eng.davidson_test_get_vector(k)
        assert np.array_equal(x, post.x[:, k])
        r = nd.ld_sigma(op, x)[0] - nd._ld(post.yom[k]) * nd._ld(x)
        if rhs is not None:
            r = r + nd._ld(rhs[:, k % rhs.shape[1]])
        true = float(np.sqrt(np.sum(nd._ld(w) * r * r)))
        ya = np.abs(post.y[:, k])
        E = ck.sbound @ ya + nd.tol_factor(post.B.shape[1]) * (np.abs(post.S) @ ya + nd.abs_apply(op, np.abs(post.B) @ ya))
        M = np.abs(post.sx[:, k]) + abs(post.yom[k]) * np.abs(post.x[:, k]) + (np.abs(rhs[:, k % rhs.shape[1]]) if rhs is not None else 0.0)
        bound = float(np.sqrt(np.sum(w * E * E))) + (op.nvec + 132) * nd.EPS53 * float(np.sum(w * M * M)) / max(post.resnorm[k], 1e-300)
        print(f"  {case.name} root {k}: resnorm {post.resnorm[k]:.3e}, recomputed {true:.3e}, bound on the difference {bound:.3e}")
        assert true <= post.resnorm[k] + bound
        out.append(true)
    return np.array(out)


def end_to_end(eng, case, ck, post, conv, expect=None):
    """small nvec: converged, the residual certificate, and the roots against dense numpy.linalg.eig"""
    assert conv and np.all(post.resnorm < case.tol)
    true = residual_certificate(eng, case, ck, post)
    w, v = np.linalg.eig(case.op.dense())
    order = np.argsort(w.real)
    kappa = float(np.linalg.cond(v))
    ref = w[order].real[:case.nroots] if expect is None else expect
    # kappa(V) resnorm_k with the device's own resnorm, and the dense reference's own error in the form the complex case has it
    bound = kappa * post.resnorm + kappa * nd.tol_factor(case.op.nvec) * float(np.linalg.norm(case.op.dense(), 2))
    print(f"  {case.name}: |omega - dense eig| {np.abs(post.omega - ref)}, bound {bound}")
    assert np.all(np.abs(post.omega - ref) <= bound)


# ---------------------------------------------------------------------------------------------------------------- the grids
@pytest.mark.parametrize("metric", range(4))
@pytest.mark.parametrize("nvec", nd.NVECS)
def test_vector_length_and_metric_grid(eng, nvec, metric):
    n1, w2 = nd.metrics(nvec)[metric]
    case = nd.grid_case(nvec, n1, w2)
    start(eng, case)
    small = nvec <= 600
    st, ck, post, conv = run_checked(eng, case, SMALL_STEPS if small else LARGE_STEPS, quiet=not small and metric != 3)
    assert st.ncollapse >= 1                                                          # the collapse was checked too
    if nvec >= 32768:
        assert abs(post.x[-1, 0]) > 0.5                                                   # a unit-magnitude entry in the last element
    if small:
        end_to_end(eng, case, ck, post, conv)
    else:
        residual_certificate(eng, case, ck, post)


@pytest.mark.parametrize("full", [False, True], ids=["2nroots", "40"])
@pytest.mark.parametrize("nroots", [1, 8, 9, 17])
@pytest.mark.parametrize("nvec", [600, 32769])
def test_root_count_grid(eng, nvec, nroots, full):
    case = nd.roots_case(nvec, nroots, 40 if full else 2 * nroots)
    start(eng, case)
    small = nvec <= 600
    st, ck, post, conv = run_checked(eng, case, SMALL_STEPS if small else (LARGE_STEPS if nroots > 1 else 6), quiet=True)
    if not full:
        assert st.ncollapse >= 1
    if small:
        end_to_end(eng, case, ck, post, conv)
    else:
        residual_certificate(eng, case, ck, post)


# ---------------------------------------------------------------------------------------------------------------- the named cases
def test_complex_pair_among_the_lowest_roots(eng):
    case = nd.complex_case()
    start(eng, case)
    st = case.restatement(nd.library_eig)
    ck = nd.StepChecker(case.op, case.n1, case.w2, case.nroots, case.ms, nd.library_eig, None)
    pre = snapshot(eng, False, None)
    for it in range(1, 25):
        st.step(case.tol)
        out, counts, conv = device_step(eng, case.tol, False)
        post = snapshot(eng, False, out)
        assert not ck.step(pre, post, case.tol) and not conv
        assert counts == st.counts()
        assert np.all(post.flags == nd.FLAG_COMPLEX) and post.omega[0] == post.omega[1]     # both members, the pair's real part
        assert np.array_equal(post.x[:, 0], post.x[:, 1])                                   # their vectors are identical
        assert counts["nb"] == (2 if it == 1 else min(pre.counts["nb"] + 1, 24)) and counts["npend"] == 2   # the duplicate is dropped
        pre = post
    print("complex:", {k: float(f"{v:.3g}") for k, v in ck.ratios.items()})
    assert "d pair subspace" in ck.ratios and pre.counts["nb"] == 24
    A = case.op.dense()
    w, v = np.linalg.eig(A)
    lowest = w[np.argsort(w.real)[0]]
    assert lowest.imag != 0.0
    bound = float(np.linalg.cond(v)) * nd.tol_factor(24) * float(np.linalg.norm(A, 2))
    print(f"complex: omega {pre.omega[0]!r}, dense eig {lowest.real!r}, error {abs(pre.omega[0] - lowest.real):.3e}, bound {bound:.3e}")
    assert abs(pre.omega[0] - lowest.real) <= bound


def test_following_keeps_the_targets_and_not_following_falls_to_the_lowest(eng):
    c1, c0 = nd.follow_case(True), nd.follow_case(False)
    w = np.sort(np.linalg.eigvals(c1.op.dense()).real)
    start(eng, c1)
    st, ck, post, conv = run_checked(eng, c1, SMALL_STEPS, quiet=True)
    assert st.features["selected_not_lowest"] > 0 and len(post.target) == 2
    end_to_end(eng, c1, ck, post, conv, expect=w[[5, 6]])
    followed = post.omega.copy()
    # a guess set after a running iteration starts over: no basis, no targets, the counts at zero
    eng.davidson_test_set_guess(0, c0.guesses[0])
    assert eng.davidson_test_fetch("counts") == dict(nsigma=0, ncollapse=0, nb=0, npend=1) and len(eng.davidson_test_fetch("target")) == 0
    eng.davidson_test_set_guess(1, c0.guesses[1])
    st, ck, post2, conv = run_checked(eng, c1, SMALL_STEPS, quiet=True)                       # the same run again, to the bit
    assert np.array_equal(post2.omega, followed) and np.array_equal(post2.x, post.x)
    start(eng, c0)
    st, ck, post, conv = run_checked(eng, c0, SMALL_STEPS, quiet=True)
    assert st.features["selected_not_lowest"] == 0 and post.target == []
    end_to_end(eng, c0, ck, post, conv, expect=w[[0, 1]])


def test_following_with_a_dropped_guess_fills_the_place_with_the_lowest_root(eng):
    """two targets for three roots: `nt = min(nr, targets)` and the places beyond the targets in the selection"""
    case = nd.follow_drop_case()
    w = np.sort(np.linalg.eigvals(case.op.dense()).real)
    start(eng, case)
    st, ck, post, conv = run_checked(eng, case, SMALL_STEPS)
    assert len(post.target) == 2 and post.counts["nb"] > 3 and st.sel == [0, 5, 6]
    end_to_end(eng, case, ck, post, conv, expect=w[[0, 5, 6]])


def test_clamp_with_each_sign(eng):
    case = nd.clamp_case()
    start(eng, case)
    st = case.restatement(nd.library_eig)
    ck = nd.StepChecker(case.op, case.n1, case.w2, case.nroots, case.ms, nd.library_eig, print)
    pre = snapshot(eng, False, None)
    st.step(case.tol)
    out, counts, conv = device_step(eng, case.tol, False)
    post = snapshot(eng, False, out)
    ck.step(pre, post, case.tol)
    den = post.omega[0] - case.op.diag
    assert 0.0 < den[case.e_pos] < nd.CLAMP and -nd.CLAMP < den[case.e_neg] < 0.0
    rho = post.sx[:, 0] - post.omega[0] * post.x[:, 0]
    for e, sign in ((case.e_pos, 1.0), (case.e_neg, -1.0)):
        assert abs(rho[e]) > 1e-6
        # rho / +-1e-4, from the x and sx held: one fused multiply-add and one division
        assert abs(post.corr[e, 0] - rho[e] / (sign * nd.CLAMP)) <= nd.tol_factor(3) * (abs(post.sx[e, 0]) + abs(post.omega[0] * post.x[e, 0])) / nd.CLAMP
        assert np.sign(post.corr[e, 0]) == sign * np.sign(rho[e])
    start(eng, case)
    st, ck, post, conv = run_checked(eng, case, SMALL_STEPS, quiet=True)
    end_to_end(eng, case, ck, post, conv)


def test_dropped_guesses_and_a_vanished_block(eng):
    case = nd.drop_case()
    start(eng, case)
    st, ck, post, conv = run_checked(eng, case, 1)
    assert st.features["dropped"] == 2 and post.counts == dict(nsigma=2, ncollapse=0, nb=2, npend=2)
    assert np.all(np.isinf(post.resnorm[2:])) and np.all(post.omega[2:] == 0.0) and np.all(post.flags[2:] == 0)
    start(eng, case)
    st, ck, post, conv = run_checked(eng, case, SMALL_STEPS, quiet=True)
    end_to_end(eng, case, ck, post, conv)
    # every guess vector vanished: status 1, and the state stays usable
    eng.davidson_test_set_guess(1, np.zeros(case.op.nvec))
    with pytest.raises(AfespError, match="status 1: .*every guess vector vanished"):
        eng.davidson_test_iterate(case.tol)
    with pytest.raises(AfespError, match="status 1: .*no guess vectors"):
        eng.davidson_test_iterate(case.tol)
    for k, g in enumerate(case.guesses):
        if g is not None:
            eng.davidson_test_set_guess(k, g)
    st, ck, post2, conv = run_checked(eng, case, SMALL_STEPS, quiet=True)
    assert conv and np.array_equal(post2.omega, post.omega) and np.array_equal(post2.x, post.x)


# ---------------------------------------------------------------------------------------------------------------- linear mode
def linear_start(eng, case):
    eng.davidson_test_create(case.n1, case.op.nvec, case.w2, False, case.nroots, case.ms, case.op.d, case.op.U, case.op.V, case.op.diag)
    eng.davidson_test_linear_start(case.rhs, case.shifts)


@pytest.mark.parametrize("nroots", [3, 12])
@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("nvec", [600, 32769])
def test_linear_mode(eng, nvec, nrhs, nroots):
    case = nd.LinearCase(nvec, nrhs, nroots)
    linear_start(eng, case)
    small = nvec <= 600
    st, ck, post, conv = run_checked(eng, case, SMALL_STEPS if small else 3, linear=True, quiet=not (small and nroots == 3))
    assert st.ncollapse >= 1 and {"c prhs", "d LU residual", "b collapse S = A B"} <= set(ck.ratios)
    true = residual_certificate(eng, case, ck, post, case.shifts, case.rhs)
    if small:
        assert conv
        A, n = case.op.dense(), nvec
        for j in range(nroots):
            m = A - case.shifts[j] * np.eye(n)
            x = np.linalg.solve(m, -case.rhs[:, j % nrhs])
            # |x - x*|_2 <= |m^-1|_2 |rho|_2 (kappa resnorm in absolute terms), |rho|_2 <= |rho|_W / sqrt(min w); and the dense solve's own error
            smin = np.linalg.svd(m, compute_uv=False)[-1]
            bound = true[j] / np.sqrt(ck.w.min()) / smin + n * np.linalg.cond(m) * nd.EPS53 * np.linalg.norm(x)
            assert np.linalg.norm(x - post.x[:, j]) <= bound


def test_linear_start_clamps_with_each_sign(eng):
    """davidson_precondition_kernel: shift - diag inside +-CLAMP with each sign gives rhs / +-1e-4"""
    case = nd.LinearCase(600, 3, 3, clamp=True)
    linear_start(eng, case)
    pend = eng.davidson_test_fetch("pend")
    den = case.shifts[None, :] - case.op.diag[:, None]
    assert 0.0 < den[case.e_pos, 0] < nd.CLAMP and -nd.CLAMP < den[case.e_neg, 2] < 0.0
    for e, j, sign in ((case.e_pos, 0, 1.0), (case.e_neg, 2, -1.0)):
        r = case.rhs[e, j % 3]
        assert r != 0.0 and abs(pend[e, j] - r / (sign * nd.CLAMP)) <= nd.tol_factor(1) * abs(r) / nd.CLAMP
    st, ck, post, conv = run_checked(eng, case, 2, linear=True)                               # (checks the whole start, then two steps)
    assert "start pend" in ck.ratios


def test_pole_after_an_eigenvalue_run_and_back(eng):
    case = nd.pole_case()
    start(eng, case)
    st, ck, post, conv = run_checked(eng, case, 20, quiet=True)
    assert conv and post.counts["nb"] == 7
    first = post
    shifts = [post.omega[0], case.other_shift]
    lin = nd.LinearCase.of(case.op, case.n1, case.w2, 2, case.ms, case.rhs, shifts, 1e-9, "pole-linear")   # the same operator and state
    eng.davidson_test_linear_start(case.rhs, shifts)
    st.linear_start(case.rhs, shifts)
    st, ck, post, conv = run_checked(eng, lin, 2, linear=True, st=st, quiet=True)
    assert not conv
    with pytest.raises(nd.Pole):
        st.linear_step(1e-9)
    for _ in range(2):                                                                        # a repeated call raises again, nsigma unchanged
        with pytest.raises(AfespError, match="status 26: .*frequency at a pole: system 0"):
            eng.davidson_test_linear_iterate(1e-9)
        assert eng.davidson_test_fetch("counts") == st.counts() == dict(nsigma=6, ncollapse=0, nb=6, npend=0)
        with pytest.raises(AfespError, match="status 1: .*no coefficients"):                  # (they are those of a smaller basis)
            eng.davidson_test_fetch("y")
    with pytest.raises(AfespError, match="status 1: .*linear mode"):
        eng.davidson_test_iterate(1e-9)
    for k, g in enumerate(case.guesses):                                                      # and back: the same eigenvalue run, to the bit
        eng.davidson_test_set_guess(k, g)
    st, ck, post, conv = run_checked(eng, case, 20, quiet=True)
    assert conv and np.array_equal(post.omega, first.omega) and np.array_equal(post.x, first.x) and np.array_equal(post.resnorm, first.resnorm)


# ---------------------------------------------------------------------------------------------------------------- the promises
def plain_run(e, case, steps):
    start(e, case)
    for _ in range(steps):
        om, res, fl, counts, conv = e.davidson_test_iterate(case.tol)
    return om, res, e.davidson_test_fetch("x"), counts


def test_same_bits_on_every_run(eng):
    """the header of davidson_so.hip: the same input gives the same bits on every run"""
    for case, steps in ((nd.grid_case(70001, 23333, 0.25), 4), (nd.roots_case(600, 9, 18), 5)):
        a, b = plain_run(eng, case, steps), plain_run(eng, case, steps)
        with Engine(0) as other:
            c = plain_run(other, case, steps)
        for u, v, t in zip(a, b, c):
            assert np.array_equal(u, v) and np.array_equal(u, t) if isinstance(u, np.ndarray) else u == v == t


def test_state_lives_beside_the_eom_and_response_states(eng):
    from afesp_amd import density
    from test_gpu_eom import _feed_model
    from test_gpu_response import _converged
    from test_response_cpu import random_symmetric
    c = _converged(5, 2, 2, 72)
    _feed_model(eng, c)
    density.so_lambda_solve(eng, 300, 1e-12, 1e-12)
    ops = np.stack([random_symmetric(np.random.default_rng(5), c["o"] + c["v"]) for _ in range(2)])
    case = nd.grid_case(257, 85, 0.25)

    def eom_run():
        eng.so_eom_init(3, 24)
        eng.so_eom_guess()
        for _ in range(3):
            out = eng.so_eom_iterate(1e-8)
        return out[0], out[1], eng.so_eom_vector(0)[1]

    def resp_run():
        eng.so_response_init(ops, [0.0, 0.05], 16)
        for _ in range(3):
            out = eng.so_response_iterate(1e-8)
        return out[0], eng.so_response_vector(1, 1)[1]

    eng.davidson_test_destroy()                                                               # (a state an earlier test of this module left)
    live0 = eng.arena_stats()["live_gb"]
    hook_alone = plain_run(eng, case, 3)
    eng.davidson_test_destroy()
    assert eng.arena_stats()["live_gb"] == live0
    eom_alone, resp_alone = eom_run(), resp_run()
    # now interleaved: each state's next call comes after the others' calls
    start(eng, case)
    eng.so_eom_init(3, 24)
    eng.so_eom_guess()
    eng.so_response_init(ops, [0.0, 0.05], 16)
    for _ in range(3):
        hook = eng.davidson_test_iterate(case.tol)
        eom_out = eng.so_eom_iterate(1e-8)
        resp_out = eng.so_response_iterate(1e-8)
    got = (hook[0], hook[1], eng.davidson_test_fetch("x"), hook[3])
    for u, v in zip(got, hook_alone):
        assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v
    for u, v in zip((eom_out[0], eom_out[1], eng.so_eom_vector(0)[1]), eom_alone):
        assert np.array_equal(u, v)
    for u, v in zip((resp_out[0], eng.so_response_vector(1, 1)[1]), resp_alone):
        assert np.array_equal(u, v)
    with_states = eng.arena_stats()["live_gb"]
    eng.davidson_test_destroy()
    assert eng.arena_stats()["live_gb"] < with_states
    with pytest.raises(AfespError, match="status 1: .*no Davidson test state"):
        eng.davidson_test_iterate(1e-8)


def test_create_refuses_what_the_unit_cannot_hold(eng):
    d = np.ones(10)
    for args in ((0, 10, 0.25, 0, 3, 5), (11, 10, 0.25, 0, 2, 4), (0, 10, 0.0, 0, 2, 4), (0, 10, 0.25, 0, 0, 4), (0, 10, 0.25, 0, 11, 22)):
        with pytest.raises(AfespError, match="status 1: afesp_test_davidson_create"):
            eng.davidson_test_create(*args, d, None, None, d)
    eng.davidson_test_create(0, 10, 0.25, 0, 2, 4, d, None, None, d)                          # r = 0: a diagonal matrix
    with pytest.raises(AfespError, match="status 1"):
        eng.davidson_test_get_vector(0)                                                       # no Ritz vector before the first step
    eng.davidson_test_destroy()
