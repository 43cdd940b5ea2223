"""The numpy restatement of the block Davidson unit (np_davidson.py) held to dense numpy.linalg.eig / solve on every small case of
tests/test_gpu_davidson.py, the facts those GPU tests rely on pinned case by case -- a case whose restatement does not show its intended
feature is re-seeded HERE, never loosened there -- and the long-double one-step evaluators checked against the float64 restatement within
their own bounds.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import np_davidson as nd
from afesp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXITER = 40


def eigen_cases():
    cs = [nd.grid_case(nvec, n1, w2) for nvec in nd.NVECS if nvec <= 600 for n1, w2 in nd.metrics(nvec)]
    cs += [nd.roots_case(600, nroots, ms) for nroots in (1, 8, 9, 17) for ms in (2 * nroots, 40)]
    cs += [nd.follow_case(False), nd.clamp_case(), nd.drop_case()]
    return cs


def test_linear_start_of_the_clamp_case_clamps_with_each_sign():
    c = nd.LinearCase(600, 3, 3, clamp=True)
    st = c.restatement()
    den = c.shifts[None, :] - c.op.diag[:, None]
    assert 0.0 < den[c.e_pos, 0] < nd.CLAMP and -nd.CLAMP < den[c.e_neg, 2] < 0.0
    assert st.pend[0][c.e_pos] == c.rhs[c.e_pos, 0] / nd.CLAMP and st.pend[2][c.e_neg] == c.rhs[c.e_neg, 2] / -nd.CLAMP
    assert c.rhs[c.e_pos, 0] != 0.0 and c.rhs[c.e_neg, 2] != 0.0
    ref, M = nd.ld_precondition(c.rhs, c.shifts, c.op.diag)
    assert np.all(np.abs(nd._ld(np.array(st.pend).T) - ref) <= nd.tol_factor(1) * M)
    for _ in range(2):                                                              # the two steps of the GPU test stay clear of tol
        assert not st.linear_step(c.tol) and st.resnorm.min() > 1e-6


def linear_cases():
    return [nd.LinearCase(600, nrhs, nroots) for nrhs in (1, 3) for nroots in (3, 12)]


def run_pinned(st, tol, linear=False):
    """to convergence; no residual norm of any step may lie within 5 % of tol (the device's own rounding moves a norm near
    tol by parts in 10^4 at the most, and it must decide as the restatement does)"""
    for it in range(1, MAXITER + 1):
        conv = st.linear_step(tol) if linear else st.step(tol)
        res = st.resnorm[np.isfinite(st.resnorm)]
        assert not np.any((res > tol / 1.05) & (res < tol * 1.05)), (it, res)
        if conv:
            return it
    raise AssertionError("not converged within MAXITER")


def dense_spectrum(op):
    w, v = np.linalg.eig(op.dense())
    order = np.argsort(w.real)
    return w[order], float(np.linalg.cond(v))


@pytest.mark.parametrize("case", eigen_cases(), ids=lambda c: c.name)
def test_restatement_finds_the_lowest_roots_of_dense_eig(case):
    st = case.restatement()
    run_pinned(st, case.tol)
    w, kappa = dense_spectrum(case.op)
    assert np.all(w[:case.nroots + 1].imag == 0.0)
    # kappa(V) resnorm_k, and the dense reference's own error kappa(V) (nvec + 64) 2^-53 |A|_2
    bound = kappa * st.resnorm + kappa * nd.tol_factor(case.op.nvec) * np.linalg.norm(case.op.dense(), 2)
    assert np.all(np.abs(st.omega - w[:case.nroots].real) <= bound), (st.omega, w[:case.nroots], bound)
    if case.ms == 2 * case.nroots and case.op.nvec > 7:
        assert st.ncollapse >= 1
    if case.ms == 40 and case.nroots <= 9:
        assert st.ncollapse == 0


def large_cases():
    """(case, steps of its GPU run, linear)"""
    cs = [(nd.grid_case(nvec, n1, w2), 4, False) for nvec in nd.NVECS if nvec > 600 for n1, w2 in nd.metrics(nvec)]
    cs += [(nd.roots_case(32769, nroots, ms), 4 if nroots > 1 else 6, False) for nroots in (1, 8, 9, 17) for ms in (2 * nroots, 40)]
    cs += [(nd.LinearCase(32769, nrhs, nroots), 3, True) for nrhs in (1, 3) for nroots in (3, 12)]
    return cs


@pytest.mark.parametrize("case,steps,linear", large_cases(), ids=lambda c: getattr(c, "name", None))
def test_large_cases_collapse_within_their_steps_and_stay_clear_of_tol(case, steps, linear):
    """above nvec = 600 the GPU tests run a fixed number of steps; the restatement shows that these hold a collapse, that no residual norm
    comes near tol, and that the lowest vector has an entry of unit size in the last element"""
    st = case.restatement()
    for it in range(steps):
        conv = st.linear_step(case.tol) if linear else st.step(case.tol)
        res = st.resnorm[np.isfinite(st.resnorm)]
        assert not np.any((res > case.tol / 1.05) & (res < case.tol * 1.05)), (it, res)
        if conv:
            break
    if case.ms == 2 * case.nroots:
        assert st.ncollapse >= 1
    assert linear or abs(st.x[-1, 0]) > 0.5


PINS = {   # name: (steps, collapses) of the named cases
    "follow-1": (5, 0), "follow-0": (6, 0), "clamp": (5, 1), "drop": (6, 3),
    "linear-600-1-3": (5, 3), "linear-600-1-12": (4, 2), "linear-600-3-3": (5, 3), "linear-600-3-12": (4, 2),
}


@pytest.mark.parametrize("case", [nd.follow_case(True), nd.follow_case(False), nd.clamp_case(), nd.drop_case()] + linear_cases(), ids=lambda c: c.name)
def test_step_and_collapse_counts_of_the_named_cases(case):
    linear = isinstance(case, nd.LinearCase)
    st = case.restatement()
    assert (run_pinned(st, case.tol, linear), st.ncollapse) == PINS[case.name]


def test_followed_roots_are_not_the_lowest():
    c1, c0 = nd.follow_case(True), nd.follow_case(False)
    w, kappa = dense_spectrum(c1.op)
    s1, s0 = c1.restatement(), c0.restatement()
    run_pinned(s1, c1.tol)
    run_pinned(s0, c0.tol)
    assert np.allclose(s1.omega, w[[5, 6]].real, atol=1e-8, rtol=0) and s1.features["selected_not_lowest"] > 0
    assert s1.omega.min() > w[c1.nroots - 1].real + 0.1              # not among the lowest nroots
    assert np.allclose(s0.omega, w[[0, 1]].real, atol=1e-8, rtol=0) and s0.features["selected_not_lowest"] == 0
    # the lower roots did enter the following state's basis: its projected matrix has roots below the ones it keeps
    assert np.sort(np.linalg.eigvals(s1.G).real)[0] < w[1].real + 1e-3


def test_following_with_a_dropped_guess_has_fewer_targets_than_roots():
    """the branch `k >= nt` of the selection: two targets, three roots, and the third place goes to the lowest root not yet taken"""
    c = nd.follow_drop_case()
    w, kappa = dense_spectrum(c.op)
    st = c.restatement()
    assert not st.step(c.tol)
    assert st.features["dropped"] == 1 and st.nb == 2 and len(st.target) == 2 and np.isinf(st.resnorm[2])
    seen = 0
    for it in range(2, MAXITER):
        conv = st.step(c.tol)
        wr = np.sort(np.linalg.eigvals(st.G).real)
        assert st.nb > 3 and len(st.target) == 2 < len(st.sel) == 3                   # fewer targets than roots at a step with nb > nr
        near = [int(np.argmin(np.abs(wr - t))) for t in st.target]
        assert st.sel == sorted(near + [min(set(range(st.nb)) - set(near))])         # the nearest to each target, then the lowest not taken
        assert st.sel[0] == 0 and st.sel[1] > 1
        seen += 1
        if conv:
            break
    assert conv and seen >= 3 and (it, st.ncollapse) == (6, 0)
    assert np.allclose(st.omega, w[[0, 5, 6]].real, atol=1e-8, rtol=0)


def test_clamp_case_clamps_with_each_sign():
    c = nd.clamp_case()
    st = c.restatement()
    st.step(c.tol)
    den = st.omega[0] - c.op.diag
    assert 0.0 < den[c.e_pos] < nd.CLAMP and -nd.CLAMP < den[c.e_neg] < 0.0
    assert (st.features["clamp_pos"], st.features["clamp_neg"]) == (1, 1)
    assert st.corr[c.e_pos, 0] == st.rho[c.e_pos, 0] / nd.CLAMP and st.corr[c.e_neg, 0] == st.rho[c.e_neg, 0] / -nd.CLAMP
    assert abs(st.rho[c.e_pos, 0]) > 1e-6 and abs(st.rho[c.e_neg, 0]) > 1e-6        # (a clamp that divides zero would show nothing)


def test_drop_case_drops_the_dependent_and_the_zero_guess():
    c = nd.drop_case()
    st = c.restatement()
    st.step(c.tol)
    assert st.features["dropped"] == 2 and st.nb == 2 and st.nsigma == 2
    assert np.all(np.isinf(st.resnorm[2:])) and len(st.pend) == 2
    z = nd.Restatement(c.op, c.n1, c.w2, c.nroots, c.ms)
    z.set_guess(1, np.zeros(c.op.nvec))
    with pytest.raises(nd.Vanished):
        z.step(c.tol)


def test_complex_pair_among_the_lowest_roots():
    c = nd.complex_case()
    A = c.op.dense()
    w, kappa = dense_spectrum(c.op)
    assert w[0].imag != 0.0 and w[1] == np.conj(w[0]) and w[2].imag == 0.0 and w[2].real > w[0].real + 0.5
    for eig in (nd.numpy_eig, nd.library_eig):
        st = c.restatement(eig)
        for it in range(1, 25):
            nb0 = st.nb
            assert not st.step(c.tol)                                           # the real part of a complex vector is no eigenvector
            assert np.all(st.flags == nd.FLAG_COMPLEX) and st.omega[0] == st.omega[1]
            assert np.array_equal(st.x[:, 0], st.x[:, 1])
            assert st.nb == (2 if it == 1 else min(nb0 + 1, 24)) and len(st.pend) == 2   # the duplicate correction is dropped
        assert st.nb == 24 and st.ncollapse == 0
        assert abs(st.omega[0] - w[0].real) <= kappa * nd.tol_factor(24) * np.linalg.norm(A, 2)


@pytest.mark.parametrize("case", linear_cases(), ids=lambda c: c.name)
def test_linear_restatement_matches_dense_solve(case):
    st = case.restatement()
    run_pinned(st, case.tol, linear=True)
    assert st.ncollapse >= 1
    A, n = case.op.dense(), case.op.nvec
    for j in range(case.nroots):
        m = A - case.shifts[j] * np.eye(n)
        x = np.linalg.solve(m, -case.rhs[:, j % case.rhs.shape[1]])
        # |x - x*|_2 <= |m^-1|_2 |rho|_2, |rho|_2 <= |rho|_W / sqrt(min w); the dense solve's own error: cond 2^-53 |x| with a factor n
        smin = np.linalg.svd(m, compute_uv=False)[-1]
        bound = st.resnorm[j] / np.sqrt(st.w.min()) / smin + n * np.linalg.cond(m) * nd.EPS53 * np.linalg.norm(x)
        assert np.linalg.norm(x - st.x[:, j]) <= bound, (j, np.linalg.norm(x - st.x[:, j]), bound)


def test_pole_after_an_eigenvalue_run_and_back():
    c = nd.pole_case()
    st = c.restatement()
    assert nd.run(st, c.tol, 20) == 4 and st.nb == 7
    w, _ = dense_spectrum(c.op)
    assert abs(st.omega[0] - w[0].real) < 1e-13
    st.linear_start(c.rhs, [st.omega[0], c.other_shift])
    assert not st.linear_step(1e-9) and not st.linear_step(1e-9)
    for _ in range(2):                                                          # a repeated call raises again, nothing is built
        with pytest.raises(nd.Pole):
            st.linear_step(1e-9)
        assert st.counts() == dict(nsigma=6, ncollapse=0, nb=6, npend=0)
    for k, g in enumerate(c.guesses):                                           # and back to the eigenvalue mode
        st.set_guess(k, g)
    assert nd.run(st, c.tol, 20) == 4


def checked_run(case, linear=False, eig=nd.numpy_eig, maxiter=MAXITER):
    st = case.restatement() if linear else case.restatement(eig)
    ck = nd.StepChecker(case.op, case.n1, case.w2, case.nroots, case.ms, eig)
    for it in range(maxiter):
        pre = nd.snapshot_restatement(st)
        conv = st.linear_step(case.tol) if linear else st.step(case.tol)
        got = ck.step(pre, nd.snapshot_restatement(st), case.tol, linear, case.rhs if linear else None, case.shifts if linear else None,
                      False if linear else case.follow)
        assert got == conv
        if conv:
            break
    return ck


@pytest.mark.parametrize("case", [nd.grid_case(7, 2, 0.25), nd.grid_case(257, 3, 0.5), nd.grid_case(600, 600, 1.0), nd.roots_case(600, 9, 18),
                                  nd.roots_case(600, 17, 40), nd.follow_case(True), nd.clamp_case(), nd.drop_case(), nd.grid_case(32769, 0, 0.25)],
                         ids=lambda c: c.name)
def test_long_double_evaluators_bound_the_float64_restatement(case):
    ck = checked_run(case)
    assert {"a new B", "b new S = A b", "c G columns", "e x = B y", "e corr", "e resnorm"} <= set(ck.ratios)
    if case.ms == 2 * case.nroots:
        assert "b collapse S = A B" in ck.ratios


def test_long_double_evaluators_in_the_complex_and_linear_cases():
    ck = checked_run(nd.complex_case(), eig=nd.library_eig, maxiter=25)
    assert "d pair subspace" in ck.ratios
    ck = checked_run(nd.LinearCase(600, 3, 12), linear=True)
    assert {"c prhs", "d LU residual", "b collapse S = A B"} <= set(ck.ratios)


def test_step_checker_sees_a_wrong_weight_a_lost_tail_and_a_wrong_chunk():
    """the checker itself: a state changed the way a wrong kernel would change it does not pass"""
    case = nd.grid_case(600, 200, 0.25)
    st = case.restatement()
    st.step(case.tol)
    pre = nd.snapshot_restatement(st)
    st.step(case.tol)
    post = nd.snapshot_restatement(st)

    def fresh():
        ck = nd.StepChecker(case.op, case.n1, case.w2, case.nroots, case.ms)
        ck.sbound = np.zeros((600, pre.B.shape[1]))
        return ck
    fresh().step(pre, post, case.tol)
    bad = nd.snapshot_restatement(st)
    bad.G = (bad.B.T @ bad.S).copy()                                            # w2 taken as 1 behind n1
    bad.G[:3, :3] = pre.G
    with pytest.raises(AssertionError, match="c G"):
        fresh().step(pre, bad, case.tol)
    bad = nd.snapshot_restatement(st)
    bad.x = bad.x.copy()
    bad.x[-1, 2] = 0.0                                                          # the last element of the last root lost
    with pytest.raises(AssertionError, match="e x = B y"):
        fresh().step(pre, bad, case.tol)
    bad = nd.snapshot_restatement(st)
    bad.B = bad.B.copy()
    bad.B[:, 4] += 1e-9 * bad.B[:, 0]                                           # a projection coefficient off in its ninth digit
    with pytest.raises(AssertionError, match="a new B"):
        fresh().step(pre, bad, case.tol)


def test_hook_is_declared_exported_and_refuses_a_null_context():
    names = ("afesp_test_davidson_create", "afesp_test_davidson_destroy", "afesp_test_davidson_set_guess", "afesp_test_davidson_iterate",
             "afesp_test_davidson_linear_start", "afesp_test_davidson_linear_iterate", "afesp_test_davidson_get_vector", "afesp_test_davidson_fetch")
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "afesp.h")).read()
    for s in names:
        assert s in capi.EXPORTS and f"int {s}(afesp_ctx* ctx" in header and hasattr(lib, s)
    assert lib.afesp_test_davidson_destroy(None) == 1
    assert lib.afesp_test_davidson_iterate(None, ctypes.c_double(1e-8), np.zeros(1), np.zeros(1), None, None, None) == 1
