"""The complex linear mode of the block Davidson unit (csrc/davidson_so.hip: davidson_linear_start_complex, davidson_cfused_kernel) run
directly, through the test entry afesp_test_davidson_*, on matrices given as data (A = diag(d) + U V^T, np_davidson.generate) and held
step by step against the float64 restatement np_response_complex.ComplexLinear of the same run.

Per step: the counts {sigma builds, collapses, basis vectors, pending vectors} are equal, the convergence decision is the same, x agrees
within 1e-3 of the residual norm (in the unit's metric, per system), the residual norms within 1e-3 relative -- the bound
test_gpu_response.py holds the real mode to --, and |B^T W B - 1| < 1e-12.  The shapes are the smallest at which the fused pass can go
wrong: one element; 257 elements (one block and one element of a second) with every split of the metric; 5000 (twenty blocks of
partials); one system more than the kernel's chunk of 8, and 11 (no multiple of it); gamma = 0 and gamma != 0 systems side by side;
max_space = 4 nsys, the least the unit takes, so that it collapses.  The restatement is checked to collapse and to converge on every
case, and no residual of it may lie within 5 % of tol, where the two could decide differently.

The bound on x is relative to the residual, so it means something only while 1e-3 |rho| is above what two fp64 evaluations of x = B y
can differ by (1e-15 or so for |x| of order one): the runs stop at tol = 2e-6 and 5e-7, where the smallest residual any step of them
compares at is 3e-9 (bound on x: 3e-12).  The two cases whose residual is at rounding level from the first step -- one element, and
the two-dimensional damped solve -- are held to their exact solutions instead.

How far two correct runs can differ was measured with the restatement against itself, the sigma vectors of one run perturbed by
1e-16 relative: a collapse orthonormalises solutions that are nearly dependent (many shifts, three right-hand sides), the vectors it
keeps are scaled up from norms as small as DROP, and the difference of x then reaches 1e-6 .. 6e-2 of the residual depending on the
case.  The cases here are those where that figure is 3e-5 or below, a fortieth of the bound: 257 elements at coupling 1.0 with two
collapses (5e-6 .. 3e-5 over five perturbations), and 5000 elements at coupling 0.2, which converges in two steps without a collapse
(4e-6; at coupling 0.6 it collapses and the perturbed restatement itself is 6e-2 of the residual off).  Seen on an MI355X: |x - x_np| / |rho| at most 3.8e-5, |res / res_np - 1| at most 1.3e-5 (257
elements, after the second collapse), |B^T W B - 1| at most 1e-15."""
import numpy as np
import pytest

import np_davidson as nd
import np_response_complex as npc
from afesp_amd.capi import AfespError, Engine

pytestmark = pytest.mark.gpu

TOL = 2e-6
GAMMAS = np.array([0.0, 0.05, 0.0, 0.1, 0.02, 0.0, 0.3, 0.05, 1.0, 0.0, 0.2])


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def make_case(nvec, nsys, nrhs=3, seed=5, coupling=1.0):
    """-> (operator, rhs (nvec, nrhs), complex shifts): real parts alternate in sign and reach into the spectrum (lowest diagonal elements
    0.5, 0.6, ...) where gamma > 0; the gamma = 0 systems stay below it; system 1 is purely imaginary"""
    op, places = nd.generate(nvec, r=4, seed=seed, coupling=coupling)
    rng = np.random.default_rng(400 + nvec + nsys)
    nrhs = min(nrhs, nsys)
    rhs = 0.05 * rng.standard_normal((nvec, nrhs))
    rhs[places[:nrhs], np.arange(nrhs)] += 1.0
    rhs[-1, :] += 0.5
    om = np.linspace(-0.3, 0.9, nsys) * np.where(np.arange(nsys) % 2, 1.0, -1.0)
    ga = GAMMAS[:nsys].copy()
    om[1] = 0.0
    om = np.where(ga == 0.0, np.clip(om, -0.35, 0.35), om)
    return op, rhs, om + 1j * ga


def start(eng, op, n1, w2, rhs, zs, ms):
    eng.davidson_test_create(n1, op.nvec, w2, False, len(zs), ms, op.d, op.U, op.V, op.diag)
    eng.davidson_test_linear_start_complex(rhs, zs)


def wnorm(w, x):
    return float(np.sqrt(np.sum(w * (x.real ** 2 + x.imag ** 2))))


def run_checked(eng, op, n1, w2, rhs, zs, ms, tol=TOL, maxsteps=40, tag=""):
    """the device and the restatement side by side -> (restatement, the device's x, resnorm, steps)"""
    w = nd.weights(n1, op.nvec, w2)
    st = npc.ComplexLinear(op.apply, op.diag, w, rhs, zs, ms)
    start(eng, op, n1, w2, rhs, zs, ms)
    assert eng.davidson_test_fetch("counts") == st.counts()
    pend = eng.davidson_test_fetch("pend")
    for j, z in enumerate(zs):
        if z.imag == 0.0:
            assert not np.any(pend[:, 2 * j + 1])                           # an exactly zero imaginary vector
        assert np.max(np.abs(pend[:, 2 * j] - st.pend[2 * j])) <= 1e-12 * np.max(np.abs(st.pend[2 * j]))
        assert np.max(np.abs(pend[:, 2 * j + 1] - st.pend[2 * j + 1])) <= 1e-12 * max(np.max(np.abs(st.pend[2 * j + 1])), 1e-300)
    worst = dict(x=0.0, res=0.0, orth=0.0)
    for it in range(1, maxsteps + 1):
        conv_ref = st.step(tol)
        assert not np.any((st.resnorm > tol / 1.05) & (st.resnorm < tol * 1.05)), "the case is too close to tol: re-seed it"
        res, fl, counts, conv = eng.davidson_test_linear_iterate(tol)
        assert counts == st.counts(), (it, counts, st.counts())
        assert conv == conv_ref and np.array_equal(fl != 0, st.resnorm < tol)
        x = eng.davidson_test_fetch("x")
        B = eng.davidson_test_fetch("B")
        orth = float(np.max(np.abs((B * w[:, None]).T @ B - np.eye(B.shape[1]))))
        for j in range(len(zs)):
            ex, er = wnorm(w, x[:, j] - st.x[:, j]) / st.resnorm[j], abs(res[j] / st.resnorm[j] - 1.0)
            worst["x"], worst["res"] = max(worst["x"], ex), max(worst["res"], er)
        worst["orth"] = max(worst["orth"], orth)
        print(f"  {tag} step {it}: counts {counts}, |x - x_np| / |rho| {max(wnorm(w, x[:, j] - st.x[:, j]) / st.resnorm[j] for j in range(len(zs))):.2e}, "
              f"|res / res_np - 1| {np.max(np.abs(res / st.resnorm - 1.0)):.2e}, |B^T W B - 1| {orth:.2e}")
        for j in range(len(zs)):
            assert wnorm(w, x[:, j] - st.x[:, j]) <= 1e-3 * st.resnorm[j]
        assert np.all(np.abs(res / st.resnorm - 1.0) < 1e-3)
        assert orth < 1e-12
        # the pending vectors: two per unconverged system, the imaginary one of a gamma = 0 system exactly zero (it is dropped next step)
        pend = eng.davidson_test_fetch("pend")
        open_ = [j for j in range(len(zs)) if not st.resnorm[j] < tol]
        assert pend.shape[1] == 2 * len(open_)
        for k, j in enumerate(open_):
            if zs[j].imag == 0.0:
                assert not np.any(pend[:, 2 * k + 1]) and not np.any(x[:, j].imag)
        if conv:
            break
    print(f"{tag}: {it} steps, {st.counts()}, dropped {st.dropped}, largest |x - x_np| / |rho| {worst['x']:.2e}, |res / res_np - 1| {worst['res']:.2e}, "
          f"|B^T W B - 1| {worst['orth']:.2e}")
    return st, x, res, it


def check_dense(op, w, rhs, zs, x, res):
    """|x - x*|_2 <= |rho|_2 / sigma_min(A - z), |rho|_2 <= |rho|_W / sqrt(min w); and the dense solve's own error"""
    A, n = op.dense(), op.nvec
    for j, z in enumerate(zs):
        m = A - z * np.eye(n)
        ref = np.linalg.solve(m, -rhs[:, j % rhs.shape[1]].astype(complex))
        smin = np.linalg.svd(m, compute_uv=False)[-1]
        bound = res[j] / np.sqrt(w.min()) / smin + n * np.linalg.cond(m) * nd.EPS53 * np.linalg.norm(ref)
        assert np.linalg.norm(x[:, j] - ref) <= bound, (j, z)


def test_one_element(eng):
    op = nd.Operator(np.array([0.7]))
    rhs, zs = np.array([[1.0]]), np.array([0.2 + 0.1j])
    st = npc.ComplexLinear(op.apply, op.diag, nd.weights(0, 1, 0.25), rhs, zs, 4)
    assert st.step(TOL) and st.counts() == dict(nsigma=1, ncollapse=0, nb=1, npend=0) and st.dropped == 1   # Im is parallel to Re: dropped
    start(eng, op, 0, 0.25, rhs, zs, 4)
    assert eng.davidson_test_fetch("counts") == dict(nsigma=0, ncollapse=0, nb=0, npend=2)
    res, fl, counts, conv = eng.davidson_test_linear_iterate(TOL)
    assert conv and counts == st.counts() and res[0] < 1e-14               # (a few roundings of numbers of order one)
    x = eng.davidson_test_fetch("x")
    assert x.shape == (1, 1) and abs(x[0, 0] - (-1.0 / (0.7 - zs[0]))) < 1e-14


@pytest.mark.parametrize("n1", [0, 100, 257])
def test_257_elements_nine_systems_every_metric_split(eng, n1):
    """one system more than the kernel's chunk; gamma = 0 and gamma != 0 mixed; max_space = 4 nsys: it collapses"""
    op, rhs, zs = make_case(257, 9)
    st, x, res, it = run_checked(eng, op, n1, 0.25, rhs, zs, 36, tag=f"nvec 257 n1 {n1}")
    assert st.ncollapse >= 1 and np.all(st.resnorm < TOL) and st.dropped >= 4
    check_dense(op, nd.weights(n1, 257, 0.25), rhs, zs, x, res)


def test_5000_elements_eleven_systems(eng):
    """twenty blocks of partials and a ragged last one; 11 systems: a whole chunk and a rest of three.  Two steps, no collapse (see the
    module docstring: the collapse is checked at 257 elements)"""
    op, rhs, zs = make_case(5000, 11, coupling=0.2)
    st, x, res, it = run_checked(eng, op, 1666, 0.25, rhs, zs, 44, tol=5e-7, tag="nvec 5000")
    assert it == 2 and np.all(st.resnorm < 5e-7)
    assert abs(x[-1, 0]) > 0.1                                               # an entry of size one in the last element


def plain_run(e, op, rhs, zs, steps):
    start(e, op, 1666, 0.25, rhs, zs, 44)
    for _ in range(steps):
        res, fl, counts, conv = e.davidson_test_linear_iterate(TOL)
    return res, e.davidson_test_fetch("x"), e.davidson_test_fetch("corr"), counts


def test_same_bits_on_every_run(eng):
    op, rhs, zs = make_case(5000, 11, coupling=0.2)
    a, b = plain_run(eng, op, rhs, zs, 2), plain_run(eng, op, rhs, zs, 2)
    for u, v in zip(a, b):
        assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v


def test_a_real_shift_at_a_pole_is_status_26_and_a_damped_one_converges(eng):
    """a diagonal A, a right-hand side on two of its elements: after two steps the basis spans both, the projected matrix has the
    diagonal entry itself as a root and the undamped system at that entry is singular; with gamma = 1e-3 nothing is"""
    nvec, k, m = 257, 40, 60
    d = np.linspace(0.5, 4.0, nvec)
    op = nd.Operator(d)
    rhs = np.zeros((nvec, 1))
    rhs[k, 0] = rhs[m, 0] = 1.0
    w = nd.weights(100, nvec, 0.25)
    st = npc.ComplexLinear(op.apply, op.diag, w, rhs, [d[k] + 0.0j], 4)
    assert not st.step(TOL)
    with pytest.raises(npc.Pole):
        st.step(TOL)
    start(eng, op, 100, 0.25, rhs, [d[k] + 0.0j], 4)
    res, fl, counts, conv = eng.davidson_test_linear_iterate(TOL)
    assert not conv and counts == dict(nsigma=1, ncollapse=0, nb=1, npend=2)
    for _ in range(2):                                                       # a repeated call raises again
        with pytest.raises(AfespError, match="status 26: .*frequency at a pole: system 0"):
            eng.davidson_test_linear_iterate(TOL)
        assert eng.davidson_test_fetch("counts") == dict(nsigma=2, ncollapse=0, nb=2, npend=0)
    zs = np.array([d[k] + 1e-3j])
    st = npc.ComplexLinear(op.apply, op.diag, w, rhs, zs, 4)
    assert st.step(TOL) and st.counts() == dict(nsigma=2, ncollapse=0, nb=2, npend=0)   # Re and Im span both elements: an exact solve
    start(eng, op, 100, 0.25, rhs, zs, 4)
    res, fl, counts, conv = eng.davidson_test_linear_iterate(TOL)
    assert conv and counts == st.counts()
    x = eng.davidson_test_fetch("x")
    check_dense(op, w, rhs, zs, x, res)
    assert abs(x[k, 0] + 1000.0j) < 1e-9 and abs(x[m, 0] + 1.0 / (d[m] - zs[0])) < 1e-13   # -1 / (d_k - z) = 1 / (i gamma) = -1000 i


def test_the_state_goes_back_to_the_real_modes_and_refuses_what_it_cannot_hold(eng):
    case = nd.LinearCase(600, 3, 3, ms=12)
    eng.davidson_test_create(case.n1, 600, case.w2, False, 3, 12, case.op.d, case.op.U, case.op.V, case.op.diag)
    eng.davidson_test_linear_start(case.rhs, case.shifts)
    real = [eng.davidson_test_linear_iterate(case.tol) for _ in range(3)][-1]
    xr = eng.davidson_test_fetch("x")
    eng.davidson_test_linear_start_complex(case.rhs, case.shifts + 0.0j)      # gamma = 0 throughout: the real solutions
    for _ in range(3):
        cplx = eng.davidson_test_linear_iterate(case.tol)
    xc = eng.davidson_test_fetch("x")
    assert xc.shape == (600, 3) and not np.any(xc.imag)
    assert cplx[2]["nsigma"] == real[2]["nsigma"] and np.max(np.abs(xc.real - xr)) < 1e-3 * np.max(real[0])
    eng.davidson_test_linear_start(case.rhs, case.shifts)                     # back on the widened state: the same bits as before
    again = [eng.davidson_test_linear_iterate(case.tol) for _ in range(3)][-1]
    assert np.array_equal(again[0], real[0]) and np.array_equal(eng.davidson_test_fetch("x"), xr) and eng.davidson_test_fetch("x").shape == (600, 3)
    eng.davidson_test_create(case.n1, 600, case.w2, False, 3, 11, case.op.d, case.op.U, case.op.V, case.op.diag)
    with pytest.raises(AfespError, match="status 1: .*4 nroots <= max_space"):
        eng.davidson_test_linear_start_complex(case.rhs, case.shifts + 0.0j)
    eng.davidson_test_destroy()
