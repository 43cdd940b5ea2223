"""GPU parity of the left-hand side of EOM-EE-CCSD on the spin-orbital state (afesp_ccsd_so_eom_lsigma, _left_*, _ref_coupling, _density;
afesp_amd.eom): the left sigma build against A^T of the complex-step Jacobian at the shapes of tests/test_gpu_lambda.py and against the
GPU's own right-hand build, that nothing else is written, the left Davidson iteration on the four converged models of np_eom.MODELS,
the bilinear density against the central difference in f, FCI densities and transition moments for two electrons through the Python
drivers, and the statuses.

Tolerances: 1e-11 x max(1, max |ref|) for sigma and the density at equal amplitudes; 1e-12 x max(1, |<l, sigma(r)>|) for
the adjoint identity between the two device builds; 1e-8 for omega at tol = 1e-8; 10 tol for the residual norm recomputed from the
returned vectors; 1e-9 against FCI.

Not covered here: a recording context (Context::rec) is refused by every entry point as by the right-hand ones, but no call of the C
interface leaves a context recording, so the refusal cannot be reached from a test."""
import numpy as np
import pytest

import np_eom
import np_eom_left
import np_lambda
from afesp_amd import density, eom
from afesp_amd.capi import AfespError
from test_eom_left_cpu import check_two_electron_properties, two_electron_case
from test_gpu_eom import _antisymmetric_to_the_bit, _feed_model
from test_gpu_lambda import SHAPES, _build_case, _case, _close, _feed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_left_sigma_equals_the_transposed_jacobian_at_random_amplitudes(eng, name):
    """sigma_L(l) = A^T l at O(0.3) random t and l, and <l, sigma(r)> = <sigma_L(l), r> against the right-hand build"""
    c = _case(name)
    cc, o, v = c["cc"], c["o"], c["v"]
    rng = np.random.default_rng(29)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    ls = [np_lambda.antisym_random(rng, o, v) for _ in range(3)]
    r1, r2 = np_lambda.antisym_random(rng, o, v)
    _, A = np_lambda.jacobian(cc, t1, t2)
    _feed(eng, c)
    eng.so_set_amplitudes(t1, t2)
    eng.so_lambda_init(0)
    s1, s2 = eng.so_eom_lsigma(np.stack([l[0] for l in ls]), np.stack([l[1] for l in ls]))      # nvec = 3 in one call
    q1, q2 = eng.so_eom_sigma(r1, r2)
    for k, (l1, l2) in enumerate(ls):
        d1, d2 = np_eom_left.lsigma_definition(cc, t1, t2, l1, l2, A)
        _close(s1[k], d1, 1e-11, f"{name} left sigma1 of vector {k}")
        _close(s2[k], d2, 1e-11, f"{name} left sigma2 of vector {k}")
        assert _antisymmetric_to_the_bit(s2[k])
        assert not np.any(s2[k][np.arange(o), np.arange(o)]) and not np.any(s2[k][:, :, np.arange(v), np.arange(v)])
        a1, a2 = eng.so_eom_lsigma(l1, l2)                                  # ... equals three calls bit for bit
        assert np.array_equal(a1, s1[k]) and np.array_equal(a2, s2[k])
        lhs, rhs = np_eom.dot(l1, l2, q1, q2), np_eom.dot(s1[k], s2[k], r1, r2)
        print(name, "adjoint", lhs, rhs, "error", abs(lhs - rhs))
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    if o == 1:
        assert not np.any(s2)
    a1, a2 = eng.so_amplitudes()
    assert np.array_equal(a1, t1) and np.array_equal(a2, t2)


def test_a_lambda_iteration_is_the_same_after_left_calls(eng):
    """lambda, l2_old, X, G_vv / G_oo, the DIIS ring and the pseudo energy are the Lambda state's: a left sigma build, a density call and
    left Davidson steps in between leave the next iteration's bits as they were"""
    c = _case("uhf_fed")
    o, v = c["o"], c["v"]
    rng = np.random.default_rng(31)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    l = np_lambda.antisym_random(rng, o, v)
    x, r = np_lambda.antisym_random(rng, o, v), np_lambda.antisym_random(rng, o, v)
    _feed(eng, c)
    eng.so_set_amplitudes(t1, t2)
    runs = []
    for with_left_calls in (False, True):
        eng.so_lambda_init(8)
        eng.so_set_lambda(*l)
        first = eng.so_lambda_iterate(1e-11, 1e-11)
        if with_left_calls:
            eng.so_eom_lsigma(*x)
            eng.so_eom_density(0.7, x, -0.4, r)
            eng.so_eom_ref_coupling(*r)
            eng.so_eom_left_init(2, 8)
            eng.so_eom_left_guess()
            eng.so_eom_left_iterate(1e-8)
            eng.so_eom_left_iterate(1e-8)
        second = eng.so_lambda_iterate(1e-11, 1e-11)
        runs.append((first[:2], second[:2], *eng.so_lambda(), eng.so_density()))
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_a_left_solve_changes_nothing_else(eng):
    c = _case("uhf_fed")
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    e_t = eng.do_ccsd_t_spinorb()
    density.so_lambda_solve(eng, 300, 1e-11, 1e-11)
    omega, R, info = eom.so_eom_solve(eng, 3)
    before = (*eng.so_amplitudes(), *eng.so_lambda(), eng.so_density(), *[x for k in range(3) for x in eng.so_eom_vector(k)])
    wl, L, linfo = eom.so_eom_left_solve(eng, R)
    assert np.max(np.abs(wl - omega)) < 1e-7 and linfo["nsigma"] >= 3
    eng.so_eom_density(0.0, L[0], 0.1, R[0])
    after = (*eng.so_amplitudes(), *eng.so_lambda(), eng.so_density(), *[x for k in range(3) for x in eng.so_eom_vector(k)])
    for a, b in zip(before, after):
        assert np.array_equal(a, b)                                         # t1, t2, l1, l2, the density, the right vectors: bit for bit
    again = eng.so_eom_iterate(1e-8)                                        # the right-hand state is live: its roots as they were
    assert np.array_equal(again[0], omega) and again[3] == info["nsigma"] and again[4]
    assert eng.do_ccsd_t_spinorb() == e_t
    eng.so_lambda_iterate(1e-11, 1e-11)                                     # ... and the Lambda state is still live


def _left_residual_norms(eng, omega, vectors):
    out = []
    for w, (x1, x2) in zip(omega, vectors):
        s1, s2 = eng.so_eom_lsigma(x1, x2)
        out.append(np.sqrt(np_eom.dot(s1 - w * x1, s2 - w * x2, s1 - w * x1, s2 - w * x2)))
    return np.array(out)


@pytest.mark.parametrize("name", sorted(np_eom.MODELS))
@pytest.mark.parametrize("nroots", [4, 6])
def test_left_davidson_finds_the_lowest_roots_of_the_jacobian(eng, name, nroots):
    c = np_eom.converged_model(name)
    ref = c["w"][:nroots].real
    _feed_model(eng, c)
    tol = 1e-8
    omega_r, R, _ = eom.so_eom_solve(eng, nroots, tol=tol, maxiter=300)
    runs = []
    # Twice from the right vectors with a space so small that the collapse runs, then from the unit guesses with the default space.
    # (Unit guesses AND max_space = 4 nroots is left out: on o4v6_canonical with 4 roots, where roots 4 and 5 lie 3e-3 Eh apart, the
    # reference iteration of np_eom.davidson cycles under these rules -- root 4 stays at |rho| ~ 2e-3 for 3000 steps -- and so does the
    # device's; DESIGN.md 4.16.  The right-hand iteration needs 87 steps there.)
    for max_space, guess in ((4 * nroots, R), (4 * nroots, R), (None, None)):
        omega, vectors, info = eom.so_eom_left_solve(eng, guess, nroots, tol=tol, max_space=max_space, maxiter=300)
        print(name, nroots, "max_space", info["max_space"], info["iterations"], "steps", info["nsigma"], "left sigma builds, omega error",
              np.max(np.abs(omega - ref)), "against the right roots", np.max(np.abs(omega - omega_r)))
        assert np.max(np.abs(omega - ref)) < 1e-8 and np.max(np.abs(omega - omega_r)) < 1e-8
        assert not info["complex"] and np.all(info["flags"] & eom.FLAG_CONVERGED)
        res = _left_residual_norms(eng, omega, vectors)
        print(name, nroots, "recomputed residual norms", res)
        assert np.all(res < 10.0 * tol)
        for x1, x2 in vectors:
            assert abs(np_eom.dot(x1, x2, x1, x2) - 1.0) < 1e-12 and _antisymmetric_to_the_bit(x2)
        runs.append((omega, vectors, info))
    assert runs[0][2]["nsigma"] > 4 * nroots                                # more sigma builds than basis vectors fit: it collapsed
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][2]["nsigma"] == runs[1][2]["nsigma"]
    for (a1, a2), (b1, b2) in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2)            # a second run: identical bits
    L = eom.biorthonormalise(runs[2][0], runs[2][1], R)
    S = np.array([[eom.dot(l, r) for r in R] for l in L])
    print(name, nroots, "biorthonormality", np.max(np.abs(S - np.eye(nroots))))
    assert np.max(np.abs(S - np.eye(nroots))) < 1e-5                        # (off the clusters: |rho| / gap of two solves at tol = 1e-8)


@pytest.mark.parametrize("name", ["uhf_fed", "fock_rotated", "two_electron", "one_electron"])
def test_density_equals_the_central_difference_in_f(eng, name):
    """(o,v) = (4,6) with unequal spins, (3,5) with every f term, (2,2) and (1,5) -- the last with an empty pair space"""
    c = _case(name)
    cc, o, v = c["cc"], c["o"], c["v"]
    rng = np.random.default_rng(37)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    l, r = np_lambda.antisym_random(rng, o, v), np_lambda.antisym_random(rng, o, v)
    _feed(eng, c)
    eng.so_set_amplitudes(t1, t2)
    eng.so_lambda_init(0)
    for what, (l0, lv, r0, rv) in {"random": (0.7, l, -0.4, r), "no right vector": (0.9, l, 1.1, None), "no left vector": (1.3, None, 0.6, r),
                                   "no vector": (1.2, None, -0.8, None), "excited state": (0.0, l, 0.3, r)}.items():
        d = eng.so_eom_density(l0, lv, r0, rv)
        _close(d, np_eom_left.density_definition(c["g"], c["f"], o, t1, t2, l0, lv, r0, rv), 1e-11, f"{name} density, {what}")
        assert np.array_equal(d, d.T) and abs(np.trace(d)) < 1e-12
    eng.so_set_lambda(*l)
    ground = eng.so_eom_density(1.0, l, 1.0, None)
    _close(ground, eng.so_density(), 1e-11, f"{name} (1, lambda; 1, 0) against afesp_ccsd_so_density")
    rs = [r, l, np_lambda.antisym_random(rng, o, v)]
    cs = eng.so_eom_ref_coupling(np.stack([x[0] for x in rs]), np.stack([x[1] for x in rs]))
    for k, x in enumerate(rs):
        ref = np_eom_left.ref_coupling(cc, t1, t2, *x)
        print(name, "reference coupling", cs[k], ref)
        assert abs(cs[k] - ref) <= 1e-12 * max(1.0, abs(ref)) and eng.so_eom_ref_coupling(*x) == cs[k]
    a1, a2 = eng.so_amplitudes()
    b1, b2 = eng.so_lambda()
    assert np.array_equal(a1, t1) and np.array_equal(a2, t2) and np.array_equal(b1, l[0]) and np.array_equal(b2, l[1])


def test_two_electron_densities_and_oscillator_strengths_are_fci(eng):
    """CCSD is exact for two electrons: through so_eom_solve, so_eom_left_solve, biorthonormalise, so_eom_properties and
    oscillator_strengths, the singlets' densities and transition-moment products are FCI's and every triplet component is dark"""
    ref = two_electron_case()
    c = _build_case("two_electron", "fock", ref["n"], 1, 1, 21)
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-13, 1e-13)
    assert nit > 0
    density.so_lambda_solve(eng, 300, 1e-12, 1e-12)
    lam = eng.so_lambda()
    nroots = ref["nroots"]
    omega, R, info = eom.so_eom_solve(eng, nroots, tol=1e-10)
    wl, L, _ = eom.so_eom_left_solve(eng, R, tol=1e-10)
    assert np.max(np.abs(wl - omega)) < 1e-9 and 3 in [len(x) for x in eom.clusters(omega)]
    L = eom.biorthonormalise(omega, L, R)
    S = np.array([[eom.dot(l, r) for r in R] for l in L])
    assert np.max(np.abs(S - np.eye(nroots))) < 1e-8
    props = eom.so_eom_properties(eng, omega, L, R, lam)
    check_two_electron_properties(ref, omega, props)
    n = ref["n"]
    orb, spin = density.so_spin_order(n, 1, 1, False)
    rng = np.random.default_rng(41)
    dip = [np_eom_left.so_matrix(m + m.T, m + m.T, orb, spin) for m in rng.uniform(-1.0, 1.0, (3, n, n))]
    f = eom.oscillator_strengths(omega, [p["g0k"] for p in props], [p["gk0"] for p in props], dip)
    exc = ref["fci_w"] - ref["fci_w"][0]
    for k, w in enumerate(omega):
        ck = ref["fci_c"][int(np.argmin(np.abs(exc - w)))]
        ta, tb = np_eom_left.fci_density(ref["fci_c"][0], ck)
        fk = 2.0 / 3.0 * w * sum(float(np.sum(m * np_eom_left.so_matrix(ta, tb, orb, spin))) ** 2 for m in dip)
        print("root", k, "f", f[k], "FCI", fk if np_eom_left.fci_is_singlet(ck) else 0.0)
        assert abs(f[k] - (fk if np_eom_left.fci_is_singlet(ck) else 0.0)) < 1e-9 * max(1.0, w)


def test_statuses_and_release(eng):
    c = _case("rhf_fed")
    o, v = c["o"], c["v"]
    nvec = o * v + o * o * v * v
    rng = np.random.default_rng(3)
    x, y = np_lambda.antisym_random(rng, o, v), np_lambda.antisym_random(rng, o, v)
    _feed(eng, c)
    live_state = eng.arena_stats()["live_gb"]
    for call in (lambda: eng.so_eom_left_init(2, 8), lambda: eng.so_eom_lsigma(*x), lambda: eng.so_eom_ref_coupling(*x),
                 lambda: eng.so_eom_density(1.0, x, 1.0, y)):
        with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
            call()
    eng.so_lambda_init(0)
    for nroots, max_space in ((0, 8), (3, 5), (2, 5000)):
        with pytest.raises(AfespError, match="status 1: afesp_ccsd_so_eom_left_init: (nroots|max_space) must be"):
            eng.so_eom_left_init(nroots, max_space)
    eng.so_eom_init(2, 8)                                                   # a right-hand state is no left one
    eng._eom_nroots = {"left": 2}
    for call in (lambda: eng.so_eom_left_guess(), lambda: eng.so_eom_left_iterate(), lambda: eng.so_eom_left_vector(0),
                 lambda: eng.so_eom_left_set_guess(0, *x)):
        with pytest.raises(AfespError, match="status 21: .*no left EOM state"):
            call()
    n = o + v
    with pytest.raises(AfespError, match=f"status 22: .*holds {n * n - 1} doubles"):
        eng.so_eom_density(1.0, x, 1.0, y, capacity=n * n - 1)
    a, buf = np.zeros(nvec), np.zeros(n * n)
    for ptrs in ((a.ctypes.data, None, None, None), (None, a.ctypes.data, None, None), (None, None, a.ctypes.data, None),
                 (None, None, None, a.ctypes.data)):
        with pytest.raises(AfespError, match="status 1: .*both NULL or both given"):
            eng._chk(eng.L.afesp_ccsd_so_eom_density(eng.h, 1.0, ptrs[0], ptrs[1], 1.0, ptrs[2], ptrs[3], buf, buf.size))
    eng.so_eom_lsigma(*x)                                                   # (the scratch of the left builds is there from now on)
    eng.so_eom_density(1.0, x, 1.0, y)
    live0 = eng.arena_stats()["live_gb"]
    eng.so_eom_left_init(2, 40)
    live1 = eng.arena_stats()["live_gb"]
    assert (live1 - live0) * 1e9 >= 8 * 2 * 40 * nvec
    with pytest.raises(AfespError, match="status 1: afesp_ccsd_so_eom_left_iterate: no guess vectors"):
        eng.so_eom_left_iterate()
    with pytest.raises(AfespError, match="status 1: .*tol must be positive"):
        eng.so_eom_left_iterate(0.0)
    eng.so_eom_left_guess()
    first = eng.so_eom_left_iterate(1e-8)
    with pytest.raises(AfespError, match="status 1: afesp_ccsd_so_eom_left_get_vector: no Ritz vector"):
        eng.so_eom_left_vector(2)
    eng.so_eom_guess()                                                      # the right-hand state serves beside it
    eng.so_eom_iterate(1e-8)
    eng.so_lambda_init(0)                                                   # releases both EOM states with the Lambda state they borrowed from
    assert (live1 - eng.arena_stats()["live_gb"]) * 1e9 >= 0.9 * 8 * 2 * 40 * nvec
    for call in (lambda: eng.so_eom_left_iterate(), lambda: eng.so_eom_left_guess()):
        with pytest.raises(AfespError, match="status 21: .*no left EOM state"):
            call()
    eng.so_eom_left_init(2, 40)                                             # ... and a new one serves again, with the same numbers
    eng.so_eom_left_guess()
    again = eng.so_eom_left_iterate(1e-8)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[3] == again[3]
    t1, t2 = eng.so_amplitudes()
    eng.so_set_amplitudes(t1, t2)                                           # may have changed t: stale, whatever was written
    for call in (lambda: eng.so_eom_left_iterate(), lambda: eng.so_eom_lsigma(*x), lambda: eng.so_eom_left_guess(),
                 lambda: eng.so_eom_left_init(2, 8), lambda: eng.so_eom_density(1.0, x, 1.0, y), lambda: eng.so_eom_ref_coupling(*x)):
        with pytest.raises(AfespError, match="status 21: .*stale"):
            call()
    live_stale = eng.arena_stats()["live_gb"]
    _feed(eng, c)                                                           # a new state: everything of the old one is released (so_free)
    live_new = eng.arena_stats()["live_gb"]
    print("live bytes: state", live_state * 1e9, "with stale Lambda and the left state", live_stale * 1e9, "after the new init", live_new * 1e9)
    assert (live_stale - live_new) * 1e9 >= 0.9 * 8 * 2 * 40 * nvec
    assert (live_new - live_state) * 1e9 < 0.5 * 8 * 2 * 40 * nvec           # (a leaked B or S would stand out over the arena's block slack)
    _feed(eng, c, published=False)
    with pytest.raises(AfespError, match="status 20: .*F_mi"):
        eng.so_lambda_init(0)
    for call in (lambda: eng.so_eom_left_init(2, 8), lambda: eng.so_eom_lsigma(*x), lambda: eng.so_eom_density(1.0, x, 1.0, y)):
        with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
            call()
