"""GPU parity of EOM-EE-CCSD on the spin-orbital state (afesp_ccsd_so_eom_*, afesp_amd.eom): the sigma build against the complex-step
definition of np_eom at the shapes of tests/test_gpu_lambda.py, the adjoint identity against the GPU's own Lambda step, the Davidson
iteration against the eigenvalues of the complex-step Jacobian on four converged models (np_eom.MODELS) and against FCI for two
electrons, that an EOM solve changes nothing else, and the statuses.

Tolerances: 1e-11 x max(1, max |ref|) for sigma at equal amplitudes; 1e-8 for omega at tol = 1e-8 (the reference Davidson
of tests/test_eom_cpu.py stays within 2e-10 there); 10 tol for the residual norm recomputed from the returned vectors.

Not covered here: a recording context (Context::rec) is refused by every EOM entry point as by Lambda's, but no call of the C interface
leaves a context recording, so the refusal cannot be reached from a test."""
import numpy as np
import pytest

import np_eom
import np_lambda
import np_rocc
import np_ucc
from afesp_amd import density, eom
from afesp_amd.capi import AfespError
from test_gpu_lambda import SHAPES, _build_case, _case, _close, _feed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _antisymmetric_to_the_bit(x2):
    return np.array_equal(x2, -x2.transpose(1, 0, 2, 3)) and np.array_equal(x2, -x2.transpose(0, 1, 3, 2))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_sigma_equals_the_complex_step_at_random_amplitudes(eng, name):
    """sigma(r) = Im R(t + i h r) / h at O(0.3) random t and r: a missing or mis-signed term shows at 1e-2 and upward"""
    c = _case(name)
    cc, o, v = c["cc"], c["o"], c["v"]
    rng = np.random.default_rng(17)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    rs = [np_lambda.antisym_random(rng, o, v) for _ in range(3)]
    _feed(eng, c)
    eng.so_set_amplitudes(t1, t2)
    eng.so_lambda_init(0)
    s1, s2 = eng.so_eom_sigma(np.stack([r[0] for r in rs]), np.stack([r[1] for r in rs]))       # nvec = 3 in one call
    for k, (r1, r2) in enumerate(rs):
        d1, d2 = np_eom.sigma_definition(cc, t1, t2, r1, r2)
        _close(s1[k], d1, 1e-11, f"{name} sigma1 of vector {k}")
        _close(s2[k], d2, 1e-11, f"{name} sigma2 of vector {k}")
        assert _antisymmetric_to_the_bit(s2[k])
        a1, a2 = eng.so_eom_sigma(r1, r2)                                   # ... equals three calls bit for bit
        assert np.array_equal(a1, s1[k]) and np.array_equal(a2, s2[k])
    if o == 1:
        assert not np.any(s2)
    a1, a2 = eng.so_amplitudes()
    assert np.array_equal(a1, t1) and np.array_equal(a2, t2)


@pytest.mark.parametrize("name", ["rhf_fed", "uhf_fed", "fock_rotated"])
def test_adjoint_identity_against_the_lambda_step(eng, name):
    """<l, sigma(r)> = <G(l) - G(0), r> with G = (l_new - l) D of afesp_ccsd_so_lambda_iterate: sigma is the transpose of Lambda's matrix"""
    c = _case(name)
    cc, o, v = c["cc"], c["o"], c["v"]
    rng = np.random.default_rng(19)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    l1, l2 = np_lambda.antisym_random(rng, o, v)
    r1, r2 = np_lambda.antisym_random(rng, o, v)
    _feed(eng, c)
    eng.so_set_amplitudes(t1, t2)
    eng.so_lambda_init(0)
    G = []
    for x1, x2 in ((l1, l2), (0.0 * l1, 0.0 * l2)):
        eng.so_set_lambda(x1, x2)
        eng.so_lambda_iterate(1e-11, 1e-11)
        n1, n2 = eng.so_lambda()
        G.append(((n1 - x1) * cc.D1, (n2 - x2) * cc.D2))
    s1, s2 = eng.so_eom_sigma(r1, r2)
    lhs, rhs = np_eom.dot(l1, l2, s1, s2), np_eom.dot(G[0][0] - G[1][0], G[0][1] - G[1][1], r1, r2)
    err, bound = abs(lhs - rhs), 1e-11 * max(1.0, abs(lhs))
    print(name, "adjoint", lhs, rhs, "error", err, "bound", bound)
    assert err < bound


def _feed_model(eng, c):
    """a model of np_eom.MODELS as a Fock-fed state in the model's own orbitals, at the numpy side's converged amplitudes"""
    n, blk = c["n"], c["blocks"]
    eng.do_mp2_spatial(n, 1, np.eye(n), np.arange(n, dtype=np.float64), np_ucc.pack8(blk["chem"]), want_eri_mo=False)
    eng.mo_rotate_uhf(n, np.eye(n), np.eye(n))
    eng.uso_init_fock(n, c["na"], c["nb"], blk["fa"], blk["fb"], 8)
    eng.so_set_amplitudes(c["t1"], c["t2"])
    eng.so_lambda_init(0)


def _residual_norms(eng, omega, vectors):
    out = []
    for w, (x1, x2) in zip(omega, vectors):
        s1, s2 = eng.so_eom_sigma(x1, x2)
        out.append(np.sqrt(np_eom.dot(s1 - w * x1, s2 - w * x2, s1 - w * x1, s2 - w * x2)))
    return np.array(out)


@pytest.mark.parametrize("name", sorted(np_eom.MODELS))
@pytest.mark.parametrize("nroots", [4, 6])
def test_davidson_finds_the_lowest_roots_of_the_jacobian(eng, name, nroots):
    c = np_eom.converged_model(name)
    ref = c["w"][:nroots].real
    _feed_model(eng, c)
    tol = 1e-8
    runs = []
    for max_space in (4 * nroots, 4 * nroots, None):                         # twice with a space so small that the collapse runs
        omega, vectors, info = eom.so_eom_solve(eng, nroots, tol=tol, max_space=max_space, maxiter=300)
        print(name, nroots, "max_space", info["max_space"], info["iterations"], "steps", info["nsigma"], "sigma builds, omega error",
              np.max(np.abs(omega - ref)))
        assert np.max(np.abs(omega - ref)) < 1e-8
        assert not info["complex"] and np.all(info["flags"] & eom.FLAG_CONVERGED)
        res = _residual_norms(eng, omega, vectors)
        print(name, nroots, "recomputed residual norms", res)
        assert np.all(res < 10.0 * tol)
        for x1, x2 in vectors:
            assert abs(np_eom.dot(x1, x2, x1, x2) - 1.0) < 1e-12 and _antisymmetric_to_the_bit(x2)
        runs.append((omega, vectors, info))
    assert runs[0][2]["nsigma"] > 4 * nroots                                # more sigma builds than basis vectors fit: it collapsed
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][2]["nsigma"] == runs[1][2]["nsigma"]
    for (a1, a2), (b1, b2) in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2)            # a second run: identical bits


def test_two_electron_roots_are_fci_excitation_energies(eng):
    """CCSD is exact for two electrons: every eigenvalue of A is an FCI excitation energy (the Ms = +-1 components of a triplet at the
    energy of its Ms = 0 component), and the lowest FCI excitations are all found"""
    c = _build_case("two_electron", "fock", 4, 1, 1, 21)
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-13, 1e-13)
    assert nit > 0
    eng.so_lambda_init(0)
    nroots = 6
    omega, vectors, info = eom.so_eom_solve(eng, nroots, tol=1e-10)
    fci = np_eom.fci_two_electron_spectrum(c["h"], c["chem"])
    exc = fci[1:] - fci[0]
    print("omega", omega, "FCI", exc[:nroots], "degeneracy", info["degeneracy"])
    for w in omega:
        assert np.min(np.abs(exc - w)) < 1e-9
    for x in exc[exc < omega[-1] - 1e-6]:
        assert np.min(np.abs(omega - x)) < 1e-9
    assert 3 in info["degeneracy"]                                          # a triplet appears threefold
    labels = [eom.label_root(x1, x2, c["n"], 1, 1, False) for x1, x2 in vectors]
    print([(l["kind"], l["occ"], l["virt"], l["delta_ms"]) for l in labels])
    assert all(l["delta_ms"] in (-1.0, 0.0, 1.0) for l in labels)          # (degenerate components may mix: no more is fixed)


def test_an_eom_solve_changes_nothing_else(eng):
    c = _case("uhf_fed")
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    e_t = eng.do_ccsd_t_spinorb()
    density.so_lambda_solve(eng, 300, 1e-11, 1e-11)
    before = (*eng.so_amplitudes(), *eng.so_lambda(), eng.so_density())
    omega, _, info = eom.so_eom_solve(eng, 3)
    assert np.all(omega > 0.0) and info["nsigma"] >= 3
    after = (*eng.so_amplitudes(), *eng.so_lambda(), eng.so_density())
    for a, b in zip(before, after):
        assert np.array_equal(a, b)                                         # t1, t2, l1, l2, the density: bit for bit
    assert eng.do_ccsd_t_spinorb() == e_t
    eng.so_lambda_iterate(1e-11, 1e-11)                                     # ... and the Lambda state is still live


def test_the_callers_guesses_replace_the_unit_guesses(eng):
    """sigma builds of the first step count the vectors that entered the basis"""
    c = _case("rhf_fed")
    o, v = c["o"], c["v"]
    rng = np.random.default_rng(23)
    (p1, p2), (q1, q2) = np_lambda.antisym_random(rng, o, v), np_lambda.antisym_random(rng, o, v)
    _feed(eng, c)
    eng.so_lambda_init(0)
    eng.so_eom_init(2, 8)
    eng.so_eom_guess()
    eng.so_eom_set_guess(1, p1, p2)                                         # starts over: the unit guesses are gone, column 0 is zero and dropped
    assert eng.so_eom_iterate(1e-8)[3] == 1
    eng.so_eom_set_guess(0, q1, q2)                                         # after a step: starts over again ...
    eng.so_eom_set_guess(1, p1, p2)                                         # ... and the second one joins the first
    omega, _, _, nsigma, _ = eng.so_eom_iterate(1e-8)
    assert nsigma == 2
    x1, x2 = eng.so_eom_vector(0)
    span = np.array([np.concatenate([a.ravel(), 0.5 * b.ravel()]) for a, b in ((q1, q2), (p1, p2))]).T      # (weights 1, 1/4 as a plain dot)
    y = np.concatenate([x1.ravel(), 0.5 * x2.ravel()])
    assert np.linalg.norm(y - span @ np.linalg.lstsq(span, y, rcond=None)[0]) < 1e-12                     # the Ritz vector lies in their span
    eng.so_eom_guess()                                                      # the unit guesses again: two vectors
    assert eng.so_eom_iterate(1e-8)[3] == 2


def test_statuses_and_release(eng):
    c = _case("rhf_fed")
    o, v = c["o"], c["v"]
    nvec, nunique = o * v + o * o * v * v, o * v + (o * (o - 1) // 2) * (v * (v - 1) // 2)
    r1, r2 = np_lambda.antisym_random(np.random.default_rng(3), o, v)
    _feed(eng, c)
    live_state = eng.arena_stats()["live_gb"]                              # the state alone: no Lambda state, no EOM state, no scratch
    for call in (lambda: eng.so_eom_init(2, 8), lambda: eng.so_eom_sigma(r1, r2)):
        with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
            call()
    eng.so_lambda_init(0)
    for nroots, max_space in ((0, 8), (-1, 8), (nunique + 1, 4 * nunique), (3, 5), (2, 5000)):
        with pytest.raises(AfespError, match="status 1: .*(nroots|max_space) must be"):
            eng.so_eom_init(nroots, max_space)
    eng._eom_nroots = {"ee": 2}
    for call in (lambda: eng.so_eom_guess(), lambda: eng.so_eom_iterate(), lambda: eng.so_eom_vector(0)):
        with pytest.raises(AfespError, match="status 21: .*no EOM state"):
            call()
    eng.so_eom_sigma(r1, r2)                                                # (its scratch is there from now on)
    live0 = eng.arena_stats()["live_gb"]
    eng.so_eom_init(2, 40)
    live1 = eng.arena_stats()["live_gb"]
    assert (live1 - live0) * 1e9 >= 8 * 2 * 40 * nvec
    with pytest.raises(AfespError, match="status 1: .*no guess vectors"):
        eng.so_eom_iterate()
    with pytest.raises(AfespError, match="status 1: .*tol must be positive"):
        eng.so_eom_iterate(0.0)
    eng.so_eom_guess()
    first = eng.so_eom_iterate(1e-8)
    with pytest.raises(AfespError, match="status 1: .*no Ritz vector"):
        eng.so_eom_vector(2)
    eng.so_lambda_init(0)                                                   # releases the EOM state with the Lambda state it borrowed from
    # (the new Lambda state may be handed blocks up to a quarter larger than it asks for: nine tenths of B and S are certainly back)
    assert (live1 - eng.arena_stats()["live_gb"]) * 1e9 >= 0.9 * 8 * 2 * 40 * nvec
    with pytest.raises(AfespError, match="status 21: .*no EOM state"):
        eng.so_eom_iterate()
    eng.so_eom_init(2, 40)                                                  # ... and a new one serves again, with the same numbers
    eng.so_eom_guess()
    again = eng.so_eom_iterate(1e-8)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[3] == again[3]
    t1, t2 = eng.so_amplitudes()
    eng.so_set_amplitudes(t1, t2)                                           # may have changed t: stale, whatever was written
    for call in (lambda: eng.so_eom_iterate(), lambda: eng.so_eom_sigma(r1, r2), lambda: eng.so_eom_guess(), lambda: eng.so_eom_init(2, 8)):
        with pytest.raises(AfespError, match="status 21: .*stale"):
            call()
    live_stale = eng.arena_stats()["live_gb"]                              # the state, its stale Lambda state and the EOM state of 2 x 40 columns
    _feed(eng, c)                                                           # a new state: everything of the old one is released (so_free)
    live_new = eng.arena_stats()["live_gb"]
    print("live bytes: state", live_state * 1e9, "with stale Lambda and EOM", live_stale * 1e9, "after the new init", live_new * 1e9,
          "B and S", 8 * 2 * 40 * nvec)
    assert (live_stale - live_new) * 1e9 >= 0.9 * 8 * 2 * 40 * nvec
    assert (live_new - live_state) * 1e9 < 0.5 * 8 * 2 * 40 * nvec           # (a leaked B or S would stand out over the arena's block slack)
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
        eng.so_eom_guess()
    _feed(eng, c, published=False)
    with pytest.raises(AfespError, match="status 20: .*F_mi"):
        eng.so_lambda_init(0)
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
        eng.so_eom_init(2, 8)
