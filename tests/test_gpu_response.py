"""GPU parity of EOM-CCSD linear response on the spin-orbital state (afesp_ccsd_so_response_*, afesp_amd.response) against np_response:
the operator vectors xi at handed-in random amplitudes, the perturbed amplitudes and the response function against dense numpy solves
at converged amplitudes, FCI for two electrons through the library, the statuses, and that a whole solve writes nothing else.

Tolerances: 1e-12 x max(1, |xi|) for xi at equal amplitudes; 10 tol |R| for R against the dense solve (the residual bound) and 1e-7
relative for the response function at tol = 1e-8, 1e-9 at tol = 1e-11; 1e-8 against FCI."""
import numpy as np
import pytest

import np_eom
import np_lambda
import np_response
import np_rocc
import np_ucc
from afesp_amd import density, eom, response
from afesp_amd.capi import AfespError
from test_eom_left_cpu import two_electron_case
from test_gpu_eom import _feed_model
from test_gpu_lambda import _build_case, _case, _feed
from test_response_cpu import random_symmetric, two_electron_operators

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _model_case(n, na, nb, seed):
    """an np_lambda.model as a Fock-fed state in its own orbitals (test_gpu_eom._feed_model takes it)"""
    g, f, o, blk = np_lambda.model(n, na, nb, seed)
    return dict(n=n, na=na, nb=nb, o=o, v=2 * n - o, blocks=blk, g=g, f=f)


def _feed_plain(eng, c):
    n, blk = c["n"], c["blocks"]
    eng.do_mp2_spatial(n, 1, np.eye(n), np.arange(n, dtype=np.float64), np_ucc.pack8(blk["chem"]), want_eri_mo=False)
    eng.mo_rotate_uhf(n, np.eye(n), np.eye(n))
    eng.uso_init_fock(n, c["na"], c["nb"], blk["fa"], blk["fb"], 8)


def check_xi(eng, o, v, tag, seed=11):
    """xi of three random symmetric operators at handed-in random O(0.3) t: against numpy, antisymmetric to the bit, batched = single
    calls bit for bit, two runs bit for bit.  (test_gpu_response_mid.py runs this too)"""
    rng = np.random.default_rng(seed)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    ops = np.stack([random_symmetric(rng, o + v) for _ in range(3)])
    eng.so_set_amplitudes(t1, t2)
    x1, x2 = eng.so_response_xi(ops)                                         # nop = 3 in one launch
    y1, y2 = eng.so_response_xi(ops)
    assert np.array_equal(x1, y1) and np.array_equal(x2, y2)
    for k in range(3):
        r1, r2 = np_response.xi_explicit(t1, t2, ops[k])
        bound = 1e-12 * max(1.0, float(np.max(np.abs(r1))), float(np.max(np.abs(r2))) if r2.size else 0.0)
        err = max(float(np.max(np.abs(x1[k] - r1))), float(np.max(np.abs(x2[k] - r2))) if r2.size else 0.0)
        print(tag, (o, v), "operator", k, "xi error", err, "bound", bound)
        assert err < bound
        assert np.array_equal(x2[k], -x2[k].transpose(1, 0, 2, 3)) and np.array_equal(x2[k], -x2[k].transpose(0, 1, 3, 2))
        a1, a2 = eng.so_response_xi(ops[k])
        assert np.array_equal(a1, x1[k]) and np.array_equal(a2, x2[k])
    a1, a2 = eng.so_amplitudes()
    assert np.array_equal(a1, t1) and np.array_equal(a2, t2)


@pytest.mark.parametrize("n,na,nb,seed", [(5, 2, 1, 62), (6, 3, 2, 64)])
def test_xi_on_the_models(eng, n, na, nb, seed):
    c = _model_case(n, na, nb, seed)
    _feed_plain(eng, c)
    check_xi(eng, c["o"], c["v"], "model")


@pytest.mark.parametrize("name", ["rhf_fed", "uhf_fed", "fock_rotated"])
def test_xi_on_every_kind_of_state(eng, name):
    c = _case(name)
    _feed(eng, c)
    check_xi(eng, c["o"], c["v"], name)


_CONV = {}


def _converged(n, na, nb, seed):
    """a model at its converged amplitudes with the dense Jacobian, made once and left unchanged"""
    key = (n, na, nb, seed)
    if key not in _CONV:
        c = _model_case(n, na, nb, seed)
        cc = np_rocc.ROCC(c["g"], c["f"], c["o"])
        cc.solve(300, 1e-13, 1e-13)
        c.update(cc=cc, t1=cc.t1.copy(), t2=cc.t2.copy())
        c["A"] = np_lambda.jacobian(cc, c["t1"], c["t2"])[1]
        c["w1"] = float(np.min(np.linalg.eigvals(c["A"]).real))
        _CONV[key] = c
    return _CONV[key]


def _norm(x):
    return np.sqrt(np_eom.dot(*x, *x))


@pytest.mark.parametrize("n,na,nb,seed", [(5, 2, 2, 72), (6, 3, 2, 74)])
def test_solve_against_the_dense_numpy_solve(eng, n, na, nb, seed):
    c = _converged(n, na, nb, seed)
    cc, t1, t2, A, o, v = c["cc"], c["t1"], c["t2"], c["A"], c["o"], c["v"]
    _feed_model(eng, c)
    density.so_lambda_solve(eng, 300, 1e-12, 1e-12)
    lam = eng.so_lambda()
    rng = np.random.default_rng(seed)
    ops = [random_symmetric(rng, o + v) for _ in range(3)]
    omegas = [0.0, 0.5 * c["w1"]]
    xis = [np_response.xi_explicit(t1, t2, X) for X in ops]
    for tol, rbound, fbound in ((1e-8, 1e-7, 1e-7), (1e-11, 1e-9, 1e-9)):
        rf, info = response.so_response_solve(eng, ops, omegas, tol=tol)
        print((o, v), "tol", tol, info["iterations"], "steps", info["nsigma"], "sigma builds, residuals", info["resnorm"].ravel())
        assert np.all(info["resnorm"] < tol)
        signed = list(info["omega_signed"])
        assert signed == [0.0, omegas[1], -omegas[1]]
        if (o, v) == (4, 6) and tol == 1e-8:
            # the device follows np_response.linear_davidson rule by rule: the same steps, sigma builds and collapses -- and residuals that
            # agree as far as two summation orders let an iterate of size 1e-9 agree (1e-3 relative; 1e-7 was seen)
            I = np_lambda.hbar(cc, t1, t2)
            _, ninfo = np_response.linear_davidson(lambda a, b: np_eom.sigma_explicit(cc, t1, t2, a, b, I), cc.D1, cc.D2, xis * 3,
                                                   [w for w in signed for _ in range(3)], tol=tol, max_space=info["max_space"])
            print("numpy restatement:", ninfo)
            assert (ninfo["iterations"], ninfo["nsigma"]) == (info["iterations"], info["nsigma"])
            assert np.max(np.abs(ninfo["resnorm"] / info["resnorm"].ravel() - 1.0)) < 1e-3
        vec = {}
        for g, w in enumerate(signed):
            for a in range(3):
                R = eng.so_response_vector(a, g)
                ref = np_response.solve_dense(A, o, v, xis[a], w)
                err, bound = _norm((R[0] - ref[0], R[1] - ref[1])), rbound * _norm(ref)
                print((o, v), "tol", tol, "omega", w, "operator", a, "R error", err, "bound", bound)
                assert err < bound
                assert np.array_equal(R[1], -R[1].transpose(1, 0, 2, 3)) and np.array_equal(R[1], -R[1].transpose(0, 1, 3, 2))
                vec[a, w] = R
        for f, w in enumerate(omegas):
            ref = np_response.response_dense(cc, t1, t2, lam, A, ops, w)
            err, bound = float(np.max(np.abs(rf[f] - ref))), fbound * float(np.max(np.abs(ref)))
            print((o, v), "tol", tol, "omega", w, "response function error", err, "bound", bound)
            assert err < bound
            own = np_response.response_from_vectors(cc, t1, t2, lam, ops, [vec[a, w] for a in range(3)], [vec[a, -w] for a in range(3)])
            # Phi of the device's own vectors: the density call is held to 1e-11 per element (test_gpu_eom_left), its trace with an
            # operator of (o+v)^2 elements up to 2 in size to (o+v)^2 x 2 x that
            assert np.max(np.abs(rf[f] - own)) < 2.0 * (o + v) ** 2 * 1e-11 * max(1.0, float(np.max(np.abs(ref))))
    again, info2 = response.so_response_solve(eng, ops, omegas, tol=1e-11)
    assert np.array_equal(again, rf) and info2["nsigma"] == info["nsigma"]    # a second run: identical bits


def test_sigma_builds_of_the_shared_basis_and_of_six_separate_solves(eng):
    """3 operators x (+omega, -omega) at one nonzero frequency on (6,3,2): the counts DESIGN.md 4.19 quotes"""
    c = _converged(6, 3, 2, 74)
    o, v = c["o"], c["v"]
    _feed_model(eng, c)
    rng = np.random.default_rng(74)
    ops = [random_symmetric(rng, o + v) for _ in range(3)]
    w = 0.5 * c["w1"]
    eng.so_response_init(np.stack(ops), [w, -w], 48)
    for it in range(100):
        res, shared, conv = eng.so_response_iterate(1e-8)
        if conv:
            break
    assert conv
    Rs = {(a, g): eng.so_response_vector(a, g) for a in range(3) for g in range(2)}
    separate = []
    for g, s in enumerate((w, -w)):
        for a in range(3):
            eng.so_response_init(ops[a], [s], 8)
            for it in range(100):
                res, ns, conv = eng.so_response_iterate(1e-8)
                if conv:
                    break
            assert conv
            separate.append(ns)
            R = eng.so_response_vector(0, 0)
            d = (R[0] - Rs[a, g][0], R[1] - Rs[a, g][1])
            assert _norm(d) < 1e-6 * _norm(R)                               # the same solution either way
    print("sigma builds: shared basis", shared, "six separate solves", separate, "sum", sum(separate))
    assert shared > 0 and len(separate) == 6


def test_two_electron_response_is_fci_through_the_library(eng):
    ref = two_electron_case()
    c = _build_case("two_electron", "fock", ref["n"], 1, 1, 21)
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-13, 1e-13)
    assert nit > 0
    density.so_lambda_solve(eng, 300, 1e-12, 1e-12)
    ms, ops = two_electron_operators(ref)
    w1 = float(np.min(np.linalg.eigvals(ref["A"]).real))
    omegas = [0.0, 0.5 * w1]
    rf, info = response.so_response_solve(eng, ops, omegas, tol=1e-10)
    for f, w in enumerate(omegas):
        fci = np.array([[np_response.fci_response(ref["fci_w"], ref["fci_c"], x, y, w) for y in ms] for x in ms])
        print("omega", w, "alpha", -rf[f], "FCI", -fci)
        assert np.max(np.abs(rf[f] - fci)) < 1e-8
        assert abs(rf[f][0, 1] - rf[f][1, 0]) < 1e-8                        # exact here, and only here, off omega = 0
    dip = [ops[0], ops[1], 0.0 * ops[0]]
    alpha, iso, aniso, _ = response.polarizability(eng, dip, omegas, tol=1e-10)
    assert np.max(np.abs(alpha[:, :2, :2] + rf)) < 1e-9 and not np.any(alpha[:, 2, :]) and not np.any(alpha[:, :, 2])
    assert abs(iso[0] - np.trace(alpha[0]) / 3.0) < 1e-14 and aniso[0] > 0.0


def test_statuses(eng):
    c = np_eom.converged_model("o4v6")
    o, v = c["o"], c["v"]
    n = o + v
    rng = np.random.default_rng(3)
    X = random_symmetric(rng, n)
    _feed_model(eng, c)                                                      # (ends with so_lambda_init)
    bad = X.copy()
    bad[0, n - 1] += 1e-6
    for call in (lambda: eng.so_response_xi(bad), lambda: eng.so_response_init(bad[None], [0.0], 8)):
        with pytest.raises(AfespError, match="status 1: .*not symmetric"):
            call()
    for call in (lambda: eng.so_response_xi(np.zeros((0, n, n))), lambda: eng.so_response_init(np.zeros((0, n, n)), [0.0], 8)):
        with pytest.raises(AfespError, match="status 1: .*nop must be"):
            call()
    with pytest.raises(AfespError, match="status 1: .*max_space must be"):
        eng.so_response_init(X[None], [0.1, -0.1], 3)
    for call in (lambda: eng.so_response_iterate(), lambda: eng.so_response_function([0.0])):
        with pytest.raises(AfespError, match="status 21: .*no response state"):
            call()
    eng.so_response_init(X[None], [0.0, 0.1], 16)
    with pytest.raises(AfespError, match="status 27: .*not converged"):
        eng.so_response_function([0.0])                                     # no step yet
    with pytest.raises(AfespError, match="status 1: .*no solution"):
        eng.so_response_vector(0, 0)
    with pytest.raises(AfespError, match="status 1: .*tol must be positive"):
        eng.so_response_iterate(0.0)
    for it in range(100):
        _, _, conv = eng.so_response_iterate(1e-8)
        if conv:
            break
    assert conv
    assert eng.so_response_function([0.0]).shape == (1, 1, 1)
    for w in (0.1, 0.2):                                                     # +0.1 was solved, -0.1 was not; 0.2 not at all
        with pytest.raises(AfespError, match="status 1: .*was not solved at both signs"):
            eng.so_response_function([w])
    with pytest.raises(AfespError, match="status 1: .*no solution"):
        eng.so_response_vector(1, 0)
    with pytest.raises(AfespError, match="status 27: .*not converged"):      # maxiter = 1 at a tight tol
        response.so_response_solve(eng, [X], [0.1], tol=1e-13, maxiter=1)
    # ---- stale after anything that may have written t or lambda
    eng.so_response_init(X[None], [0.0], 8)
    eng.so_set_lambda(*eng.so_lambda())
    for call in (lambda: eng.so_response_iterate(), lambda: eng.so_response_function([0.0]), lambda: eng.so_response_vector(0, 0)):
        with pytest.raises(AfespError, match="status 21: .*stale"):
            call()
    eng.so_response_init(X[None], [0.0], 8)
    eng.so_response_iterate()
    eng.so_set_amplitudes(*eng.so_amplitudes())
    for call in (lambda: eng.so_response_iterate(), lambda: eng.so_response_function([0.0]), lambda: eng.so_response_init(X[None], [0.0], 8)):
        with pytest.raises(AfespError, match="status 21: .*stale"):
            call()
    eng.so_response_xi(X)                                                    # xi needs the amplitudes alone


def test_a_frequency_at_a_converged_eom_root_is_a_pole(eng):
    c = np_eom.converged_model("o4v6")
    o, v = c["o"], c["v"]
    _feed_model(eng, c)
    omega, R, info = eom.so_eom_solve(eng, 4, tol=1e-9, maxiter=300)
    k = int(np.argmax(info["r1_norm2"]))
    print("root", k, "omega", omega[k], "distance to the nearest eigenvalue of the dense Jacobian", np.min(np.abs(c["w"] - omega[k])))
    X = np.zeros((o + v, o + v))
    X[:o, o:] = np.abs(R[k][0])                                              # an operator whose xi overlaps root k
    X = X + X.T
    with pytest.raises(AfespError, match="status 26: .*frequency at a pole"):
        response.so_response_solve(eng, [X], [omega[k]], tol=1e-8)
    rf, _ = response.so_response_solve(eng, [X], [0.5 * omega[k]], tol=1e-8)  # ... and off the root the same state type serves
    assert np.isfinite(rf).all()
    again = eng.so_eom_iterate(1e-9)                                         # the EE state is live and as it was
    assert np.array_equal(again[0], omega) and again[3] == info["nsigma"] and again[4]


def test_a_response_solve_changes_nothing_else(eng):
    c = _case("uhf_fed")
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    e_t = eng.do_ccsd_t_spinorb()
    density.so_lambda_solve(eng, 300, 1e-11, 1e-11)
    omega, R, info = eom.so_eom_solve(eng, 3)
    wl, L, linfo = eom.so_eom_left_solve(eng, R)
    snapshot = lambda: (*eng.so_amplitudes(), *eng.so_lambda(), *[x for k in range(3) for x in eng.so_eom_vector(k)],
                        *[x for k in range(3) for x in eng.so_eom_left_vector(k)])
    before = snapshot()
    rng = np.random.default_rng(9)
    ops = [random_symmetric(rng, c["o"] + c["v"]) for _ in range(3)]
    live0 = eng.arena_stats()["live_gb"]
    rf, rinfo = response.so_response_solve(eng, ops, [0.0, 0.05])
    assert rinfo["nsigma"] >= 9 and np.isfinite(rf).all()
    nvec = c["o"] * c["v"] + (c["o"] * c["v"]) ** 2
    assert (eng.arena_stats()["live_gb"] - live0) * 1e9 >= 8 * 2 * rinfo["max_space"] * nvec    # a basis of its own
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)                                         # t1, t2, l1, l2, the right and left EE vectors: bit for bit
    again = eng.so_eom_iterate(1e-8)
    assert np.array_equal(again[0], omega) and again[3] == info["nsigma"] and again[4]
    left = eng.so_eom_left_iterate(1e-8)
    assert np.array_equal(left[0], wl) and left[3] == linfo["nsigma"] and left[4]
    assert eng.do_ccsd_t_spinorb() == e_t
    eng.so_lambda_init(0)                                                    # releases the response state with the others
    with pytest.raises(AfespError, match="status 21: .*no response state"):
        eng.so_response_iterate()
