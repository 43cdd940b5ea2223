"""GPU parity of EOM-CCSD linear response at complex frequencies (afesp_ccsd_so_response_*_complex, afesp_amd.response) against
np_response_complex: the perturbed amplitudes R(z) = P + i Q and the response function against dense complex numpy solves at converged
amplitudes, complex FCI and the closed-form C6 for two electrons through the library, the real path at gamma = 0, the statuses, and that
a whole complex solve writes nothing else.

Tolerances (those of test_gpu_response.py): 10 tol |R| for R against the dense solve; 1e-7 relative for the response function at
tol = 1e-8, 1e-9 at tol = 1e-11; 1e-8 against FCI; 1e-6 relative for C6 (the quadrature's own 2.1e-7 is most of it); 10 tol between
the complex entry points at gamma = 0 and the real ones."""
import numpy as np
import pytest

import np_eom
import np_lambda
import np_response
import np_response_complex as npc
from afesp_amd import density, eom, response
from afesp_amd.capi import AfespError
from test_eom_left_cpu import two_electron_case
from test_gpu_eom import _feed_model
from test_gpu_lambda import _build_case, _case, _feed
from test_gpu_response import _converged
from test_response_cpu import random_symmetric, two_electron_operators

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _cnorm(x):
    return np.sqrt(np_eom.dot(x[0].real, x[1].real, x[0].real, x[1].real) + np_eom.dot(x[0].imag, x[1].imag, x[0].imag, x[1].imag))


@pytest.mark.parametrize("n,na,nb,seed", [(5, 2, 2, 72), (6, 3, 2, 74)])
def test_solve_against_the_dense_complex_solve(eng, n, na, nb, seed):
    c = _converged(n, na, nb, seed)
    cc, t1, t2, A, o, v = c["cc"], c["t1"], c["t2"], c["A"], c["o"], c["v"]
    _feed_model(eng, c)
    density.so_lambda_solve(eng, 300, 1e-12, 1e-12)
    lam = eng.so_lambda()
    rng = np.random.default_rng(seed)
    ops = [random_symmetric(rng, o + v) for _ in range(3)]
    zs = [0.3j, 0.5 * c["w1"] + 0.02j, c["w1"] + 0.05j]
    xis = [np_response.xi_explicit(t1, t2, X) for X in ops]
    for tol, rbound, fbound in ((1e-8, 1e-7, 1e-7), (1e-11, 1e-9, 1e-9)):
        rf, info = response.so_response_solve_complex(eng, ops, zs, tol=tol)
        print((o, v), "tol", tol, info["iterations"], "steps", info["nsigma"], "sigma builds, residuals", info["resnorm"].ravel())
        assert np.all(info["resnorm"] < tol)
        signed = list(info["z_signed"])
        assert signed == [zs[0], zs[1], -zs[1], zs[2], -zs[2]]
        if tol == 1e-8:
            # the device follows np_response_complex.ComplexLinear rule by rule: the same steps and sigma builds.  (Fifteen systems of two
            # vectors each fill the 114 / 280 unique amplitudes of these models in the last step, so the final residuals are rounding, 1e-15,
            # on both sides and their ratio says nothing; test_gpu_davidson_complex.py compares residuals step by step)
            I = np_lambda.hbar(cc, t1, t2)
            _, ninfo = npc.linear_davidson_complex(lambda a, b: np_eom.sigma_explicit(cc, t1, t2, a, b, I), cc.D1, cc.D2, xis * 5,
                                                   [z for z in signed for _ in range(3)], tol=tol, max_space=info["max_space"])
            print("numpy restatement:", {k: ninfo[k] for k in ("iterations", "nsigma", "collapses", "dropped")})
            assert (ninfo["iterations"], ninfo["nsigma"]) == (info["iterations"], info["nsigma"])
        vec = {}
        for g, z in enumerate(signed):
            for a in range(3):
                R = eng.so_response_vector_complex(a, g)
                ref = npc.solve_dense(A, o, v, xis[a], z)
                err, bound = _cnorm((R[0] - ref[0], R[1] - ref[1])), rbound * _cnorm(ref)
                print((o, v), "tol", tol, "z", z, "operator", a, "R error", err, "bound", bound)
                assert err < bound
                assert np.array_equal(R[1], -R[1].transpose(1, 0, 2, 3)) and np.array_equal(R[1], -R[1].transpose(0, 1, 3, 2))
                vec[a, z] = R
        for f, z in enumerate(zs):
            ref = npc.response_dense(cc, t1, t2, lam, A, ops, z)
            err, bound = float(np.max(np.abs(rf[f] - ref))), fbound * float(np.max(np.abs(ref)))
            print((o, v), "tol", tol, "z", z, "response function error", err, "bound", bound)
            assert err < bound
            # Phi of the device's own vectors; for the imaginary z the partner is the conjugate of the one solve
            Rm = [vec[a, -z] if z.real != 0.0 else (vec[a, z][0].conj(), vec[a, z][1].conj()) for a in range(3)]
            own = npc.response_from_vectors(cc, t1, t2, lam, ops, [vec[a, z] for a in range(3)], Rm)
            assert np.max(np.abs(rf[f] - own)) < 2.0 * (o + v) ** 2 * 1e-11 * max(1.0, float(np.max(np.abs(ref))))
        assert not np.any(np.diagonal(rf[0]).imag)                          # alpha_XX(i gamma) is real, exactly
    again, info2 = response.so_response_solve_complex(eng, ops, zs, tol=1e-11)
    assert np.array_equal(again, rf) and info2["nsigma"] == info["nsigma"]    # a second run: identical bits


def test_two_electron_complex_response_and_c6_through_the_library(eng):
    ref = two_electron_case()
    c = _build_case("two_electron", "fock", ref["n"], 1, 1, 21)
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-13, 1e-13)
    assert nit > 0
    density.so_lambda_solve(eng, 300, 1e-12, 1e-12)
    ms, ops = two_electron_operators(ref, nops=3)
    w1 = float(np.min(np.linalg.eigvals(ref["A"]).real))
    zs = [0.3j, w1 + 0.05j, 0.5 * w1 + 0.01j]
    rf, info = response.so_response_solve_complex(eng, ops, zs, tol=1e-10)
    for f, z in enumerate(zs):
        fci = np.array([[npc.fci_response(ref["fci_w"], ref["fci_c"], x, y, z) for y in ms] for x in ms])
        print("z", z, "alpha", -rf[f], "FCI", -fci, "error", np.max(np.abs(rf[f] - fci)))
        assert np.max(np.abs(rf[f] - fci)) < 1e-8
    # C6 of the homo-dimer of the model: alpha-bar(iu) on the default grid, one response state of 3 x 19 systems
    u, wts = response.casimir_polder_grid()
    alpha, iso, cinfo = response.polarizability_complex(eng, ops, 1j * u, tol=1e-10)
    assert len(cinfo["z_signed"]) == len(u) and not np.any(iso.imag)
    c6 = response.c6_coefficient(iso, iso, wts)
    exact = npc.c6_closed_form(*npc.fci_strengths(ref["fci_w"], ref["fci_c"], ms))
    print("C6", c6, "closed form", exact, "relative error", abs(c6 / exact - 1.0), "sigma builds", cinfo["nsigma"])
    assert abs(c6 / exact - 1.0) < 1e-6
    sig = response.absorption_cross_section([w1], 0.05, -rf[1:2])
    assert sig[0] > 0.0


def test_gamma_zero_through_the_complex_entry_points_is_the_real_path(eng):
    c = _converged(5, 2, 2, 72)
    o, v = c["o"], c["v"]
    _feed_model(eng, c)
    density.so_lambda_solve(eng, 300, 1e-12, 1e-12)
    rng = np.random.default_rng(72)
    ops = [random_symmetric(rng, o + v) for _ in range(3)]
    omegas, tol = [0.0, 0.5 * c["w1"]], 1e-8
    rr, rinfo = response.so_response_solve(eng, ops, omegas, tol=tol)
    Rr = {(a, g): eng.so_response_vector(a, g) for a in range(3) for g in range(3)}
    rc, cinfo = response.so_response_solve_complex(eng, ops, omegas, tol=tol)
    assert [z.real for z in cinfo["z_signed"]] == list(rinfo["omega_signed"]) and not np.any(cinfo["z_signed"].imag)
    print("sigma builds: real", rinfo["nsigma"], "complex", cinfo["nsigma"], "function difference", np.max(np.abs(rc - rr)))
    assert not np.any(rc.imag) and np.max(np.abs(rc.real - rr)) < 10.0 * tol * max(1.0, float(np.max(np.abs(rr))))
    for (a, g), R in Rr.items():
        Rc = eng.so_response_vector_complex(a, g)
        assert not np.any(Rc[0].imag) and not np.any(Rc[1].imag)
        assert _cnorm((Rc[0] - R[0], Rc[1] - R[1])) < 10.0 * tol


def test_statuses(eng):
    c = np_eom.converged_model("o4v6")
    o, v = c["o"], c["v"]
    n = o + v
    rng = np.random.default_rng(3)
    X = random_symmetric(rng, n)
    _feed_model(eng, c)                                                      # (ends with so_lambda_init)
    with pytest.raises(AfespError, match="status 1: .*max_space must be in 4"):
        eng.so_response_init_complex(X[None], [0.1 + 0.1j, -0.1 - 0.1j], 7)
    with pytest.raises(AfespError, match="status 21: .*no response state"):
        eng.so_response_function_complex([0.1j])
    eng.so_response_init_complex(X[None], [0.2j, 0.1 + 0.05j], 16)
    with pytest.raises(AfespError, match="status 27: .*not converged"):
        eng.so_response_function_complex([0.2j])                             # no step yet
    with pytest.raises(AfespError, match="status 1: .*no solution"):
        eng.so_response_vector_complex(0, 0)
    # a real entry point on a complex state: no silent reinterpretation
    for call in (lambda: eng.so_response_function([0.0]), lambda: eng.so_response_vector(0, 0)):
        with pytest.raises(AfespError, match="status 1: .*made for complex frequencies"):
            call()
    for it in range(100):
        _, _, conv = eng.so_response_iterate(1e-8)
        if conv:
            break
    assert conv
    assert eng.so_response_function_complex([0.2j]).shape == (1, 1, 1)       # -z is the conjugate: one solve
    for z in (0.1 + 0.05j, 0.3j):                                            # z was solved, neither -z nor -conj z; 0.3i not at all
        with pytest.raises(AfespError, match="status 1: .*was not solved at z and at -z"):
            eng.so_response_function_complex([z])
    eng.so_response_init_complex(X[None], [0.1 + 0.05j, -0.1 + 0.05j], 16)   # -conj z serves as the partner of z
    for it in range(100):
        _, _, conv = eng.so_response_iterate(1e-8)
        if conv:
            break
    a = eng.so_response_function_complex([0.1 + 0.05j])
    eng.so_response_init_complex(X[None], [0.1 + 0.05j, -0.1 - 0.05j], 16)
    for it in range(100):
        _, _, conv = eng.so_response_iterate(1e-8)
        if conv:
            break
    b = eng.so_response_function_complex([0.1 + 0.05j])
    assert abs(a[0, 0, 0] - b[0, 0, 0]) < 1e-7 * abs(b[0, 0, 0])
    # a complex entry point on a real state
    eng.so_response_init(X[None], [0.0], 8)
    for call in (lambda: eng.so_response_function_complex([0.0]), lambda: eng.so_response_vector_complex(0, 0)):
        with pytest.raises(AfespError, match="status 1: .*made for real frequencies"):
            call()
    with pytest.raises(AfespError, match="status 27: .*not converged"):      # maxiter = 1 at a tight tol
        response.so_response_solve_complex(eng, [X], [0.1 + 0.02j], tol=1e-13, maxiter=1)
    # ---- stale after anything that may have written t or lambda
    eng.so_response_init_complex(X[None], [0.2j], 8)
    eng.so_set_lambda(*eng.so_lambda())
    for call in (lambda: eng.so_response_iterate(), lambda: eng.so_response_function_complex([0.2j]), lambda: eng.so_response_vector_complex(0, 0)):
        with pytest.raises(AfespError, match="status 21: .*stale"):
            call()
    eng.so_response_init_complex(X[None], [0.2j], 8)
    eng.so_response_iterate()
    eng.so_set_amplitudes(*eng.so_amplitudes())
    for call in (lambda: eng.so_response_iterate(), lambda: eng.so_response_function_complex([0.2j]),
                 lambda: eng.so_response_init_complex(X[None], [0.2j], 8)):
        with pytest.raises(AfespError, match="status 21: .*stale"):
            call()


def test_a_damped_frequency_at_a_converged_eom_root_is_no_pole(eng):
    """the frequency that test_gpu_response.py shows to be a pole (status 26) has a response once it is damped"""
    c = np_eom.converged_model("o4v6")
    o, v = c["o"], c["v"]
    _feed_model(eng, c)
    omega, R, info = eom.so_eom_solve(eng, 4, tol=1e-9, maxiter=300)
    k = int(np.argmax(info["r1_norm2"]))
    X = np.zeros((o + v, o + v))
    X[:o, o:] = np.abs(R[k][0])
    X = X + X.T
    with pytest.raises(AfespError, match="status 26: .*frequency at a pole"):
        response.so_response_solve_complex(eng, [X], [omega[k] + 0.0j], tol=1e-8)
    rf, _ = response.so_response_solve_complex(eng, [X], [omega[k] + 0.01j], tol=1e-8)
    assert np.isfinite(rf).all() and -rf[0, 0, 0].imag > 0.0                # on the pole: Im alpha ~ strength / gamma


def test_a_complex_response_solve_changes_nothing_else(eng):
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
    rf, rinfo = response.so_response_solve_complex(eng, ops, [0.2j, 0.05 + 0.02j])
    assert rinfo["nsigma"] >= 9 and np.isfinite(rf).all()
    nvec = c["o"] * c["v"] + (c["o"] * c["v"]) ** 2
    assert (eng.arena_stats()["live_gb"] - live0) * 1e9 >= 8 * (2 * rinfo["max_space"] + 8 * 9) * nvec    # a basis of its own, two columns per system
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
