"""GPU parity of the orbital gradient, the Z-vector equations and the relaxed one-particle density of spin-orbital CCSD
(afesp_ccsd_so_orbital_gradient / _zvector_apply / _zvector_solve / _relaxed_density, afesp_amd.density.so_relaxed_density_solve) against
np_relax: gradient_explicit (X_pq = f D + 1/2 g Gamma over the whole arrays, itself held to the defining finite difference in
test_relax_cpu.py), hessian_dense and numpy's dense solve.

Shapes: those of test_gpu_lambda.py -- the interleaved RHF-fed state (4,6), unequal spin blocks (4,6), every f_ov / f_oo / f_vv term (3,5),
one pair each way (2,2) and no occupied pair at all (1,5: no va, Gamma_ovvv = ga = 0).  The Fock-fed shapes take the gradient and the
operator and refuse the solve (status 24).

Tolerances: 1e-11 x max(1, max |ref|) at equal amplitudes, 1e-9 for the separately converged z (tol = 1e-12)."""
import numpy as np
import pytest

import np_density2
import np_lambda
import np_relax
from afesp_amd import density
from afesp_amd.capi import AfespError
from test_gpu_lambda import SHAPES, _case, _close, _feed

pytestmark = pytest.mark.gpu

NAMES = ("oooo", "ooov", "oovv", "ovov", "ovvv", "vvvv_pairs")
_REF = {}


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _ref(name):
    """random O(0.3) t and lambda of a shape with the reference gradient, operator, z and relaxed density: made once, left unchanged"""
    if name not in _REF:
        c = _case(name)
        o, v, cc = c["o"], c["v"], c["cc"]
        rng = np.random.default_rng(7)
        t = np_lambda.antisym_random(rng, o, v)
        l = np_lambda.antisym_random(rng, o, v)
        D = np_lambda.density_explicit(cc, *t, *l)
        G = np_density2.gamma_explicit(*t, *l)
        F = np_density2.expand(G, o, v)
        w = [np_relax.gradient_explicit(c["g"], c["f"], o, D, F, fr) for fr in (0, 1)]
        _, terms = np_relax.gradient_blocks(cc, c["f"], D, G, 1)
        lev = np.diag(c["f"]).copy()
        A = np_relax.hessian_dense(c["g"], lev, o)
        z = np.linalg.solve(A, -w[1].reshape(-1)).reshape(o, v)
        _REF[name] = dict(c=c, t=t, l=l, D=D, w=w, terms=terms, A=A, z=z, D_rel=np_relax.relaxed_density(D, z, o))
    return _REF[name]


def _set(eng, r):
    _feed(eng, r["c"])
    eng.so_set_amplitudes(*r["t"])
    eng.so_lambda_init(0)
    eng.so_set_lambda(*r["l"])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gradient_operator_solve_and_density_at_random_amplitudes(eng, name):
    """a missing or mis-signed term of X shows at 1e-2 and upward"""
    r = _ref(name)
    c, o, v = r["c"], r["c"]["o"], r["c"]["v"]
    _set(eng, r)
    eng.so_density2_build()
    for fr in (0, 1):
        w = eng.so_orbital_gradient(fr)
        _close(w, r["w"][fr], 1e-11, f"{name} w fock_response={fr}")
        assert np.array_equal(eng.so_orbital_gradient(fr), w)                       # bit-identical repeat
    for which, key in ((0, "pair_ai"), (1, "pair_ia")):
        out, _ = eng.so_relax_pair_row(which)
        _close(out, r["terms"][key], 1e-11, f"{name} pair-row term {key}")
        if o == 1 or v < 2:
            assert not np.any(out)
    rng = np.random.default_rng(11)
    x = rng.uniform(-1.0, 1.0, (o, v))
    y = eng.so_zvector_apply(x)
    _close(y, (r["A"] @ x.reshape(-1)).reshape(o, v), 1e-11, f"{name} A x")
    assert np.array_equal(eng.so_zvector_apply(x), y)
    if c["src"] == "fock":
        with pytest.raises(AfespError, match="status 24: .*not stationary"):
            eng.so_zvector_solve(1e-12, 100)
        with pytest.raises(AfespError, match="status 24: .*not stationary"):
            eng.so_relaxed_density()
        assert np.array_equal(eng.so_orbital_gradient(1), eng.so_orbital_gradient(1))   # the engine serves on
    else:
        assert np.all(np.linalg.eigvalsh(r["A"]) > 0.0)
        z, it, res = eng.so_zvector_solve(1e-12, 200)
        print(name, "Z-vector iterations", it, "residual", res, "max |z|", np.max(np.abs(z)))
        assert 0 < it <= 200 and res < 1e-12
        _close(z, r["z"], 1e-9, f"{name} z")
        d = eng.so_relaxed_density()
        assert np.array_equal(d, d.T)
        _close(d, r["D_rel"], 1e-9, f"{name} relaxed density")
        d0 = eng.so_density()
        assert np.array_equal(d[:o, :o], d0[:o, :o]) and np.array_equal(d[o:, o:], d0[o:, o:])
        assert np.array_equal(d[:o, o:], d0[:o, o:] + 0.5 * z)
        z2, it2, res2 = eng.so_zvector_solve(1e-12, 200)
        assert np.array_equal(z2, z) and it2 == it and res2 == res
        assert np.array_equal(eng.so_relaxed_density(), d)
        d3, z3, it3 = density.so_relaxed_density_solve(eng, 1e-12, 200)
        assert np.array_equal(d3, d) and np.array_equal(z3, z) and it3 == it
    a1, a2 = eng.so_amplitudes()
    l1, l2 = eng.so_lambda()
    assert np.array_equal(a1, r["t"][0]) and np.array_equal(a2, r["t"][1]) and np.array_equal(l1, r["l"][0]) and np.array_equal(l2, r["l"][1])


@pytest.mark.parametrize("name", ["rhf_fed", "two_electron", "uhf_fed"])
def test_converged_state_spin_purity_and_the_exact_two_electron_case(eng, name):
    """at converged (spin-pure) t and lambda the spin-flip elements of w and z are exact zeros; for two electrons CCSD is exact, the
    unrelaxed density is FCI's and the orbital gradient of E_ref + E_CCSD, w_ai + 2 f_ia with fock_response = 1, vanishes to the
    convergence level"""
    c = _case(name)
    o, v, cc = c["o"], c["v"], c["cc"]
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    density.so_lambda_solve(eng, 300, 1e-11, 1e-11)
    eng.so_density2_build()
    t, l = eng.so_amplitudes(), eng.so_lambda()
    D = np_lambda.density_explicit(cc, *t, *l)
    F = np_density2.expand(np_density2.gamma_explicit(*t, *l), o, v)
    w = eng.so_orbital_gradient(1)
    _close(w, np_relax.gradient_explicit(c["g"], c["f"], o, D, F, 1), 1e-11, f"{name} converged w")
    _, spin = density.so_spin_order(c["n"], c["na"], c["nb"], c["src"] == "rhf")
    flip = spin[:o, None] != spin[None, o:]
    assert np.any(flip) and not np.any(w[flip])
    if name == "two_electron":                 # (not Hartree-Fock orbitals: the reference energy's own gradient 2 f_ia closes the sum)
        fov = c["f"][:o, o:]
        print("two-electron max |w + 2 f_ov|", np.max(np.abs(w + 2.0 * fov)), "max |w|", np.max(np.abs(w)))
        assert np.max(np.abs(w + 2.0 * fov)) < 1e-8 and np.max(np.abs(fov)) > 1e-3
        return
    d, z, it = density.so_relaxed_density_solve(eng, 1e-12, 200)
    print(name, "iterations", it, "max |z|", np.max(np.abs(z)))
    assert not np.any(z[flip])
    zr = np_relax.zvector(c["g"], np.diag(c["f"]).copy(), o, w)
    _close(z, zr, 1e-9, f"{name} converged z")
    assert np.array_equal(d, d.T) and np.array_equal(d, np_relax.relaxed_density(eng.so_density(), z, o))


def test_calls_do_not_interfere_bit_for_bit(eng):
    """t, lambda, the one-particle density, every density2 block, (T) and a Lambda iteration are the same bits with and without the
    relaxation calls before them"""
    r = _ref("uhf_fed")
    o, v = r["c"]["o"], r["c"]["v"]

    def rest():
        out = [eng.so_density()] + [eng.so_density2_get(k) for k in NAMES] + [eng.so_density2_energy()]
        out += [eng.do_ccsd_t_spinorb(), eng.so_lambda_t()]
        out += [eng.so_lambda_iterate(1e-11, 1e-11), *eng.so_lambda(), *eng.so_amplitudes()]
        return out
    _set(eng, r)
    eng.so_density2_build()
    plain = rest()
    _set(eng, r)
    eng.so_density2_build()
    eng.so_orbital_gradient(0)
    eng.so_orbital_gradient(1)
    eng.so_zvector_apply(np.ones((o, v)))
    eng.so_zvector_solve(1e-12, 200)
    eng.so_relaxed_density()
    eng.so_relax_pair_row(0)
    eng.so_relax_pair_row(1)
    for a, b in zip(rest(), plain):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_every_status_and_the_engine_after_each(eng):
    from afesp_amd.capi import Engine
    r = _ref("rhf_fed")
    c = r["c"]
    o, v = c["o"], c["v"]
    n = o + v
    x = np.ones((o, v))
    calls = (lambda: eng.so_orbital_gradient(1), lambda: eng.so_zvector_apply(x), lambda: eng.so_zvector_solve(1e-12, 200),
             lambda: eng.so_relaxed_density())
    with Engine(0) as fresh:                                           # no state at all
        fresh.so_o, fresh.so_v = o, v
        for call in (lambda: fresh.so_orbital_gradient(1), lambda: fresh.so_zvector_apply(x), lambda: fresh.so_zvector_solve(1e-12, 10),
                     lambda: fresh.so_relaxed_density()):
            with pytest.raises(AfespError, match="status 1: .*no spin-orbital CCSD state"):
                call()
    _feed(eng, c)
    for call in calls:
        with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
            call()
    eng.so_set_amplitudes(*r["t"])
    eng.so_lambda_init(0)
    eng.so_set_lambda(*r["l"])
    for call in calls:                                                 # a live Lambda state, no build
        with pytest.raises(AfespError, match="status 21: .*no two-particle density"):
            call()
    eng.so_density2_build()
    with pytest.raises(AfespError, match="status 21: .*no converged Z-vector"):
        eng.so_relaxed_density()                                       # no solve yet
    with pytest.raises(AfespError, match="status 22: .*needs"):
        eng.so_orbital_gradient(1, capacity=o * v - 1)
    with pytest.raises(AfespError, match="status 1: .*fock_response"):
        eng.so_orbital_gradient(2)
    L = eng.L
    buf = np.zeros(o * v)
    assert L.afesp_ccsd_so_orbital_gradient(eng.h, 1, None, 1 << 40) == 22
    assert L.afesp_ccsd_so_zvector_apply(eng.h, None, buf.ctypes.data) == 1
    assert L.afesp_ccsd_so_zvector_apply(eng.h, buf.ctypes.data, None) == 1
    assert L.afesp_ccsd_so_zvector_solve(eng.h, 0.0, 10, None, None, None) == 1
    assert L.afesp_ccsd_so_zvector_solve(eng.h, 1e-10, 0, None, None, None) == 1
    with pytest.raises(AfespError, match="status 25: .*tol not reached"):
        eng.so_zvector_solve(1e-12, 1)                                 # maxiter = 1 does not converge ...
    assert eng.so_zvector_last[0] == 1 and eng.so_zvector_last[1] > 1e-12
    with pytest.raises(AfespError, match="status 21: .*no converged Z-vector"):
        eng.so_relaxed_density()                                       # ... and leaves no usable solve
    w = eng.so_orbital_gradient(1)                                     # the engine serves after each refusal
    _close(w, r["w"][1], 1e-11, "w after the refusals")
    z, _, _ = eng.so_zvector_solve(1e-12, 200)
    d = eng.so_relaxed_density()
    with pytest.raises(AfespError, match="status 22: .*needs"):
        eng.so_relaxed_density(capacity=n * n - 1)
    assert L.afesp_ccsd_so_zvector_solve(eng.h, 1e-12, 200, None, None, None) == 0   # every output is optional
    assert np.array_equal(eng.so_relaxed_density(), d)
    l1, l2 = eng.so_lambda()
    eng.so_set_lambda(l1, l2)                                          # may have changed lambda: the build and the solve are stale
    for call in calls:
        with pytest.raises(AfespError, match="status 21: .*no two-particle density"):
            call()
    eng.so_density2_build()
    with pytest.raises(AfespError, match="status 21: .*no converged Z-vector"):
        eng.so_relaxed_density()
    z2, _, _ = eng.so_zvector_solve(1e-12, 200)
    assert np.array_equal(z2, z) and np.array_equal(eng.so_relaxed_density(), d)
    t1, t2 = eng.so_amplitudes()
    eng.so_set_amplitudes(t1, t2)                                      # may have changed t: the Lambda state itself is stale
    for call in calls:
        with pytest.raises(AfespError, match="status 21: .*stale"):
            call()
    eng.so_lambda_init(0)                                              # released with the Lambda state
    eng.so_set_lambda(*r["l"])
    eng.so_density2_build()
    with pytest.raises(AfespError, match="status 21: .*no converged Z-vector"):
        eng.so_relaxed_density()
    d4, z4, _ = density.so_relaxed_density_solve(eng, 1e-12, 200)
    assert np.array_equal(z4, z) and np.array_equal(d4, d)
    eng.so_lambda_init(0)                                              # so_relaxed_density_solve builds the density2 itself
    eng.so_set_lambda(*r["l"])
    d5, z5, _ = density.so_relaxed_density_solve(eng, 1e-12, 200)
    assert np.array_equal(z5, z) and np.array_equal(d5, d)
