"""GPU parity of the left-hand side of EOM-IP-CCSD and EOM-EA-CCSD on the spin-orbital state (afesp_ccsd_so_eom_ipea_lsigma, _left_*,
_dyson; afesp_amd.eom): the left sigma build of both sectors against the ghost-orbital definition of np_eom_ipea_left at the shapes of
tests/test_gpu_lambda.py and against the GPU's own right-hand build, the left Davidson iteration on the four converged models of
np_eom.MODELS, the Dyson vectors against the ghost row of the bilinear density, two exactly solvable models against FCI through the Python
drivers, that nothing else is written, and the statuses.

Tolerances: 1e-11 x max(1, max |ref|) for sigma_L and the Dyson vectors at equal amplitudes; 1e-12 x max(1, |<l, sigma(r)>|)
for the adjoint identity between the two device builds; 1e-8 for omega at tol = 1e-8; 10 tol for the residual norm recomputed from the
returned vectors; 1e-9 against FCI.

Step limits of the Davidson runs: the numpy reference iteration on A^T needs at most 151 steps from the right vectors with four basis
vectors per root (o4v6_canonical, IP, 6 roots) and at most 27 from the library's guesses with the default space; the limits here are
1000 and 300."""
import numpy as np
import pytest

import np_eom
import np_eom_ipea as X
import np_eom_ipea_left as XL
import np_lambda
import np_ucc
from afesp_amd import density, eom
from afesp_amd.capi import AfespError
from test_eom_ipea_left_cpu import check_ea_one_electron_poles, check_ip_two_electron_poles, one_electron_case
from test_gpu_eom import _feed_model
from test_gpu_lambda import SHAPES, _build_case, _case, _close, _feed

pytestmark = pytest.mark.gpu

SECTORS = {"IP": X.IP, "EA": X.EA}


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _exchanged(sec, x2):
    return x2.transpose(1, 0, 2) if sec == X.IP else x2.transpose(0, 2, 1)


@pytest.mark.parametrize("sector", sorted(SECTORS))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_left_sigma_equals_the_ghost_orbital_definition_at_random_amplitudes(eng, name, sector):
    """sigma_L(l) = A^T l at O(0.3) random t and l, and <l, sigma(r)> = <sigma_L(l), r> against the right-hand build.  The shapes hold
    (o, v) = (1, 5) -- IP without doubles, EA without the pair-form ladder array -- and (2, 2): EA with the direct ladder"""
    sec = SECTORS[sector]
    c = _case(name)
    o, v = c["o"], c["v"]
    rng = np.random.default_rng(41)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    ls = [X.random_vector(rng, sec, o, v) for _ in range(3)]
    r1, r2 = X.random_vector(rng, sec, o, v)
    _feed(eng, c)
    eng.so_set_amplitudes(t1, t2)
    eng.so_lambda_init(0)
    s1, s2 = eng.so_eom_ipea_lsigma(sec, np.stack([l[0] for l in ls]), np.stack([l[1] for l in ls]))       # nvec = 3 in one call
    q1, q2 = eng.so_eom_ipea_sigma(sec, r1, r2)
    for k, (l1, l2) in enumerate(ls):
        d1, d2, leak = XL.lsigma_definition(sec, c["g"], c["f"], o, t1, t2, l1, l2)
        assert leak == 0.0
        _close(s1[k], d1, 1e-11, f"{sector} {name} left sigma1 of vector {k}")
        _close(s2[k], d2, 1e-11, f"{sector} {name} left sigma2 of vector {k}")
        assert np.array_equal(s2[k], -_exchanged(sec, s2[k]))               # antisymmetric to the bit ...
        diag = s2[k][np.arange(o), np.arange(o)] if sec == X.IP else s2[k][:, np.arange(v), np.arange(v)]
        assert not np.any(diag)                                             # ... and zero on the pair diagonal
        a1, a2 = eng.so_eom_ipea_lsigma(sec, l1, l2)                        # ... equals three calls bit for bit
        assert np.array_equal(a1, s1[k]) and np.array_equal(a2, s2[k])
        lhs, rhs = X.dot(l1, l2, q1, q2), X.dot(s1[k], s2[k], r1, r2)
        print(sector, name, "adjoint", lhs, rhs, "error", abs(lhs - rhs))
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    if o == 1 and sec == X.IP:
        assert not np.any(s2) and np.any(s1)                                # no 2h1p amplitude: sigma_L1 alone answers
    a1, a2 = eng.so_amplitudes()
    assert np.array_equal(a1, t1) and np.array_equal(a2, t2)


def _left_residual_norms(eng, sec, omega, vectors):
    out = []
    for w, (x1, x2) in zip(omega, vectors):
        s1, s2 = eng.so_eom_ipea_lsigma(sec, x1, x2)
        out.append(np.sqrt(X.dot(s1 - w * x1, s2 - w * x2, s1 - w * x1, s2 - w * x2)))
    return np.array(out)


@pytest.mark.parametrize("sector", sorted(SECTORS))
@pytest.mark.parametrize("name", sorted(np_eom.MODELS))
@pytest.mark.parametrize("nroots", [4, 6])
def test_left_davidson_finds_the_roots_of_the_sector(eng, name, nroots, sector):
    """(a) from the GPU's right vectors with four basis vectors per root, twice; (b) from the library's guesses with the default space"""
    sec = SECTORS[sector]
    c = X.converged_sector(name, sec)
    ref = c["w"][:nroots].real
    _feed_model(eng, c)
    tol = 1e-8
    ip = sec == X.IP
    max_space, _ = X.davidson_case(name, sec, nroots)
    omega_r, R, _ = (eom.so_eom_ip_solve if ip else eom.so_eom_ea_solve)(eng, nroots, tol=tol, max_space=max_space, maxiter=1000)
    solve = eom.so_eom_ip_left_solve if ip else eom.so_eom_ea_left_solve
    runs = []
    for ms, guess, maxiter in ((max_space, R, 1000), (max_space, R, 1000), (None, None, 300)):
        omega, vectors, info = solve(eng, guess, nroots, tol=tol, max_space=ms, maxiter=maxiter)
        print(sector, name, nroots, "max_space", info["max_space"], info["iterations"], "steps", info["nsigma"], "left sigma builds, omega error",
              np.max(np.abs(omega - ref)), "against the right roots", np.max(np.abs(omega - omega_r)))
        assert np.max(np.abs(omega - ref)) < 1e-8 and np.max(np.abs(omega - omega_r)) < 1e-8
        assert not info["complex"] and np.all(info["flags"] & eom.FLAG_CONVERGED)
        res = _left_residual_norms(eng, sec, omega, vectors)
        print(sector, name, nroots, "recomputed residual norms", res)
        assert np.all(res < 10.0 * tol)
        for x1, x2 in vectors:
            assert abs(X.dot(x1, x2, x1, x2) - 1.0) < 1e-12 and np.array_equal(x2, -_exchanged(sec, x2))
        runs.append((omega, vectors, info))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][2]["nsigma"] == runs[1][2]["nsigma"]
    for (a1, a2), (b1, b2) in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2)            # a second run: identical bits


@pytest.mark.parametrize("sector", sorted(SECTORS))
@pytest.mark.parametrize("name", ["uhf_fed", "fock_rotated", "two_electron", "one_electron"])
def test_dyson_vectors_equal_the_ghost_row_of_the_density(eng, name, sector):
    """(o,v) = (4,6) with unequal spins, (3,5) with every f term, (2,2) and (1,5); random t, lambda, l, r; every NULL combination"""
    sec = SECTORS[sector]
    c = _case(name)
    o, v = c["o"], c["v"]
    rng = np.random.default_rng(43)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    lam = np_lambda.antisym_random(rng, o, v)
    ls, rs = [X.random_vector(rng, sec, o, v) for _ in range(2)], [X.random_vector(rng, sec, o, v) for _ in range(2)]
    stack = lambda xs: (np.stack([x[0] for x in xs]), np.stack([x[1] for x in xs]))
    _feed(eng, c)
    eng.so_set_amplitudes(t1, t2)
    eng.so_lambda_init(0)
    eng.so_set_lambda(*lam)
    gl, gr = eng.so_eom_ipea_dyson(sec, stack(ls), stack(rs))               # nvec = 2, both sides
    assert gl.shape == gr.shape == (2, o + v)
    for k in range(2):
        dl, dr = XL.dyson_definition(sec, c["g"], c["f"], o, t1, t2, *lam, ls[k], rs[k])
        _close(gl[k], dl, 1e-11, f"{sector} {name} left Dyson vector {k}")
        _close(gr[k], dr, 1e-11, f"{sector} {name} right Dyson vector {k}")
        a, none = eng.so_eom_ipea_dyson(sec, ls[k], None)                   # one side alone, one vector: the same bits
        assert none is None and np.array_equal(a, gl[k])
        none, b = eng.so_eom_ipea_dyson(sec, None, rs[k])
        assert none is None and np.array_equal(b, gr[k])
    again = eng.so_eom_ipea_dyson(sec, stack(ls), stack(rs))
    assert np.array_equal(again[0], gl) and np.array_equal(again[1], gr)    # a repeat: identical to the bit
    assert eng.so_eom_ipea_dyson(sec, None, None) == (None, None)
    for half in (((ls[0][0], None), None), (None, (None, rs[0][1])), ((None, ls[0][1]), rs[0])):
        with pytest.raises(AfespError, match="status 1: .*both NULL or both given"):
            eng.so_eom_ipea_dyson(sec, *half)
    a1, a2 = eng.so_amplitudes()
    b1, b2 = eng.so_lambda()
    assert np.array_equal(a1, t1) and np.array_equal(a2, t2) and np.array_equal(b1, lam[0]) and np.array_equal(b2, lam[1])


def _all_roots_with_poles(eng, sec, nroots):
    ip = sec == X.IP
    omega, R, _ = (eom.so_eom_ip_solve if ip else eom.so_eom_ea_solve)(eng, nroots, tol=1e-11, max_space=2 * nroots, maxiter=300)
    wl, L, _ = (eom.so_eom_ip_left_solve if ip else eom.so_eom_ea_left_solve)(eng, R, tol=1e-11, max_space=2 * nroots, maxiter=300)
    assert np.max(np.abs(wl - omega)) < 1e-9
    L = eom.biorthonormalise_ipea(omega, L, R)
    S = np.array([[eom.dot_ipea(l, r) for r in R] for l in L])
    print("biorthonormality", np.max(np.abs(S - np.eye(nroots))))
    assert np.max(np.abs(S - np.eye(nroots))) < 1e-9
    props = eom.so_eom_ipea_properties(eng, sec, L, R)
    return omega, props


def test_two_electron_ip_pole_strengths_are_fci(eng):
    """CCSD is exact for two electrons: through so_eom_ip_solve, so_eom_ip_left_solve, biorthonormalise_ipea and so_eom_ipea_properties
    every one of the 8 roots has FCI's pole strength (per twofold cluster), and they sum to the two electrons"""
    c = _build_case("two_electron", "fock", 4, 1, 1, 21)
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-13, 1e-13)
    assert nit > 0
    density.so_lambda_solve(eng, 300, 1e-12, 1e-12)
    omega, props = _all_roots_with_poles(eng, X.IP, 8)
    check_ip_two_electron_poles(c["h"], c["chem"], omega, [p["pole_strength"] for p in props])
    for p in props:                                                         # an ionisation of definite Ms: one spin part of each vector is zero
        for gam in (p["dyson_left"], p["dyson_right"]):
            a, b = eom.dyson_spin_parts(gam, 4, 1, 1, False)
            assert min(np.max(np.abs(a)), np.max(np.abs(b))) < 1e-9 or abs(omega[0] - omega[1]) < 1e-6


def test_one_electron_ea_pole_strengths_are_fci(eng):
    """one electron in the lowest eigenvector of h: t = 0, and the 28 roots of the EA sector are the two-electron FCI states with the weight
    of their configurations that hold the reference's electron; the strengths sum to the 7 empty spin orbitals"""
    eps, chem_e, fa, fb, _ = one_electron_case()
    n = len(eps)
    eng.do_mp2_spatial(n, 1, np.eye(n), np.arange(n, dtype=np.float64), np_ucc.pack8(chem_e), want_eri_mo=False)
    eng.mo_rotate_uhf(n, np.eye(n), np.eye(n))
    eng.uso_init_fock(n, 1, 0, fa, fb, 8)
    assert (eng.so_o, eng.so_v) == (1, 7)
    eng.do_ccsd_spinorb(300, 1e-13, 1e-13)
    t1, t2 = eng.so_amplitudes()
    assert np.max(np.abs(t1)) < 1e-13 and np.max(np.abs(t2)) < 1e-13
    density.so_lambda_solve(eng, 300, 1e-12, 1e-12)
    omega, props = _all_roots_with_poles(eng, X.EA, 28)
    check_ea_one_electron_poles(eps, chem_e, omega, [p["pole_strength"] for p in props])


def test_left_solves_and_dyson_calls_change_nothing_else_and_all_six_kinds_step_on(eng):
    c = _case("uhf_fed")
    o, v = c["o"], c["v"]
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    e_t = eng.do_ccsd_t_spinorb()
    density.so_lambda_solve(eng, 300, 1e-11, 1e-11)
    r1, r2 = np_lambda.antisym_random(np.random.default_rng(5), o, v)
    ee, Ree, _ = eom.so_eom_solve(eng, 3)
    eel, _, _ = eom.so_eom_left_solve(eng, Ree)
    ip, Rip, _ = eom.so_eom_ip_solve(eng, 3)
    ea, Rea, _ = eom.so_eom_ea_solve(eng, 3)
    state = lambda: (*eng.so_amplitudes(), *eng.so_lambda(), eng.so_density(), *eng.so_eom_sigma(r1, r2),
                     *[x for k in range(3) for sec in (X.IP, X.EA) for x in eng.so_eom_ipea_vector(sec, k)])
    before = state()
    ipl, Lip, info_ip = eom.so_eom_ip_left_solve(eng, Rip)
    eal, Lea, info_ea = eom.so_eom_ea_left_solve(eng, Rea)
    assert np.max(np.abs(ipl - ip)) < 1e-7 and np.max(np.abs(eal - ea)) < 1e-7 and info_ip["nsigma"] >= 3 and info_ea["nsigma"] >= 3
    eom.so_eom_ipea_properties(eng, X.IP, eom.biorthonormalise_ipea(ip, Lip, Rip), Rip)
    eom.so_eom_ipea_properties(eng, X.EA, eom.biorthonormalise_ipea(ea, Lea, Rea), Rea)
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)                                         # t1, t2, l1, l2, the density, an EE sigma, the right IP / EA vectors
    assert eng.do_ccsd_t_spinorb() == e_t
    steps = (eng.so_eom_iterate(1e-8), eng.so_eom_left_iterate(1e-8), eng.so_eom_ipea_iterate(X.IP, 1e-8), eng.so_eom_ipea_iterate(X.EA, 1e-8),
             eng.so_eom_ipea_left_iterate(X.IP, 1e-8), eng.so_eom_ipea_left_iterate(X.EA, 1e-8))
    for step, w in zip(steps, (ee, eel, ip, ea, ipl, eal)):                 # all six states are there and stay converged at their roots
        assert np.array_equal(step[0], w) and step[4]
    eng.so_lambda_iterate(1e-11, 1e-11)                                     # the Lambda state is still live


def test_statuses_and_release(eng):
    c = _case("rhf_fed")
    o, v = c["o"], c["v"]
    _feed(eng, c)
    vec = {sec: X.random_vector(np.random.default_rng(3), sec, o, v) for sec in (X.IP, X.EA)}
    for sec in (X.IP, X.EA):
        for call in (lambda: eng.so_eom_ipea_left_init(sec, 2, 8), lambda: eng.so_eom_ipea_lsigma(sec, *vec[sec]),
                     lambda: eng.so_eom_ipea_dyson(sec, vec[sec], vec[sec])):
            with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
                call()
    eng.so_lambda_init(0)
    for bad in (0, 3, -1):
        for call in (lambda: eng.so_eom_ipea_left_init(bad, 2, 8), lambda: eng.so_eom_ipea_left_guess(bad), lambda: eng.so_eom_ipea_left_iterate(bad),
                     lambda: eng.so_eom_ipea_left_set_guess(bad, 0, *vec[X.IP]),
                     lambda: eng._chk(eng.L.afesp_ccsd_so_eom_ipea_dyson(eng.h, bad, 1, None, None, None, None, None, None))):
            with pytest.raises(AfespError, match="status 1: .*sector must be"):
                call()
    for sec in (X.IP, X.EA):
        nunique, nvec = eom.ipea_nunique(sec, o, v), sum(int(np.prod(s)) for s in eng.so_eom_ipea_shapes(sec))
        for nroots, max_space in ((0, 8), (-1, 8), (nunique + 1, 4096), (3, 5), (2, 5000)):
            with pytest.raises(AfespError, match="status 1: .*afesp_ccsd_so_eom_ipea_left_init: (nroots|max_space) must be"):
                eng.so_eom_ipea_left_init(sec, nroots, max_space)
        eng._eom_nroots = {("left", sec): 2}
        eng.so_eom_ipea_init(sec, 2, 8)                                     # the right-hand state of the sector is none of the left one
        for call in (lambda: eng.so_eom_ipea_left_guess(sec), lambda: eng.so_eom_ipea_left_iterate(sec), lambda: eng.so_eom_ipea_left_vector(sec, 0),
                     lambda: eng.so_eom_ipea_left_set_guess(sec, 0, *vec[sec])):
            with pytest.raises(AfespError, match="status 21: .*no left EOM-(IP|EA) state"):
                call()
        eng.so_eom_ipea_lsigma(sec, *vec[sec])                              # needs the Lambda state only (its scratch is there from now on)
        eng.so_eom_ipea_dyson(sec, vec[sec], vec[sec])
        live0 = eng.arena_stats()["live_gb"]
        eng.so_eom_ipea_left_init(sec, 2, 400)
        live1 = eng.arena_stats()["live_gb"]
        assert (live1 - live0) * 1e9 >= 8 * 2 * 400 * nvec
        with pytest.raises(AfespError, match="status 1: .*no guess vectors"):
            eng.so_eom_ipea_left_iterate(sec)
        with pytest.raises(AfespError, match="status 1: .*tol must be positive"):
            eng.so_eom_ipea_left_iterate(sec, 0.0)
        eng.so_eom_ipea_left_guess(sec)
        first = eng.so_eom_ipea_left_iterate(sec, 1e-8)
        with pytest.raises(AfespError, match="status 1: .*no Ritz vector"):
            eng.so_eom_ipea_left_vector(sec, 2)
        eng.so_lambda_init(0)                                               # releases the state with the Lambda state it borrowed from
        assert (live1 - eng.arena_stats()["live_gb"]) * 1e9 >= 0.9 * 8 * 2 * 400 * nvec
        with pytest.raises(AfespError, match="status 21: .*no left EOM-(IP|EA) state"):
            eng.so_eom_ipea_left_iterate(sec)
        eng.so_eom_ipea_left_init(sec, 2, 400)                              # ... and a new one serves again, with the same numbers
        eng.so_eom_ipea_left_guess(sec)
        again = eng.so_eom_ipea_left_iterate(sec, 1e-8)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[3] == again[3]
    t1, t2 = eng.so_amplitudes()
    eng.so_set_amplitudes(t1, t2)                                           # may have changed t: stale, whatever was written
    for sec in (X.IP, X.EA):
        for call in (lambda: eng.so_eom_ipea_left_iterate(sec), lambda: eng.so_eom_ipea_lsigma(sec, *vec[sec]),
                     lambda: eng.so_eom_ipea_left_guess(sec), lambda: eng.so_eom_ipea_left_init(sec, 2, 8),
                     lambda: eng.so_eom_ipea_dyson(sec, vec[sec], None)):
            with pytest.raises(AfespError, match="status 21: .*stale"):
                call()
    live_stale = eng.arena_stats()["live_gb"]
    _feed(eng, c)                                                           # a new state: everything of the old one is released (so_free)
    nvec_ea = v + o * v * v
    assert (live_stale - eng.arena_stats()["live_gb"]) * 1e9 >= 0.9 * 8 * 2 * 400 * nvec_ea
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
        eng.so_eom_ipea_left_guess(X.IP)
    _feed(eng, c, published=False)
    with pytest.raises(AfespError, match="status 20: .*F_mi"):
        eng.so_lambda_init(0)
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
        eng.so_eom_ipea_left_init(X.EA, 2, 8)
