"""GPU parity of EOM-IP-CCSD and EOM-EA-CCSD on the spin-orbital state (afesp_ccsd_so_eom_ipea_*, afesp_amd.eom): the sigma build of both
sectors against the ghost-orbital definition of np_eom_ipea at the shapes of tests/test_gpu_lambda.py, the Davidson iteration against the
eigenvalues of the sector matrices on four converged models (np_eom.MODELS) and against the one-electron spectrum for two electrons, that
a solve changes nothing else, that both sectors' states live beside an EE state, and the statuses.

Tolerances: 1e-11 x max(1, max |ref|) for sigma at equal amplitudes; 1e-8 for omega at tol = 1e-8; 10 tol for the residual
norm recomputed from the returned vectors.

The device's guesses are unit vectors with a fixed 1e-3 admixture of every unique amplitude (np_eom_ipea.guess_vector restates them): with
bare unit vectors IP with 6 roots on o4v6, o4v6_canonical and o4v8 would miss the fifth eigenvalue, the Ms = -3/2 component of a 2h1p
quartet (tests/test_eom_ipea_cpu.py keeps that on record).

Not covered here: a recording context (Context::rec) is refused by every entry point as by EOM-EE's, but no call of the C interface
leaves a context recording, so the refusal cannot be reached from a test."""
import numpy as np
import pytest

import np_eom
import np_eom_ipea as X
import np_lambda
from afesp_amd import density, eom
from afesp_amd.capi import AfespError
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


def _antisymmetric_to_the_bit(sec, x2):
    return np.array_equal(x2, -(x2.transpose(1, 0, 2) if sec == X.IP else x2.transpose(0, 2, 1)))


@pytest.mark.parametrize("sector", sorted(SECTORS))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_sigma_equals_the_ghost_orbital_definition_at_random_amplitudes(eng, name, sector):
    """at O(0.3) random t and r: a missing or mis-signed term shows at 1e-2 and upward"""
    sec = SECTORS[sector]
    c = _case(name)
    o, v = c["o"], c["v"]
    rng = np.random.default_rng(17)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    rs = [X.random_vector(rng, sec, o, v) for _ in range(3)]
    _feed(eng, c)
    eng.so_set_amplitudes(t1, t2)
    eng.so_lambda_init(0)
    s1, s2 = eng.so_eom_ipea_sigma(sec, np.stack([r[0] for r in rs]), np.stack([r[1] for r in rs]))       # nvec = 3 in one call
    for k, (r1, r2) in enumerate(rs):
        d1, d2, leak = X.sigma_definition(sec, c["g"], c["f"], o, t1, t2, r1, r2)
        assert leak == 0.0
        _close(s1[k], d1, 1e-11, f"{sector} {name} sigma1 of vector {k}")
        _close(s2[k], d2, 1e-11, f"{sector} {name} sigma2 of vector {k}")
        assert _antisymmetric_to_the_bit(sec, s2[k])
        a1, a2 = eng.so_eom_ipea_sigma(sec, r1, r2)                         # ... equals three calls bit for bit
        assert np.array_equal(a1, s1[k]) and np.array_equal(a2, s2[k])
    if o == 1 and sec == X.IP:
        assert not np.any(s2) and np.any(s1)                                # no 2h1p amplitude: sigma1 alone answers
    a1, a2 = eng.so_amplitudes()
    assert np.array_equal(a1, t1) and np.array_equal(a2, t2)


def test_one_occupied_spin_orbital_limits_the_ip_roots_and_still_solves(eng):
    c = _case("one_electron")
    o, v = c["o"], c["v"]
    assert (o, v) == (1, 5)
    _feed(eng, c)
    eng.so_lambda_init(0)
    with pytest.raises(AfespError, match="status 1: .*nroots must be in 1 .. 1 "):
        eng.so_eom_ipea_init(X.IP, 2, 4)
    omega, vectors, info = eom.so_eom_ip_solve(eng, 1)
    I = np_lambda.hbar(c["cc"], *eng.so_amplitudes())
    ref = X.matrix(X.IP, c["cc"], *eng.so_amplitudes(), I)
    assert ref.shape == (1, 1) and abs(omega[0] - ref[0, 0]) < 1e-11 and info["nsigma"] == 1
    assert abs(abs(vectors[0][0][0]) - 1.0) < 1e-15 and not np.any(vectors[0][1])
    with pytest.raises(AfespError, match=f"status 1: .*nroots must be in 1 .. {v + o * v * (v - 1) // 2} "):
        eng.so_eom_ipea_init(X.EA, v + o * v * (v - 1) // 2 + 1, 4096)
    omega, _, _ = eom.so_eom_ea_solve(eng, 2)
    w = np.linalg.eigvals(X.matrix(X.EA, c["cc"], *eng.so_amplitudes(), I))
    w = w[np_eom.sort_roots(w)]
    assert np.max(np.abs(omega - w[:2].real)) < 1e-8


def _residual_norms(eng, sec, omega, vectors):
    out = []
    for w, (x1, x2) in zip(omega, vectors):
        s1, s2 = eng.so_eom_ipea_sigma(sec, x1, x2)
        out.append(np.sqrt(X.dot(s1 - w * x1, s2 - w * x2, s1 - w * x1, s2 - w * x2)))
    return np.array(out)


@pytest.mark.parametrize("sector", sorted(SECTORS))
@pytest.mark.parametrize("name", sorted(np_eom.MODELS))
@pytest.mark.parametrize("nroots", [4, 6])
def test_davidson_finds_the_lowest_roots_of_the_sector(eng, name, nroots, sector):
    sec = SECTORS[sector]
    c = X.converged_sector(name, sec)
    w = c["w"].real
    _feed_model(eng, c)
    tol = 1e-8
    max_space, collapses = X.davidson_case(name, sec, nroots)
    solve = eom.so_eom_ip_solve if sec == X.IP else eom.so_eom_ea_solve
    runs = []
    for _ in range(2):
        omega, vectors, info = solve(eng, nroots, tol=tol, max_space=max_space, maxiter=1000)   # (the slowest case: 280 steps)
        print(sector, name, nroots, "max_space", info["max_space"], info["iterations"], "steps", info["nsigma"], "sigma builds, omega - w",
              np.max(np.abs(omega - w[:nroots])), "omega", omega, "w", w[:nroots + 2])
        assert not info["complex"] and np.all(info["flags"] & eom.FLAG_CONVERGED)
        res = _residual_norms(eng, sec, omega, vectors)
        print(sector, name, nroots, "recomputed residual norms", res)
        assert np.all(res < 10.0 * tol)
        for x1, x2 in vectors:
            assert abs(X.dot(x1, x2, x1, x2) - 1.0) < 1e-12 and _antisymmetric_to_the_bit(sec, x2)
        runs.append((omega, vectors, info))
    if collapses:
        assert runs[0][2]["nsigma"] > max_space                             # more sigma builds than basis vectors fit: it collapsed
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][2]["nsigma"] == runs[1][2]["nsigma"]
    for (a1, a2), (b1, b2) in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2)            # a second run: identical bits
    assert np.max(np.abs(runs[0][0] - w[:nroots])) < 1e-8


def test_two_electron_ips_are_the_one_electron_levels(eng):
    """CCSD is exact for two electrons: E(N) + omega_IP is an eigenvalue of h, and a closed-shell reference shows each doublet twofold"""
    c = _build_case("two_electron", "fock", 4, 1, 1, 21)
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-13, 1e-13)
    assert nit > 0
    eng.so_lambda_init(0)
    omega, vectors, info = eom.so_eom_ip_solve(eng, 4, tol=1e-10)
    e0 = np_lambda.fci_two_electron_density(c["h"], c["chem"])[0]
    lev = np.linalg.eigvalsh(c["h"])
    print("E(N) + omega", e0 + omega, "eig(h)", lev, "degeneracy", info["degeneracy"])
    assert np.max(np.abs(np.sort(e0 + omega) - np.repeat(lev[:2], 2))) < 1e-9
    assert list(info["degeneracy"]) == [2, 2, 2, 2]
    labels = [eom.label_ipea_root(eom.SECTOR_IP, x1, x2, c["n"], 1, 1, False) for x1, x2 in vectors]
    print([(l["kind"], l["occ"], l["virt"], l["delta_ms"]) for l in labels])
    assert all(l["delta_ms"] in (-0.5, 0.5) for l in labels)


def test_ip_and_ea_solves_change_nothing_else_and_live_beside_an_ee_state(eng):
    c = _case("uhf_fed")
    o, v = c["o"], c["v"]
    _feed(eng, c)
    nit, _, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    e_t = eng.do_ccsd_t_spinorb()
    density.so_lambda_solve(eng, 300, 1e-11, 1e-11)
    r1, r2 = np_lambda.antisym_random(np.random.default_rng(5), o, v)
    ee_omega, _, ee_info = eom.so_eom_solve(eng, 3)
    first = eng.so_eom_iterate(1e-8)
    before = (*eng.so_amplitudes(), *eng.so_lambda(), eng.so_density(), *eng.so_eom_sigma(r1, r2), *eng.so_eom_vector(1))
    ip, _, ip_info = eom.so_eom_ip_solve(eng, 3)
    ea, _, ea_info = eom.so_eom_ea_solve(eng, 3)
    assert np.all(ip > 0.0) and ip_info["nsigma"] >= 3 and ea_info["nsigma"] >= 3
    after = (*eng.so_amplitudes(), *eng.so_lambda(), eng.so_density(), *eng.so_eom_sigma(r1, r2), *eng.so_eom_vector(1))
    for a, b in zip(before, after):
        assert np.array_equal(a, b)                                         # t1, t2, l1, l2, the density, an EE sigma, an EE Ritz vector
    assert eng.do_ccsd_t_spinorb() == e_t
    again = eng.so_eom_iterate(1e-8)                                        # the EE state is still there and steps as before ...
    assert np.array_equal(first[0], again[0]) and first[3] == again[3]
    ip2 = eng.so_eom_ipea_iterate(X.IP, 1e-8)                               # ... and so are both sectors' states
    ea2 = eng.so_eom_ipea_iterate(X.EA, 1e-8)
    assert np.array_equal(ip2[0], ip) and np.array_equal(ea2[0], ea) and ip2[4] and ea2[4]
    eng.so_lambda_iterate(1e-11, 1e-11)                                     # the Lambda state is still live


def test_the_callers_guesses_replace_the_unit_guesses(eng):
    c = _case("rhf_fed")
    o, v = c["o"], c["v"]
    _feed(eng, c)
    eng.so_lambda_init(0)
    for sec in (X.IP, X.EA):
        rng = np.random.default_rng(23)
        (p1, p2), (q1, q2) = X.random_vector(rng, sec, o, v), X.random_vector(rng, sec, o, v)
        eng.so_eom_ipea_init(sec, 2, 8)
        eng.so_eom_ipea_guess(sec)
        eng.so_eom_ipea_set_guess(sec, 1, p1, p2)                           # starts over: column 0 is zero and dropped
        assert eng.so_eom_ipea_iterate(sec, 1e-8)[3] == 1
        eng.so_eom_ipea_set_guess(sec, 0, q1, q2)
        eng.so_eom_ipea_set_guess(sec, 1, p1, p2)
        assert eng.so_eom_ipea_iterate(sec, 1e-8)[3] == 2
        x1, x2 = eng.so_eom_ipea_vector(sec, 0)
        span = np.array([X.pack(sec, a, b) for a, b in ((q1, q2), (p1, p2))]).T
        y = X.pack(sec, x1, x2)
        assert np.linalg.norm(y - span @ np.linalg.lstsq(span, y, rcond=None)[0]) < 1e-12   # the Ritz vector lies in their span
        eng.so_eom_ipea_guess(sec)
        assert eng.so_eom_ipea_iterate(sec, 1e-8)[3] == 2


def test_statuses_and_release(eng):
    c = _case("rhf_fed")
    o, v = c["o"], c["v"]
    _feed(eng, c)
    vec = {sec: X.random_vector(np.random.default_rng(3), sec, o, v) for sec in (X.IP, X.EA)}
    for sec in (X.IP, X.EA):
        for call in (lambda: eng.so_eom_ipea_init(sec, 2, 8), lambda: eng.so_eom_ipea_sigma(sec, *vec[sec])):
            with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
                call()
    eng.so_lambda_init(0)
    for bad in (0, 3, -1):
        for call in (lambda: eng.so_eom_ipea_init(bad, 2, 8), lambda: eng.so_eom_ipea_guess(bad), lambda: eng.so_eom_ipea_iterate(bad),
                     lambda: eng.so_eom_ipea_set_guess(bad, 0, *vec[X.IP])):
            with pytest.raises(AfespError, match="status 1: .*sector must be"):
                call()
    for sec in (X.IP, X.EA):
        nunique, nvec = eom.ipea_nunique(sec, o, v), sum(int(np.prod(s)) for s in eng.so_eom_ipea_shapes(sec))
        for nroots, max_space in ((0, 8), (-1, 8), (nunique + 1, 4096), (3, 5), (2, 5000)):
            with pytest.raises(AfespError, match="status 1: .*(nroots|max_space) must be"):
                eng.so_eom_ipea_init(sec, nroots, max_space)
        eng._eom_nroots = {sec: 2}
        for call in (lambda: eng.so_eom_ipea_guess(sec), lambda: eng.so_eom_ipea_iterate(sec), lambda: eng.so_eom_ipea_vector(sec, 0),
                     lambda: eng.so_eom_ipea_set_guess(sec, 0, *vec[sec])):
            with pytest.raises(AfespError, match="status 21: .*no EOM-(IP|EA) state"):
                call()
        eng.so_eom_ipea_sigma(sec, *vec[sec])                               # needs the Lambda state only (its scratch is there from now on)
        live0 = eng.arena_stats()["live_gb"]
        eng.so_eom_ipea_init(sec, 2, 400)
        live1 = eng.arena_stats()["live_gb"]
        assert (live1 - live0) * 1e9 >= 8 * 2 * 400 * nvec
        with pytest.raises(AfespError, match="status 1: .*no guess vectors"):
            eng.so_eom_ipea_iterate(sec)
        with pytest.raises(AfespError, match="status 1: .*tol must be positive"):
            eng.so_eom_ipea_iterate(sec, 0.0)
        eng.so_eom_ipea_guess(sec)
        first = eng.so_eom_ipea_iterate(sec, 1e-8)
        with pytest.raises(AfespError, match="status 1: .*no Ritz vector"):
            eng.so_eom_ipea_vector(sec, 2)
        other = X.EA if sec == X.IP else X.IP
        if sec == X.IP:
            with pytest.raises(AfespError, match="status 21: .*no EOM-EA state"):   # an init of one sector is none of the other
                eng.so_eom_ipea_iterate(other)
        eng.so_lambda_init(0)                                               # releases the sector's state with the Lambda state it borrowed from
        assert (live1 - eng.arena_stats()["live_gb"]) * 1e9 >= 0.9 * 8 * 2 * 400 * nvec
        with pytest.raises(AfespError, match="status 21: .*no EOM-(IP|EA) state"):
            eng.so_eom_ipea_iterate(sec)
        eng.so_eom_ipea_init(sec, 2, 400)                                   # ... and a new one serves again, with the same numbers
        eng.so_eom_ipea_guess(sec)
        again = eng.so_eom_ipea_iterate(sec, 1e-8)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[3] == again[3]
    t1, t2 = eng.so_amplitudes()
    eng.so_set_amplitudes(t1, t2)                                           # may have changed t: stale, whatever was written
    for sec in (X.IP, X.EA):
        for call in (lambda: eng.so_eom_ipea_iterate(sec), lambda: eng.so_eom_ipea_sigma(sec, *vec[sec]), lambda: eng.so_eom_ipea_guess(sec),
                     lambda: eng.so_eom_ipea_init(sec, 2, 8)):
            with pytest.raises(AfespError, match="status 21: .*stale"):
                call()
    live_stale = eng.arena_stats()["live_gb"]
    _feed(eng, c)                                                           # a new state: everything of the old one is released (so_free)
    nvec_ea = v + o * v * v
    assert (live_stale - eng.arena_stats()["live_gb"]) * 1e9 >= 0.9 * 8 * 2 * 400 * nvec_ea
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
        eng.so_eom_ipea_guess(X.IP)
    _feed(eng, c, published=False)
    with pytest.raises(AfespError, match="status 20: .*F_mi"):
        eng.so_lambda_init(0)
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
        eng.so_eom_ipea_init(X.EA, 2, 8)
