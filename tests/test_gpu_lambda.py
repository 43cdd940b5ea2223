"""GPU parity of the spin-orbital CCSD Lambda equations and the unrelaxed one-particle density (afesp_ccsd_so_lambda_*,
afesp_ccsd_so_density, afesp_amd.density) against the complex-step / finite-difference reference of np_lambda.

Shapes: the smallest that reach every branch -- the interleaved RHF-fed state, unequal spin blocks, every f_ov / f_oo / f_vv term, one
pair each way (npo = npv = 1) and no occupied pair at all (the ladder's empty branch, l2 = 0).

Tolerances: 1e-11 x max(1, max |ref|) for tensors at equal amplitudes, 1e-9 for separately converged amplitudes
(e_tol = t_tol = l_tol = 1e-11), 1e-10 for the density built from them."""
import numpy as np
import pytest

import np_lambda
import np_rocc
import np_ucc
from afesp_amd import density
from afesp_amd.capi import AfespError

pytestmark = pytest.mark.gpu

SHAPES = {   # name: (source, n, nalpha, nbeta)
    "rhf_fed": ("rhf", 5, 2, 2),
    "uhf_fed": ("uhf", 5, 3, 1),
    "fock_rotated": ("fock", 4, 2, 1),
    "two_electron": ("fock", 2, 1, 1),
    "one_electron": ("fock", 3, 1, 0),
}


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _interleaved_integrals(chem, lev, nocc):
    """<pq||rs> and the levels over spin orbitals 2 P + spin (the RHF-fed state's order)"""
    n = chem.shape[0]
    orb, spin = np.arange(2 * n) // 2, np.arange(2 * n) % 2
    phys = chem[np.ix_(orb, orb, orb, orb)].transpose(0, 2, 1, 3)
    same = (spin[:, None] == spin[None, :]).astype(float)
    phys = phys * same[:, None, :, None] * same[None, :, None, :]
    return phys - phys.transpose(0, 1, 3, 2), lev[orb], 2 * nocc


_CASES = {}


def _case(name):
    """the numpy side of a shape, made once: integrals, the restatement, and how to feed the engine"""
    if name not in _CASES:
        _CASES[name] = _build_case(name, *SHAPES[name], 100 + sorted(SHAPES).index(name))
    return _CASES[name]


def _build_case(name, src, n, na, nb, seed):
    """(test_gpu_lambda_mid.py builds its shapes with this too)"""
    rng = np.random.default_rng(seed)
    if name == "two_electron":
        h, chem, fa, fb = np_lambda.two_electron_model(n, seed)
    else:
        _, _, _, blk = np_lambda.model(n, na, nb, seed, canonical=(src != "fock"))
        chem, fa, fb, h = blk["chem"], blk["fa"], blk["fb"], None
    packed = np_ucc.pack8(chem)
    c = dict(name=name, src=src, n=n, na=na, nb=nb, packed=packed, h=h, chem=chem)
    if src == "rhf":
        lev = np.diag(fa).copy()
        g, lev_so, o = _interleaved_integrals(chem, lev, na)
        c.update(cc=np_rocc.ROCC(g, np.diag(lev_so), o), g=g, f=np.diag(lev_so), lev=lev)
    else:
        ident = name == "two_electron"          # (its FCI reference is in the orbitals of h)
        ua = np.eye(n) if ident else np_rocc.random_orthogonal(rng, n, 0.3)
        ub = np.eye(n) if ident else np_rocc.random_orthogonal(rng, n, 0.3)
        aa, ab, bb = np_ucc.mo_blocks(n, ua, ub, packed)
        g, _, o = np_ucc.so_integrals(aa, ab, bb, np.diag(fa).copy(), np.diag(fb).copy(), na, nb)
        f = np_rocc.so_fock(fa, fb, na, nb)
        c.update(cc=np_rocc.ROCC(g, f, o), g=g, f=f, ua=ua, ub=ub, fa=fa, fb=fb)
    c["o"], c["v"] = c["cc"].o, c["cc"].v
    return c


def _feed(eng, c, published=True):
    n = c["n"]
    if c["src"] == "rhf":
        eng.init_cc_spinorb(n, 2 * c["na"], c["lev"], eri_mo=c["packed"], diis_nerr=8, foo_as_published=published)
        return
    eng.do_mp2_spatial(n, 1, np.eye(n), np.arange(n, dtype=np.float64), c["packed"], want_eri_mo=False)   # (makes the array resident)
    eng.mo_rotate_uhf(n, c["ua"], c["ub"])
    if c["src"] == "uhf":
        eng.init_cc_uspinorb(n, c["na"], c["nb"], np.diag(c["fa"]).copy(), np.diag(c["fb"]).copy(), 8)
    else:
        eng.uso_init_fock(n, c["na"], c["nb"], c["fa"], c["fb"], 8)


def _close(x, ref, tol, what):
    err, bound = float(np.max(np.abs(x - ref))), tol * max(1.0, float(np.max(np.abs(ref))))
    print(what, "error", err, "bound", bound)
    assert err < bound, what


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_iteration_and_the_density_at_random_amplitudes(eng, name):
    """(l_new - l) D = G and the density at O(1) random t and l: a missing or mis-signed term shows at 1e-2 and upward"""
    c = _case(name)
    cc, o, v = c["cc"], c["o"], c["v"]
    rng = np.random.default_rng(7)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    l1, l2 = np_lambda.antisym_random(rng, o, v)
    _feed(eng, c)
    eng.so_set_amplitudes(t1, t2)
    eng.so_lambda_init(0)
    s1, s2 = eng.so_lambda()
    assert np.array_equal(s1, t1) and np.array_equal(s2, t2)          # the start: l = t
    eng.so_set_lambda(l1, l2)
    pe0, _, _ = eng.so_lambda_energy(1e-11, 1e-11)
    assert abs(pe0 - np_lambda.pseudo_energy(cc, l1, l2)) < 1e-11 * max(1.0, abs(pe0))
    pe, rms, _ = eng.so_lambda_iterate(1e-11, 1e-11)
    n1, n2 = eng.so_lambda()
    G1, G2 = np_lambda.lambda_residual(cc, t1, t2, l1, l2)
    _close((n1 - l1) * cc.D1, G1, 1e-11, "G1")
    _close((n2 - l2) * cc.D2, G2, 1e-11, "G2")
    assert abs(pe - np_lambda.pseudo_energy(cc, n1, n2)) < 1e-11 * max(1.0, abs(pe))
    assert abs(rms - np.sum((n2 - l2) ** 2)) < 1e-11 * max(1.0, rms)
    if o == 1:
        assert not np.any(n2)
    eng.so_set_lambda(l1, l2)
    _close(eng.so_density(), np_lambda.density(c["g"], c["f"], o, t1, t2, l1, l2), 1e-11, "density")
    a1, a2 = eng.so_amplitudes()
    assert np.array_equal(a1, t1) and np.array_equal(a2, t2)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_converged_lambda_density_and_untouched_amplitudes(eng, name):
    c = _case(name)
    cc, o, n, na, nb = c["cc"], c["o"], c["n"], c["na"], c["nb"]
    _feed(eng, c)
    nit, en, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    t1, t2 = eng.so_amplitudes()
    with_t = c["src"] != "fock"                                       # ((T) takes (semi)canonical orbitals only)
    e_t = eng.do_ccsd_t_spinorb() if with_t else None
    lit, pes, rms = density.so_lambda_solve(eng, 300, 1e-11, 1e-11)
    print(name, "CCSD iterations", nit, "Lambda iterations", lit)
    l1, l2 = eng.so_lambda()
    r1, r2 = np_lambda.lambda_solve(cc, t1, t2)
    _close(l1, r1, 1e-9, "l1")
    _close(l2, r2, 1e-9, "l2")
    d = eng.so_density()
    _close(d, np_lambda.density(c["g"], c["f"], o, t1, t2, r1, r2), 1e-10, "density")
    assert abs(np.trace(d[:o, :o]) + np.trace(d[o:, o:])) < 1e-12
    da, db = density.spatial_blocks(d, n, na, nb, c["src"] == "rhf")
    occ = density.natural_occupations(da, db, None if c["src"] == "rhf" else c["ub"] @ c["ua"].T)
    assert abs(np.sum(occ) - (na + nb)) < 1e-10 and np.all(np.diff(occ) <= 0.0)
    assert occ[0] < 2.0 + 1e-10 and occ[-1] > -1e-10
    if c["src"] == "rhf":
        assert np.max(np.abs(da - db)) < 1e-10                        # closed shell
    if name == "two_electron":                                         # CCSD is exact: the FCI density
        e_fci, ra, rb = np_lambda.fci_two_electron_density(c["h"], c["chem"])
        assert abs(np_rocc.e_ref_elec(c["h"], c["fa"], c["fb"], 1, 1) + en[nit] - e_fci) < 1e-9
        assert max(np.max(np.abs(da - ra)), np.max(np.abs(db - rb))) < 1e-8
    a1, a2 = eng.so_amplitudes()
    assert np.array_equal(a1, t1) and np.array_equal(a2, t2)          # bit for bit
    if with_t:
        assert eng.do_ccsd_t_spinorb() == e_t                         # the (T) plan and its operands survived Lambda


def test_errors_leave_the_engine_usable(eng):
    from afesp_amd.capi import Engine
    c = _case("rhf_fed")
    nn = (c["o"] + c["v"]) ** 2
    with Engine(0) as fresh:                                           # no state at all
        fresh.so_o, fresh.so_v = c["o"], c["v"]
        for call in (lambda: fresh.so_lambda_init(8), lambda: fresh.so_lambda_iterate(), lambda: fresh.so_lambda_energy(),
                     lambda: fresh.so_lambda_diis(), lambda: fresh.so_lambda(), lambda: fresh.so_density()):
            with pytest.raises(AfespError, match="status 1: .*no spin-orbital CCSD state"):
                call()
    _feed(eng, c, published=False)                                     # the reference's transposed F_mi term
    with pytest.raises(AfespError, match="status 20: .*F_mi"):
        eng.so_lambda_init(8)
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
        eng.so_lambda_iterate()
    _feed(eng, c)
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
        eng.so_density()
    with pytest.raises(AfespError, match="status 1: .*diis_n_errmat"):
        eng.so_lambda_init(16)
    eng.so_lambda_init(8)
    with pytest.raises(AfespError, match="status 22: .*needs"):
        eng.so_density(capacity=nn - 1)
    first = eng.so_lambda_iterate(1e-11, 1e-11)
    t1, t2 = eng.so_amplitudes()
    eng.so_set_amplitudes(t1, t2)                                      # may have changed t: stale, whatever was written
    for call in (lambda: eng.so_lambda_iterate(), lambda: eng.so_lambda_energy(), lambda: eng.so_lambda_diis(), lambda: eng.so_lambda(),
                 lambda: eng.so_set_lambda(t1, t2), lambda: eng.so_density()):
        with pytest.raises(AfespError, match="status 21: .*stale"):
            call()
    eng.so_lambda_init(8)                                              # ... and a new init serves again, with the same numbers
    assert eng.so_lambda_iterate(1e-11, 1e-11) == first
    eng.so_iterate(1e-11, 1e-11)                                       # a T iteration: stale again
    with pytest.raises(AfespError, match="status 21: .*stale"):
        eng.so_lambda_iterate()
