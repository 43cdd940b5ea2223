"""GPU parity of the two-particle density of spin-orbital CCSD (afesp_ccsd_so_density2_*, afesp_amd.density) against the defining
finite difference of np_density2 (gamma_fd: the Lagrangian of np_lambda differentiated in g, no hand-derived term).

Shapes: those of test_gpu_lambda.py -- the interleaved RHF-fed state (4,6), unequal spin blocks (4,6), every f_ov / f_oo / f_vv term (3,5),
one pair each way (2,2) and no occupied pair at all (1,5: K = 0 for the vvvv pair product, every oo-antisymmetric block empty or zero).

Tolerances: 1e-11 x max(1, max |ref|) for tensors and scalars at equal amplitudes, 1e-9 for separately converged amplitudes
(e_tol = t_tol = l_tol = 1e-11)."""
import numpy as np
import pytest

import np_density2
import np_lambda
import np_rocc
from afesp_amd import density
from afesp_amd.capi import AfespError
from test_gpu_lambda import SHAPES, _case, _close, _feed

pytestmark = pytest.mark.gpu

NAMES = ("oooo", "ooov", "oovv", "ovov", "ovvv", "vvvv")
_REF = {}


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _ref(name):
    """random O(0.3) t and lambda of a shape with the defining Gamma, the one-particle density and the Lagrangian: made once, left unchanged"""
    if name not in _REF:
        c = _case(name)
        o, v = c["o"], c["v"]
        rng = np.random.default_rng(7)
        t1, t2 = np_lambda.antisym_random(rng, o, v)
        l1, l2 = np_lambda.antisym_random(rng, o, v)
        fd = np_density2.gamma_fd(c["g"], c["f"], o, t1, t2, l1, l2)
        _REF[name] = dict(c=c, t=(t1, t2), l=(l1, l2), fd=fd, blocks=np_density2.blocks_of(fd, o),
                          D=np_lambda.density_explicit(c["cc"], t1, t2, l1, l2), L=np_lambda.lagrangian(c["cc"], t1, t2, l1, l2))
    return _REF[name]


def _set(eng, r):
    _feed(eng, r["c"])
    eng.so_set_amplitudes(*r["t"])
    eng.so_lambda_init(0)
    eng.so_set_lambda(*r["l"])


def _scalar(x, ref, tol, what):
    err, bound = abs(x - ref), tol * max(1.0, abs(ref))
    print(what, "value", x, "error", err, "bound", bound)
    assert err < bound, what


def _bitwise_symmetry(g, name):
    """antisymmetric in each like pair, symmetric under (pq)<->(rs), exactly zero on the diagonals"""
    if name in ("oooo", "vvvv", "oovv", "ooov"):
        assert np.array_equal(g, -g.transpose(1, 0, 2, 3)), name
        assert not np.any(g[np.arange(g.shape[0]), np.arange(g.shape[0])]), name
    if name in ("oooo", "vvvv", "oovv", "ovvv"):
        assert np.array_equal(g, -g.transpose(0, 1, 3, 2)), name
        assert not np.any(g[:, :, np.arange(g.shape[2]), np.arange(g.shape[2])]), name
    if name in ("oooo", "vvvv", "ovov"):
        assert np.array_equal(g, g.transpose(2, 3, 0, 1)), name


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_block_energy_and_expectation_at_random_amplitudes(eng, name):
    """a missing or mis-signed term shows at 1e-2 and upward"""
    r = _ref(name)
    c, o, v = r["c"], r["c"]["o"], r["c"]["v"]
    n = o + v
    _set(eng, r)
    eng.so_density2_build()
    got = {k: eng.so_density2_get(k) for k in NAMES}
    for k in NAMES:
        _close(got[k], r["blocks"][k], 1e-11, f"{name} {k}")
        _bitwise_symmetry(got[k], k)
    pairs = eng.so_density2_get("vvvv_pairs")
    assert np.array_equal(pairs, pairs.T)
    assert np.array_equal(np_density2.unpair(pairs, v), got["vvvv"])          # the dense expansion IS the expanded pair matrix
    _close(pairs, np_density2.pairs_of(r["blocks"]["vvvv"]), 1e-11, f"{name} vvvv_pairs")
    full = eng.so_density2_get("full")
    _close(full, r["fd"], 1e-11, f"{name} full")
    assert np.array_equal(full, np_density2.expand(got, o, v))
    if o == 1:
        assert not np.any(got["oooo"]) and not np.any(got["ooov"]) and not np.any(got["oovv"]) and not np.any(got["vvvv"])
    # ---- the energy walk
    e = eng.so_density2_energy()
    _scalar(e[0], float(np.sum(c["f"] * r["D"])), 1e-11, f"{name} sum f D")
    fam = np_density2.family_energies(r["blocks"], c["g"], o)
    for k, x, ref in zip(NAMES, e[1:7], fam):
        _scalar(x, ref, 1e-11, f"{name} 1/4 g Gamma over {k}")
    assert e[7] == ((((e[1] + e[2]) + e[3]) + e[4]) + e[5]) + e[6]
    _scalar(e[0] + e[7], r["L"], 1e-11, f"{name} density-side Lagrangian")
    # ---- the expectation walk
    rng = np.random.default_rng(5)
    A, B = rng.uniform(-1.0, 1.0, (n, n)), rng.uniform(-1.0, 1.0, (n, n))
    _scalar(eng.so_density2_expect(A, B), float(np.einsum("pqrs,pr,qs->", r["fd"], A, B, optimize=True)), 1e-11, f"{name} expect(A, B)")
    # A = B = 1: the trace of Gamma, which the partial-trace identity sum_q Gtot_pqrq = (N - 1) gamma_pr fixes through D alone
    d = eng.so_density()
    _scalar(eng.so_density2_expect(np.eye(n), np.eye(n)), 2.0 * np.trace(d[:o, :o]) - 2.0 * o * np.trace(d), 1e-11, f"{name} expect(1, 1)")
    gt = density.total_rdm2(d, full, o)
    _close(np.einsum("pqrq->pr", gt), (o - 1) * (d + np.diag((np.arange(n) < o).astype(float))), 1e-11, f"{name} partial trace")
    a1, a2 = eng.so_amplitudes()
    l1, l2 = eng.so_lambda()
    assert np.array_equal(a1, r["t"][0]) and np.array_equal(a2, r["t"][1]) and np.array_equal(l1, r["l"][0]) and np.array_equal(l2, r["l"][1])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_density_side_energy_of_the_converged_state(eng, name):
    """sum f D + 1/4 sum g Gamma at converged t and lambda is the CCSD correlation energy: one scalar that closes t, lambda, D and Gamma"""
    c = _case(name)
    n, na, nb, o = c["n"], c["na"], c["nb"], c["o"]
    _feed(eng, c)
    nit, en, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
    assert nit > 0
    density.so_lambda_solve(eng, 300, 1e-11, 1e-11)
    eng.so_density2_build()
    e, diff = density.energy_from_densities(eng)
    print(name, "E(CCSD)", en[nit], "density side", e[0] + e[7], "difference", diff, "families", e[1:7])
    assert abs(diff) < 1e-9 and abs(e[0] + e[7] - en[nit]) < 1e-9
    interleaved = c["src"] == "rhf"
    m = None if interleaved else c["ub"] @ c["ua"].T
    s2 = density.s_squared(eng, n, na, nb, interleaved, m)
    s2_ref = density.s_squared_reference(n, na, nb, interleaved, m)
    # the same number from the full (o+v)^4 array in numpy
    orb, spin = density.so_spin_order(n, na, nb, interleaved)
    gt = density.total_rdm2(eng.so_density(), eng.so_density2_get("full"), o)
    _scalar(s2, np_density2.s_squared(gt, orb, spin, na, nb, m), 1e-11, f"{name} <S^2>")
    print(name, "<S^2> reference determinant", s2_ref, "CCSD", s2)
    if interleaved or name == "two_electron":
        assert abs(s2) < 1e-8                                              # closed shell; two electrons: the exact singlet
    if name == "one_electron":
        assert abs(s2 - 0.75) < 1e-12 and abs(s2_ref - 0.75) < 1e-12       # one electron is a doublet whatever the orbitals
    if name == "two_electron":                                             # CCSD is exact: Gtot is the 2-RDM of the FCI vector
        h, chem = c["h"], c["chem"]
        Hm = (np.einsum("pr,qs->pqrs", h, np.eye(n)) + np.einsum("pr,qs->pqrs", np.eye(n), h) + chem.transpose(0, 2, 1, 3)).reshape(n * n, n * n)
        w, vec = np.linalg.eigh(Hm)
        cf = vec[:, 0].reshape(n, n)
        ia, ib = np.where(spin == 0)[0], np.where(spin == 1)[0]
        x = np.einsum("pq,rs->pqrs", cf, cf)[np.ix_(orb[ia], orb[ib], orb[ia], orb[ib])]
        ref = np.zeros((2 * n,) * 4)
        ref[np.ix_(ia, ib, ia, ib)], ref[np.ix_(ib, ia, ib, ia)] = x, x.transpose(1, 0, 3, 2)
        ref[np.ix_(ib, ia, ia, ib)], ref[np.ix_(ia, ib, ib, ia)] = -x.transpose(1, 0, 2, 3), -x.transpose(0, 1, 3, 2)
        _close(gt, ref, 1e-9, "two-electron 2-RDM against FCI")
        assert abs(np_rocc.e_ref_elec(h, c["fa"], c["fb"], 1, 1) + e[0] + e[7] - w[0]) < 1e-9


def test_calls_do_not_interfere_bit_for_bit(eng):
    """a second build repeats the first; t, lambda, the one-particle density, (T) and a Lambda iteration are the same bits with and without
    density2 calls before them"""
    r = _ref("uhf_fed")
    n = r["c"]["o"] + r["c"]["v"]

    def rest():
        out = [eng.so_density(), eng.do_ccsd_t_spinorb(), eng.so_lambda_t()]
        out += [eng.so_lambda_iterate(1e-11, 1e-11), *eng.so_lambda(), *eng.so_amplitudes()]
        return out
    _set(eng, r)
    plain = rest()
    _set(eng, r)
    eng.so_density2_build()
    first = {k: eng.so_density2_get(k) for k in NAMES + ("vvvv_pairs", "full")}
    e1, x1 = eng.so_density2_energy(), eng.so_density2_expect(np.eye(n), r["D"])
    eng.so_density2_build()
    for k, x in first.items():
        assert np.array_equal(eng.so_density2_get(k), x), k
    assert np.array_equal(eng.so_density2_energy(), e1) and eng.so_density2_expect(np.eye(n), r["D"]) == x1
    for a, b in zip(rest(), plain):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_every_status_and_the_release_of_the_build(eng):
    from afesp_amd.capi import Engine
    r = _ref("rhf_fed")
    c = r["c"]
    n = c["o"] + c["v"]
    one = np.eye(n)
    users = (lambda: eng.so_density2_get("oovv"), lambda: eng.so_density2_energy(), lambda: eng.so_density2_expect(one, one))
    with Engine(0) as fresh:                                           # no state at all
        fresh.so_o, fresh.so_v = c["o"], c["v"]
        for call in (fresh.so_density2_build, lambda: fresh.so_density2_get("oooo"), fresh.so_density2_energy,
                     lambda: fresh.so_density2_expect(one, one)):
            with pytest.raises(AfespError, match="status 1: .*no spin-orbital CCSD state"):
                call()
    _feed(eng, c, published=False)                                     # the reference's transposed F_mi term
    with pytest.raises(AfespError, match="status 20: .*F_mi"):
        eng.so_density2_build()
    _feed(eng, c)
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
        eng.so_density2_build()
    eng.so_lambda_init(0)
    for call in users:                                                 # a live Lambda state, no build yet
        with pytest.raises(AfespError, match="status 21: .*no two-particle density"):
            call()
    eng.so_density2_build()
    for k in NAMES + ("vvvv_pairs", "full"):
        size = int(np.prod(eng.so_density2_shape(k)))
        with pytest.raises(AfespError, match="status 22: .*needs"):
            eng.so_density2_get(k, capacity=size - 1)
    L = eng.L                                                          # an unknown name, NULL arguments
    buf = np.zeros(8)
    assert L.afesp_ccsd_so_density2_get(eng.h, b"vvoo", buf.ctypes.data, 8) == 1
    assert L.afesp_ccsd_so_density2_get(eng.h, None, buf.ctypes.data, 8) == 1
    assert L.afesp_ccsd_so_density2_get(eng.h, b"oooo", None, 1 << 40) == 1
    assert L.afesp_ccsd_so_density2_energy(eng.h, None) == 1
    assert L.afesp_ccsd_so_density2_expect(eng.h, None, buf.ctypes.data, buf.ctypes.data) == 1
    assert L.afesp_ccsd_so_density2_expect(eng.h, buf.ctypes.data, None, buf.ctypes.data) == 1
    assert L.afesp_ccsd_so_density2_expect(eng.h, one.ctypes.data, one.ctypes.data, None) == 1
    first = eng.so_density2_energy()                                   # ... and the build still serves
    l1, l2 = eng.so_lambda()
    eng.so_set_lambda(l1, l2)                                          # may have changed lambda: stale, whatever was written
    for call in users:
        with pytest.raises(AfespError, match="status 21: .*no two-particle density"):
            call()
    eng.so_density2_build()
    assert np.array_equal(eng.so_density2_energy(), first)
    eng.so_lambda_iterate(1e-11, 1e-11)                                # a Lambda iteration writes lambda
    with pytest.raises(AfespError, match="status 21: .*no two-particle density"):
        eng.so_density2_energy()
    eng.so_density2_build()
    t1, t2 = eng.so_amplitudes()
    eng.so_set_amplitudes(t1, t2)                                      # may have changed t: the Lambda state itself is stale
    for call in users + (eng.so_density2_build,):
        with pytest.raises(AfespError, match="status 21: .*stale"):
            call()
    # released with the Lambda state: by a new so_lambda_init, and by whatever frees the state (a new init of it)
    eng.so_lambda_init(0)
    eng.so_density2_build()
    eng.so_lambda_init(0)
    with pytest.raises(AfespError, match="status 21: .*no two-particle density"):
        eng.so_density2_get("oooo")
    eng.so_density2_build()
    _feed(eng, c)
    with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
        eng.so_density2_get("oooo")
    eng.so_lambda_init(0)
    eng.so_density2_build()
    assert np.array_equal(eng.so_density2_energy(), first)             # (l = t of the start amplitudes, as at `first`)
