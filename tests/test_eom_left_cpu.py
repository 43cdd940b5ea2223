"""CPU checks of the left-hand side of EOM-EE-CCSD (np_eom_left, afesp_amd.eom): the explicit left sigma build the device code follows
against A^T from the complex-step Jacobian, the explicit bilinear density against the central difference in f, its special cases and
identities, FCI densities and transition moments for two electrons through the Python drivers, biorthonormalise, the eom_left input
key, and what the built library exports.

Tolerances: 1e-12 x max(1, max |ref|) between two numpy forms; 1e-9 against FCI at amplitudes converged to 1e-14."""
import ctypes

import numpy as np
import pytest

import np_eom
import np_eom_left
import np_lambda
import np_rocc
from afesp_amd import capi, density, eom, inputs


def _close(x, ref, tol, what):
    err, bound = float(np.max(np.abs(x - ref))), tol * max(1.0, float(np.max(np.abs(ref))))
    print(what, "error", err, "bound", bound)
    assert err < bound, what


@pytest.mark.parametrize("n,na,nb,seed", [(5, 2, 2, 31), (5, 2, 1, 32), (4, 1, 1, 33), (6, 3, 2, 34)])
def test_explicit_left_sigma_equals_the_transposed_jacobian(n, na, nb, seed):
    """(o,v) = (4,6), (3,7), (2,6), (5,7); at random O(0.3) t and at the converged t"""
    g, f, o, _ = np_lambda.model(n, na, nb, seed)
    cc = np_rocc.ROCC(g, f, o)
    v = cc.v
    assert (o, v) in ((4, 6), (3, 7), (2, 6), (5, 7))
    rng = np.random.default_rng(seed)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    cc.solve(300, 1e-13, 1e-13)
    for a1, a2, where in ((t1, t2, "random t"), (cc.t1.copy(), cc.t2.copy(), "converged t")):
        l1, l2 = np_lambda.antisym_random(rng, o, v)
        d1, d2 = np_eom_left.lsigma_definition(cc, a1, a2, l1, l2)
        e1, e2 = np_eom_left.lsigma_explicit(cc, a1, a2, l1, l2)
        _close(e1, d1, 1e-12, f"left sigma1 {where}")
        _close(e2, d2, 1e-12, f"left sigma2 {where}")
        assert max(np.max(np.abs(e2 + e2.transpose(1, 0, 2, 3))), np.max(np.abs(e2 + e2.transpose(0, 1, 3, 2)))) < 1e-13
        r1, r2 = np_lambda.antisym_random(rng, o, v)                        # ... and it is the adjoint of the right-hand build
        s1, s2 = np_eom.sigma_explicit(cc, a1, a2, r1, r2)
        lhs, rhs = np_eom.dot(l1, l2, s1, s2), np_eom.dot(e1, e2, r1, r2)
        assert abs(lhs - rhs) < 1e-12 * max(1.0, abs(lhs))


def _argument_pairs(rng, o, v):
    """random (l0, l, r0, r), then the four cases above the library (with random vectors in the places of lambda, L_k, R_k)"""
    l, r = np_lambda.antisym_random(rng, o, v), np_lambda.antisym_random(rng, o, v)
    return {"random": (0.7, l, -0.4, r), "ground state": (1.0, l, 1.0, None), "excited state": (0.0, l, 0.3, r),
            "gamma 0k": (1.0, l, 0.3, r), "gamma k0": (0.0, l, 1.0, None), "no left vector": (1.3, None, 0.6, r)}


@pytest.mark.parametrize("n,na,nb,seed", [(4, 2, 1, 51), (6, 3, 2, 52)])
def test_explicit_density_equals_the_central_difference_in_f(n, na, nb, seed):
    """(o,v) = (3,5) and (5,7), both with every f term (f_ov and off-diagonal f_oo / f_vv)"""
    g, f, o, _ = np_lambda.model(n, na, nb, seed)
    cc = np_rocc.ROCC(g, f, o)
    v = cc.v
    assert (o, v) in ((3, 5), (5, 7))
    rng = np.random.default_rng(seed)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    for what, (l0, l, r0, r) in _argument_pairs(rng, o, v).items():
        ref = np_eom_left.density_definition(g, f, o, t1, t2, l0, l, r0, r)
        d = np_eom_left.density_explicit(cc, t1, t2, l0, l, r0, r)
        _close(d, ref, 1e-12, f"density, {what}")
        assert np.array_equal(d, d.T) and abs(np.trace(d)) < 1e-12          # no particle is made: the trace is zero for every pair
        if what == "ground state":
            assert np.max(np.abs(d - np_lambda.density_explicit(cc, t1, t2, *l))) < 1e-14


def test_reference_coupling_is_the_derivative_of_the_energy():
    g, f, o, _ = np_lambda.model(4, 2, 1, 53)
    cc = np_rocc.ROCC(g, f, o)
    rng = np.random.default_rng(53)
    t1, t2 = np_lambda.antisym_random(rng, o, cc.v)
    r1, r2 = np_lambda.antisym_random(rng, o, cc.v)
    e = np_lambda.residual(cc, t1 + 1j * np_lambda.H * r1, t2 + 1j * np_lambda.H * r2)[0]
    c = np_eom_left.ref_coupling(cc, t1, t2, r1, r2)
    assert abs(c - e.imag / np_lambda.H) < 1e-12 * max(1.0, abs(c))


_TWO = {}


def two_electron_case(n=4, seed=21, nmin=6):
    """The two-electron model at its converged amplitudes with lambda, the lowest roots of A by the reference Davidson (right, then left
    with the right vectors as guess; the number of roots ends on a whole multiplet) and the FCI states, made once."""
    if not _TWO:
        h, chem, fa, fb = np_lambda.two_electron_model(n, seed)
        cc = np_rocc.rocc_from_blocks(chem, chem, chem, fa, fb, 1, 1)
        cc.solve(300, 1e-14, 1e-14)
        t1, t2 = cc.t1.copy(), cc.t2.copy()
        o, v = cc.o, cc.v
        jac = np_lambda.jacobian(cc, t1, t2)
        lam = np_lambda.lambda_solve(cc, t1, t2, jac)
        w, c = np_eom_left.fci_two_electron_states(h, chem)
        nroots = 0
        for ck in c[1:]:                                                     # a triplet appears threefold among the roots of A
            nroots += 1 if np_eom_left.fci_is_singlet(ck) else 3
            if nroots >= nmin:
                break
        I = np_lambda.hbar(cc, t1, t2)
        guesses = [np_eom.unit_vector(o, v, k) for k in np_eom.guess_order(cc)[:nroots]]
        wr, X, _ = np_eom.davidson(lambda a, b: np_eom.sigma_explicit(cc, t1, t2, a, b, I), cc.D1, cc.D2, guesses, nroots, tol=1e-10)
        R = [np_lambda.unpack(x, o, v) for x in X]
        wl, Y, _ = np_eom.davidson(lambda a, b: np_eom_left.lsigma_explicit(cc, t1, t2, a, b, I), cc.D1, cc.D2, R, nroots, tol=1e-10)
        L = [np_lambda.unpack(y, o, v) for y in Y]
        _TWO.update(n=n, h=h, chem=chem, fa=fa, fb=fb, cc=cc, t1=t1, t2=t2, o=o, v=v, A=jac[1], lam=lam, fci_w=w, fci_c=c, nroots=nroots,
                    omega=wr, omega_left=wl, R=R, L=L)
    return _TWO


def check_two_electron_properties(c, omega, props, tol=1e-9):
    """props[k]: dict(density, g0k, gk0) of root k.  Singlets: the excited-state density and the transition-moment products of three random
    symmetric spin-free operators against FCI; every component of a triplet: product 0.  (tests/test_gpu_eom_left.py runs this on the
    device's numbers)"""
    n = c["n"]
    orb, spin = density.so_spin_order(n, 1, 1, False)
    exc = c["fci_w"] - c["fci_w"][0]
    rng = np.random.default_rng(77)
    ops = [(lambda m: m + m.T)(rng.uniform(-1.0, 1.0, (n, n))) for _ in range(3)]
    nsinglet = 0
    for k, w in enumerate(omega):
        j = int(np.argmin(np.abs(exc - w)))
        assert j > 0 and abs(exc[j] - w) < tol
        ck, singlet = c["fci_c"][j], np_eom_left.fci_is_singlet(c["fci_c"][j])
        if singlet:
            nsinglet += 1
            da, db = density.spatial_blocks(props[k]["density"], n, 1, 1, False)
            ra, rb = np_eom_left.fci_density(ck)
            err = max(np.max(np.abs(da - ra)), np.max(np.abs(db - rb)))
            print("root", k, "singlet, excited-state density error", err)
            assert err < tol
        ta, tb = np_eom_left.fci_density(c["fci_c"][0], ck)
        for m in ops:
            mu = np_eom_left.so_matrix(m, m, orb, spin)
            got = float(np.sum(mu * props[k]["g0k"])) * float(np.sum(mu * props[k]["gk0"]))
            ref = float(np.sum(m * (ta + tb))) ** 2 if singlet else 0.0
            print("root", k, "singlet" if singlet else "triplet", "moment product", got, "FCI", ref)
            assert abs(got - ref) < tol
    assert 0 < nsinglet < len(omega)                                         # both kinds were met


def test_two_electron_left_roots_densities_and_transition_moments_are_fci():
    c = two_electron_case()
    cc, t1, t2, omega = c["cc"], c["t1"], c["t2"], c["omega"]
    ref = np.sort(np.linalg.eigvals(c["A"]).real)[:c["nroots"]]
    print("omega right", omega, "left", c["omega_left"], "eig(A)", ref)
    assert np.max(np.abs(c["omega_left"] - ref)) < 1e-9 and np.max(np.abs(c["omega_left"] - omega)) < 1e-9
    assert 3 in [len(x) for x in eom.clusters(omega)]                        # the triplet's three components are one cluster
    L = eom.biorthonormalise(omega, c["L"], c["R"])
    S = np.array([[eom.dot(l, r) for r in c["R"]] for l in L])
    assert np.max(np.abs(S - np.eye(len(L)))) < 1e-9                         # (off the clusters: eigenvectors of different roots)
    props = []
    for k, w in enumerate(omega):
        r0 = np_eom_left.ref_coupling(cc, t1, t2, *c["R"][k]) / w
        assert abs(r0 + eom.dot(c["lam"], c["R"][k])) < 1e-9                 # <0| (1 + Lambda) (r0 + R_k) |0> = 0
        props.append(dict(density=np_eom_left.density_explicit(cc, t1, t2, 0.0, L[k], r0, c["R"][k]),
                          g0k=np_eom_left.density_explicit(cc, t1, t2, 1.0, c["lam"], r0, c["R"][k]),
                          gk0=np_eom_left.density_explicit(cc, t1, t2, 0.0, L[k], 1.0, None)))
    check_two_electron_properties(c, omega, props)
    n = c["n"]
    orb, spin = density.so_spin_order(n, 1, 1, False)
    m = np.diag(np.arange(n, dtype=float))
    dip = [np_eom_left.so_matrix(x, x, orb, spin) for x in (m, 0.0 * m, 0.0 * m)]
    f = eom.oscillator_strengths(omega, [p["g0k"] for p in props], [p["gk0"] for p in props], dip)
    for k, w in enumerate(omega):
        assert abs(f[k] - 2.0 / 3.0 * w * np.sum(dip[0] * props[k]["g0k"]) * np.sum(dip[0] * props[k]["gk0"])) < 1e-14
    with pytest.raises(ValueError, match="three symmetric"):
        eom.oscillator_strengths(omega, [p["g0k"] for p in props], [p["gk0"] for p in props], dip[:2])


def test_biorthonormalise_on_a_degenerate_cluster_and_its_refusal():
    rng = np.random.default_rng(5)
    o, v = 2, 3
    R = [np_lambda.antisym_random(rng, o, v) for _ in range(4)]
    flat = np.array([np.concatenate([r[0].ravel(), 0.5 * r[1].ravel()]) for r in R])       # (weights 1, 1/4 as a plain dot)
    dual = np.linalg.pinv(flat).T                                            # <dual_j, R_k> = delta_jk
    unflat = lambda x: (x[:o * v].reshape(o, v), 2.0 * x[o * v:].reshape(o, o, v, v))
    mix = rng.uniform(-1.0, 1.0, (3, 3)) + 2.0 * np.eye(3)                  # roots 1..3 degenerate: their left vectors come out mixed
    Lflat = np.vstack([1.7 * dual[:1], mix @ dual[1:]])
    omega = np.array([0.3, 0.5, 0.5 + 2e-7, 0.5 - 3e-7])
    assert sorted(map(sorted, eom.clusters(omega))) == [[0], [1, 2, 3]]
    L = eom.biorthonormalise(omega, [unflat(x) for x in Lflat], R)
    S = np.array([[eom.dot(l, r) for r in R] for l in L])
    assert np.max(np.abs(S - np.eye(4))) < 1e-12
    with pytest.raises(ValueError, match="singular"):                       # apart by more than the tolerance: 1 x 1 clusters, S_22 = 0 ...
        bad = Lflat.copy()
        bad[2] = dual[3]
        eom.biorthonormalise(np.array([0.3, 0.5, 0.6, 0.7]), [unflat(x) for x in bad], R)
    with pytest.raises(ValueError, match="singular"):                       # ... and a cluster whose left vectors span another space
        bad = Lflat.copy()
        bad[3] = bad[2]
        eom.biorthonormalise(omega, [unflat(x) for x in bad], R)
    with pytest.raises(ValueError, match="differ in length"):
        eom.biorthonormalise(omega[:3], L, R)


def test_eom_left_key_needs_eom_nroots(tmp_path):
    def write(body):
        (tmp_path / "els.in").write_text("&elsinput\n" + body + "\n/\n")
        return str(tmp_path / "els.in")
    assert inputs.read_els_in(write('calc_type="UCCSD"')).eom_left is False
    for calc in inputs.CC_DENSITY_TYPES:
        si = inputs.read_els_in(write(f'calc_type="{calc}",\neom_nroots=4,\neom_left=.true.'))
        assert si.eom_left is True and si.eom_nroots == 4
        assert inputs.read_els_in(write(f'calc_type="{calc}",\neom_nroots=4,\neom_left=.false.')).eom_left is False
        with pytest.raises(ValueError, match="eom_left needs eom_nroots"):
            inputs.read_els_in(write(f'calc_type="{calc}",\neom_left=.true.'))
    for calc in ("CCSD_spatial", "CCSD(T)_spatial", "MP2_spinorb", "UMP2", "RHF"):
        with pytest.raises(ValueError, match="takes no eom_nroots"):
            inputs.read_els_in(write(f'calc_type="{calc}",\neom_nroots=2,\neom_left=.true.'))
        with pytest.raises(ValueError, match="eom_left needs eom_nroots"):
            inputs.read_els_in(write(f'calc_type="{calc}",\neom_left=.true.'))
        assert inputs.read_els_in(write(f'calc_type="{calc}",\neom_left=.false.')).eom_left is False
    for bad in ("1", "2.5", '"yes"'):
        with pytest.raises(ValueError, match="invalid input file format"):
            inputs.read_els_in(write(f'calc_type="UCCSD",\neom_nroots=2,\neom_left={bad}'))


def test_library_exports_the_left_hand_entry_points():
    names = ("afesp_ccsd_so_eom_lsigma", "afesp_ccsd_so_eom_left_init", "afesp_ccsd_so_eom_left_guess", "afesp_ccsd_so_eom_left_set_guess",
             "afesp_ccsd_so_eom_left_iterate", "afesp_ccsd_so_eom_left_get_vector", "afesp_ccsd_so_eom_ref_coupling",
             "afesp_ccsd_so_eom_density")
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afesp.h")).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in names:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS and f"int {s}(afesp_ctx* ctx" in header
        assert getattr(capi.load_library(), s).argtypes is not None, s
    for m in ("so_eom_lsigma", "so_eom_left_init", "so_eom_left_guess", "so_eom_left_set_guess", "so_eom_left_iterate", "so_eom_left_vector",
              "so_eom_ref_coupling", "so_eom_density"):
        assert callable(getattr(capi.Engine, m))
    for fn in (eom.so_eom_left_solve, eom.biorthonormalise, eom.so_eom_properties, eom.oscillator_strengths):
        assert callable(fn)
    assert lib.afesp_ccsd_so_eom_left_init(None, 1, 2) == 1                 # a NULL context is an argument error, as everywhere
    assert lib.afesp_ccsd_so_eom_left_guess(None) == 1
    assert lib.afesp_ccsd_so_eom_lsigma(None, 1, None, None, None, None) == 1
    assert lib.afesp_ccsd_so_eom_left_iterate(None, ctypes.c_double(1e-8), None, None, None, None, None) == 1
    assert lib.afesp_ccsd_so_eom_ref_coupling(None, 1, None, None, None) == 1
    assert lib.afesp_ccsd_so_eom_density(None, ctypes.c_double(1.0), None, None, ctypes.c_double(1.0), None, None, None, ctypes.c_int64(0)) == 1
