"""The left-hand side of EOM-IP-CCSD and EOM-EA-CCSD without a GPU: the explicit left sigma build and the four explicit Dyson forms of
tests/np_eom_ipea_left.py against their definitions, the adjoint identity against np_eom_ipea's right-hand build, two exactly solvable
models against FCI with both sum rules, the Koopmans limit, the biorthonormalisation inside degenerate clusters, the els.in key, and the
entry points the library, the Engine and the Fortran bindings export.

Tolerances: 1e-12 x max(1, max |ref|) between two numpy forms of the same quantity; 1e-9 against FCI (the bound tests/test_eom_left_cpu.py
uses: amplitudes converged to 1e-14, eigenvectors of a non-symmetric matrix)."""
import ctypes
import os
import re

import numpy as np
import pytest

import np_eom_ipea as X
import np_eom_ipea_left as XL
import np_lambda
import np_rocc
from afesp_amd import capi, eom, inputs

SECTORS = {"IP": X.IP, "EA": X.EA}
MODELS = [(5, 2, 2, 11), (5, 2, 1, 12), (4, 1, 1, 13), (6, 3, 2, 14)]         # (o, v) = (4,6) (3,7) (2,6) (5,7)


def _close(x, ref, tol, what):
    err, bound = float(np.max(np.abs(x - ref))) if np.size(ref) else 0.0, tol * max(1.0, float(np.max(np.abs(ref))) if np.size(ref) else 1.0)
    print(what, "error", err, "bound", bound)
    assert err < bound, what


_AMPS = {}


def _amplitudes(n, na, nb, seed, converged):
    """the model with random O(0.3) t and lambda, or with its converged t and lambda, made once"""
    key = (n, na, nb, seed, converged)
    if key not in _AMPS:
        g, f, o, _ = np_lambda.model(n, na, nb, seed)
        cc = np_rocc.ROCC(g, f, o)
        rng = np.random.default_rng(seed)
        if converged:
            cc.solve(300, 1e-13, 1e-13)
            t1, t2 = cc.t1.copy(), cc.t2.copy()
            lam1, lam2 = np_lambda.lambda_solve(cc, t1, t2)
        else:
            t1, t2 = np_lambda.antisym_random(rng, o, cc.v)
            lam1, lam2 = np_lambda.antisym_random(rng, o, cc.v)
        _AMPS[key] = (g, f, o, cc, t1, t2, lam1, lam2, np_lambda.hbar(cc, t1, t2))
    return _AMPS[key]


@pytest.mark.parametrize("sector", sorted(SECTORS))
@pytest.mark.parametrize("converged", [False, True])
@pytest.mark.parametrize("n,na,nb,seed", MODELS)
def test_explicit_left_sigma_and_dyson_forms_equal_their_definitions(n, na, nb, seed, converged, sector):
    sec = SECTORS[sector]
    g, f, o, cc, t1, t2, lam1, lam2, I = _amplitudes(n, na, nb, seed, converged)
    v = cc.v
    rng = np.random.default_rng(seed + 100)
    l, r = X.random_vector(rng, sec, o, v), X.random_vector(rng, sec, o, v)
    what = f"{sector} o{o}v{v} {'converged' if converged else 'random'}"
    e1, e2 = XL.lsigma_explicit(sec, cc, t1, t2, *l, I)
    d1, d2, leak = XL.lsigma_definition(sec, g, f, o, t1, t2, *l)
    assert leak == 0.0
    _close(e1, d1, 1e-12, what + " left sigma1")
    _close(e2, d2, 1e-12, what + " left sigma2")
    m1, m2 = XL.lsigma_matrix(sec, cc, t1, t2, *l)
    _close(e1, m1, 1e-12, what + " left sigma1 against matrix^T")
    _close(e2, m2, 1e-12, what + " left sigma2 against matrix^T")
    s1, s2 = X.sigma_explicit(sec, cc, t1, t2, *r, I)
    lhs, rhs = X.dot(*l, s1, s2), X.dot(e1, e2, *r)
    print(what, "adjoint", lhs, rhs)
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    gl, gr = XL.dyson_definition(sec, g, f, o, t1, t2, lam1, lam2, l, r)
    xl, xr = XL.dyson_explicit(sec, cc, t1, t2, lam1, lam2, l, r)
    _close(xl, gl, 1e-12, what + " left Dyson vector")
    _close(xr, gr, 1e-12, what + " right Dyson vector")
    assert XL.dyson_explicit(sec, cc, t1, t2, lam1, lam2, l, None)[1] is None and XL.dyson_explicit(sec, cc, t1, t2, lam1, lam2, None, r)[0] is None


def _two_electron():
    h, chem, fa, fb = np_lambda.two_electron_model(4, 21)
    cc = np_rocc.rocc_from_blocks(chem, chem, chem, fa, fb, 1, 1)
    cc.solve(300, 1e-14, 1e-14)
    t1, t2 = cc.t1.copy(), cc.t2.copy()
    return h, chem, cc, t1, t2, np_lambda.lambda_solve(cc, t1, t2, np_lambda.jacobian(cc, t1, t2))


def check_ip_two_electron_poles(h, chem, omega, pole, tol=1e-9):
    """every root of the IP sector of the two-electron model (tests/test_gpu_eom_ipea_left.py runs this on the device's numbers)"""
    ref_w, ref_p = XL.fci_ip_two_electrons(h, chem)
    got = XL.cluster_sums(omega, pole)
    print("IP clusters", got, "FCI", ref_w, ref_p, "sum", sum(pole))
    assert [c[2] for c in got] == [2] * len(ref_w)
    for (w, p, _), rw, rp in zip(got, ref_w, ref_p):
        assert abs(w - rw) < tol and abs(p - rp) < tol
    assert abs(sum(pole) - 2.0) < tol                                       # the two electrons of the ground state


def check_ea_one_electron_poles(eps, chem_e, omega, pole, tol=1e-9):
    """every root of the EA sector of the one-electron reference: singlets are single roots, a triplet's three components one cluster"""
    ref_w, ref_p, singlet = XL.fci_ea_one_electron(eps, chem_e)
    got = XL.cluster_sums(omega, pole)
    print("EA clusters", got, "sum", sum(pole))
    assert len(got) == len(ref_w)
    for (w, p, size), rw, rp, s in zip(got, ref_w, ref_p, singlet):
        assert abs(w - rw) < tol and size == (1 if s else 3)
        assert abs(p - (1.0 if s else 3.0) * rp) < tol                       # (a triplet's cluster sums to 3 x its Ms = 0 weight)
    assert abs(sum(pole) - (2 * len(eps) - 1)) < tol                        # the empty spin orbitals


def test_two_electron_ip_pole_strengths_are_fci():
    h, chem, cc, t1, t2, lam = _two_electron()
    w, L, R = XL.eigen_pairs(X.IP, cc, t1, t2)
    for k in range(len(w)):
        assert abs(X.dot(*L[k], *R[k]) - 1.0) < 1e-12
    pole = [XL.pole_strength(*XL.dyson_explicit(X.IP, cc, t1, t2, *lam, L[k], R[k])) for k in range(len(w))]
    check_ip_two_electron_poles(h, chem, w, pole)
    e0 = np_lambda.fci_two_electron_density(h, chem)[0]
    assert np.max(np.abs(np.sort(e0 + w) - np.repeat(np.linalg.eigvalsh(h), 2))) < 1e-9


def one_electron_case():
    h, chem, _, _ = np_lambda.two_electron_model(4, 21)
    eps, chem_e, fa, fb = XL.one_electron_reference(h, chem)
    cc = np_rocc.rocc_from_blocks(chem_e, chem_e, chem_e, fa, fb, 1, 0)
    return eps, chem_e, fa, fb, cc


def test_one_electron_ea_pole_strengths_are_fci():
    eps, chem_e, fa, fb, cc = one_electron_case()
    assert (cc.o, cc.v) == (1, 7) and np.max(np.abs(cc.f_ov)) < 1e-14        # t = 0 is the solution
    t1, t2 = np.zeros((1, 7)), np.zeros((1, 1, 7, 7))
    w, L, R = XL.eigen_pairs(X.EA, cc, t1, t2)
    assert len(w) == 28
    pole = [XL.pole_strength(*XL.dyson_explicit(X.EA, cc, t1, t2, t1, t2, L[k], R[k])) for k in range(len(w))]
    check_ea_one_electron_poles(eps, chem_e, w, pole)


@pytest.mark.parametrize("sector", sorted(SECTORS))
def test_koopmans_limit(sector):
    """t = 0, lambda = 0: gamma_L = l1 and gamma_R = r1 on their block, zero elsewhere, so a pure 1h / 1p root has pole strength 1"""
    sec = SECTORS[sector]
    g, f, o, _ = np_lambda.model(5, 2, 1, 12, canonical=True)
    cc = np_rocc.ROCC(g, f, o)
    v = cc.v
    z1, z2 = np.zeros((o, v)), np.zeros((o, o, v, v))
    rng = np.random.default_rng(3)
    l, r = X.random_vector(rng, sec, o, v), X.random_vector(rng, sec, o, v)
    gl, gr = XL.dyson_explicit(sec, cc, z1, z2, z1, z2, l, r)
    own = slice(0, o) if sec == X.IP else slice(o, o + v)
    other = slice(o, o + v) if sec == X.IP else slice(0, o)
    assert np.array_equal(gl[own], l[0]) and np.array_equal(gr[own], r[0]) and not np.any(gl[other]) and not np.any(gr[other])
    dl, dr = XL.dyson_definition(sec, g, f, o, z1, z2, z1, z2, l, r)
    _close(gl, dl, 1e-12, f"{sector} Koopmans left")
    _close(gr, dr, 1e-12, f"{sector} Koopmans right")
    e1, e2 = X.unit_vector(sec, o, v, (1,))
    assert XL.pole_strength(*XL.dyson_explicit(sec, cc, z1, z2, z1, z2, (e1, e2), (e1, e2))) == 1.0


def test_biorthonormalise_ipea_on_a_mixed_degenerate_cluster_and_its_refusal():
    rng = np.random.default_rng(5)
    o, v = 3, 4
    for sec in (X.IP, X.EA):
        R = [X.random_vector(rng, sec, o, v) for _ in range(4)]
        packed = np.array([X.pack(sec, *r) for r in R])                     # (packed, the metric is the plain dot product)
        dual = np.linalg.pinv(packed).T                                     # <dual_j, R_k> = delta_jk
        mix = rng.uniform(-1.0, 1.0, (2, 2)) + 2.0 * np.eye(2)              # roots 1, 2 degenerate: a doublet whose left vectors come out mixed
        Lp = np.vstack([1.7 * dual[:1], mix @ dual[1:3], -0.4 * dual[3:]])
        omega = np.array([0.3, 0.5, 0.5 + 2e-7, 0.9])
        unp = lambda x: X.unpack(sec, x, o, v)
        L = eom.biorthonormalise_ipea(omega, [unp(x) for x in Lp], R)
        S = np.array([[eom.dot_ipea(l, r) for r in R] for l in L])
        assert np.max(np.abs(S - np.eye(4))) < 1e-12
        assert abs(eom.dot_ipea(R[0], R[1]) - X.dot(*R[0], *R[1])) < 1e-15
        with pytest.raises(ValueError, match="singular"):                   # apart by more than the tolerance: 1 x 1 clusters, S_11 = 0
            bad = Lp.copy()
            bad[1] = dual[2]
            eom.biorthonormalise_ipea(np.array([0.3, 0.5, 0.6, 0.9]), [unp(x) for x in bad], R)
        with pytest.raises(ValueError, match="singular"):                   # a cluster whose left vectors span another space
            bad = Lp.copy()
            bad[2] = bad[1]
            eom.biorthonormalise_ipea(omega, [unp(x) for x in bad], R)
        with pytest.raises(ValueError, match="differ in length"):
            eom.biorthonormalise_ipea(omega[:3], L, R)
        # both members of a pair the library flagged complex carry one vector: one state, normalised once, for both roots
        twice = [R[0], R[1], R[1], R[3]]
        L = eom.biorthonormalise_ipea(omega, [unp(x) for x in np.vstack([1.7 * dual[:1], 0.6 * dual[1:2], 2.0 * dual[2:3], dual[3:]])], twice)
        assert all(abs(eom.dot_ipea(L[k], twice[k]) - 1.0) < 1e-12 for k in range(4))
        assert np.array_equal(L[1][0], L[2][0]) and np.array_equal(L[1][1], L[2][1])


def test_dyson_spin_parts_follow_the_spin_order():
    from afesp_amd.density import so_spin_order
    for n, na, nb, inter in ((4, 2, 2, True), (4, 3, 1, False)):
        orb, spin = so_spin_order(n, na, nb, inter)
        gam = np.arange(1.0, 2 * n + 1)
        a, b = eom.dyson_spin_parts(gam, n, na, nb, inter)
        for p in range(2 * n):
            assert (a if spin[p] == 0 else b)[orb[p]] == gam[p]
        assert np.sum(a) + np.sum(b) == np.sum(gam)
    with pytest.raises(ValueError, match="spin orbitals"):
        eom.dyson_spin_parts(np.zeros(5), 4, 2, 2, True)


def test_eom_ipea_left_key_needs_ip_or_ea_roots(tmp_path):
    def write(body):
        (tmp_path / "els.in").write_text("&elsinput\n" + body + "\n/\n")
        return str(tmp_path / "els.in")
    assert inputs.read_els_in(write('calc_type="UCCSD"')).eom_ipea_left is False
    for calc in inputs.CC_DENSITY_TYPES:
        for key in ("eom_ip_nroots", "eom_ea_nroots"):
            si = inputs.read_els_in(write(f'calc_type="{calc}",\n{key}=4,\neom_ipea_left=.true.'))
            assert si.eom_ipea_left is True and getattr(si, key) == 4
            assert inputs.read_els_in(write(f'calc_type="{calc}",\n{key}=4,\neom_ipea_left=.false.')).eom_ipea_left is False
        with pytest.raises(ValueError, match="eom_ipea_left needs eom_ip_nroots > 0 or eom_ea_nroots > 0"):
            inputs.read_els_in(write(f'calc_type="{calc}",\neom_ipea_left=.true.'))
        with pytest.raises(ValueError, match="eom_ipea_left needs"):        # the EE roots are not what it asks for
            inputs.read_els_in(write(f'calc_type="{calc}",\neom_nroots=3,\neom_ipea_left=.true.'))
    for calc in ("CCSD_spatial", "CCSD(T)_spatial", "MP2_spinorb", "UMP2", "RHF"):
        with pytest.raises(ValueError, match="takes no eom_ip_nroots"):
            inputs.read_els_in(write(f'calc_type="{calc}",\neom_ip_nroots=2,\neom_ipea_left=.true.'))
        with pytest.raises(ValueError, match="eom_ipea_left needs"):
            inputs.read_els_in(write(f'calc_type="{calc}",\neom_ipea_left=.true.'))
        assert inputs.read_els_in(write(f'calc_type="{calc}",\neom_ipea_left=.false.')).eom_ipea_left is False
    for bad in ("1", "2.5", '"yes"'):
        with pytest.raises(ValueError, match="invalid input file format"):
            inputs.read_els_in(write(f'calc_type="UCCSD",\neom_ip_nroots=2,\neom_ipea_left={bad}'))


NAMES = ("afesp_ccsd_so_eom_ipea_lsigma", "afesp_ccsd_so_eom_ipea_left_init", "afesp_ccsd_so_eom_ipea_left_guess",
         "afesp_ccsd_so_eom_ipea_left_set_guess", "afesp_ccsd_so_eom_ipea_left_iterate", "afesp_ccsd_so_eom_ipea_left_get_vector",
         "afesp_ccsd_so_eom_ipea_dyson")


def test_library_engine_and_fortran_bindings_export_the_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "afesp.h")).read()
    f90 = open(os.path.join(os.path.dirname(os.path.dirname(capi.__file__)), "host", "afesp_capi.f90")).read()
    public = f90[:f90.index("interface")]
    lib = ctypes.CDLL(capi.LIB_PATH)
    lib.afesp_version.restype = ctypes.c_int
    assert lib.afesp_version() >= 7
    for s in NAMES:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS and f"int {s}(afesp_ctx* ctx, int sector" in header
        assert getattr(capi.load_library(), s).argtypes is not None, s
        assert re.search(rf"\b{s}\b", public) and f"bind(C, name='{s}')" in f90, s
    for m in ("so_eom_ipea_lsigma", "so_eom_ipea_left_init", "so_eom_ipea_left_guess", "so_eom_ipea_left_set_guess", "so_eom_ipea_left_iterate",
              "so_eom_ipea_left_vector", "so_eom_ipea_dyson"):
        assert callable(getattr(capi.Engine, m))
    for fn in (eom.so_eom_ip_left_solve, eom.so_eom_ea_left_solve, eom.biorthonormalise_ipea, eom.so_eom_ipea_properties, eom.dyson_spin_parts):
        assert callable(fn)
    for sector in (1, 2, 3):                                                # a NULL context is an argument error, as everywhere
        assert lib.afesp_ccsd_so_eom_ipea_left_init(None, sector, 1, 2) == 1
        assert lib.afesp_ccsd_so_eom_ipea_left_guess(None, sector) == 1
        assert lib.afesp_ccsd_so_eom_ipea_lsigma(None, sector, 1, None, None, None, None) == 1
        assert lib.afesp_ccsd_so_eom_ipea_left_iterate(None, sector, ctypes.c_double(1e-8), None, None, None, None, None) == 1
        assert lib.afesp_ccsd_so_eom_ipea_dyson(None, sector, 1, None, None, None, None, None, None) == 1
