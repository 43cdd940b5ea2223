"""CPU checks of the Lambda equations and the one-particle density: the explicit term-by-term form the device code follows
(np_lambda.lambda_residual_explicit / density_explicit) against the defining complex-step form, stationarity, FCI for two electrons,
the Jacobi iteration, afesp_amd.density, and what the built library exports."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import np_lambda
import np_rocc
import np_ucc
from afesp_amd import capi, density, inputs

HOST_EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "a-fortran-electronic-structure-program_amd", "host",
                        "els_amd")


def _converged(n, na, nb, seed, canonical):
    g, f, o, blocks = np_lambda.model(n, na, nb, seed, canonical=canonical)
    cc = np_rocc.ROCC(g, f, o)
    cc.solve(200, 1e-13, 1e-13)
    t1, t2 = cc.t1.copy(), cc.t2.copy()
    jac = np_lambda.jacobian(cc, t1, t2)
    l1, l2 = np_lambda.lambda_solve(cc, t1, t2, jac)
    return dict(g=g, f=f, o=o, n=n, na=na, nb=nb, cc=cc, t1=t1, t2=t2, jac=jac, l1=l1, l2=l2, blocks=blocks)


@pytest.fixture(scope="module", params=["rohf_type", "uhf_type"])
def case(request):
    """the non-canonical ROHF-type model (n = 4, nalpha = 2, nbeta = 1: o = 3, v = 5) and one canonical UHF-type case"""
    if request.param == "rohf_type":
        c = _converged(4, 2, 1, 1, False)
        assert (c["o"], c["cc"].v) == (3, 5) and 0.05 < np.max(np.abs(c["cc"].f_ov)) < 0.2
    else:
        c = _converged(4, 2, 2, 5, True)
        assert not np.any(c["cc"].f_ov) and not np.any(c["cc"].f_oo)
    return c


def _close(x, ref, what):
    err, bound = np.max(np.abs(x - ref)), 1e-12 * max(1.0, np.max(np.abs(ref)))
    print(what, err, bound)
    assert err < bound, what


def _explicit_against_complex_step(g, f, cc, t1, t2, l1, l2, jac):
    G1, G2 = np_lambda.lambda_residual(cc, t1, t2, l1, l2, jac)
    X1, X2 = np_lambda.lambda_residual_explicit(cc, t1, t2, l1, l2)
    _close(X1, G1, "G1")
    _close(X2, G2, "G2")
    _close(np_lambda.density_explicit(cc, t1, t2, l1, l2), np_lambda.density(g, f, cc.o, t1, t2, l1, l2), "density")


def test_explicit_forms_equal_the_complex_step_forms(case):
    c, cc = case, case["cc"]
    rng = np.random.default_rng(11)
    o, v = cc.o, cc.v
    points = [(c["t1"], c["t2"], c["l1"], c["l2"], c["jac"]), (*np_lambda.antisym_random(rng, o, v), *np_lambda.antisym_random(rng, o, v), None)]
    for t1, t2, l1, l2, jac in points:
        _explicit_against_complex_step(c["g"], c["f"], cc, t1, t2, l1, l2, jac)
    # at the converged t and the solved l the residual itself vanishes
    G1, G2 = np_lambda.lambda_residual_explicit(cc, c["t1"], c["t2"], c["l1"], c["l2"])
    assert max(np.max(np.abs(G1)), np.max(np.abs(G2))) < 1e-12


def test_explicit_forms_equal_the_complex_step_forms_at_pairwise_distinct_extents():
    """The random-point comparison alone (nothing is converged) on the non-canonical model n = 6, nalpha = 3, nbeta = 2: o = 5, v = 7,
    npo = 10 and npv = 21 are pairwise distinct, so an einsum of the restatement with two extents transposed cannot even be evaluated,
    let alone agree.  245 unique amplitudes: 245 complex residuals for the Jacobian."""
    g, f, o, _ = np_lambda.model(6, 3, 2, 3, canonical=False)
    cc = np_rocc.ROCC(g, f, o)
    v = cc.v
    assert (o, v) == (5, 7) and len(np_lambda.pack(cc.t1, cc.t2)) == 245
    assert len({o, v, o * (o - 1) // 2, v * (v - 1) // 2}) == 4 and np.max(np.abs(cc.f_ov)) > 0.05
    rng = np.random.default_rng(12)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    l1, l2 = np_lambda.antisym_random(rng, o, v)
    _explicit_against_complex_step(g, f, cc, t1, t2, l1, l2, None)


@pytest.mark.parametrize("name,n,na,nb,canonical", [("fock_odd", 11, 5, 4, False), ("rhf_mid", 14, 5, 5, True)])
def test_float64_explicit_form_is_the_extended_precision_one_to_1e_13(name, n, na, nb, canonical):
    """The explicit form is the only reference of tests/test_gpu_lambda_mid.py (the complex step is infeasible at those extents), and
    the bound there is 1e-11 x max(1, max |ref|): here every tensor it supplies, evaluated in float64, stays within 1e-13 x max |ref| of
    the same formulas in np.longdouble (64-bit mantissa) at O(1) amplitudes -- two orders inside that bound.  Measured: 2.9e-15 (x1 at rhf_mid)."""
    assert np.finfo(np.longdouble).eps < 1e-18                     # (an extended type, not an alias of float64)
    g, f, o, _ = np_lambda.model(n, na, nb, 40 + n, canonical=canonical)
    ld = np.longdouble
    cc, cx = np_rocc.ROCC(g, f, o), np_rocc.ROCC(g.astype(ld), f.astype(ld), o)
    v = cc.v
    rng = np.random.default_rng(13)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    l1, l2 = np_lambda.antisym_random(rng, o, v)
    amps = (t1, t2, l1, l2)

    def everything(c, a):
        I = np_lambda.hbar(c, a[0], a[1])
        x1, x2 = np_lambda.lambda_rhs_explicit(c, *a, I)
        return dict(I, x1=x1, x2=x2, density=np_lambda.density_explicit(c, *a))
    got, ref = everything(cc, amps), everything(cx, tuple(x.astype(ld) for x in amps))
    assert ref["x2"].dtype == ld and ref["Hvvvo"].dtype == ld and ref["density"].dtype == ld
    worst = 0.0
    for k in sorted(ref):
        rel = float(np.max(np.abs(got[k] - ref[k])) / np.max(np.abs(ref[k])))
        print(name, k, "float64 against longdouble, relative", rel)
        worst = max(worst, rel)
        assert rel < 1e-13, k
    print(name, "worst", worst)


def test_density_is_the_derivative_of_the_converged_energy(case):
    """stationarity: D_pq = 1/2 dE_CCSD / d eps under f -> f + eps (e_pq + e_qp), one element of each block (same spin)"""
    c = case
    o, eps = c["o"], 1e-4
    d = np_lambda.density_explicit(c["cc"], c["t1"], c["t2"], c["l1"], c["l2"])
    va = o                                     # first alpha virtual
    for p, q in ((0, 1), (va, va + 1), (0, va), (1, 1)):
        x = np.zeros_like(c["f"])
        x[p, q] += eps
        x[q, p] += eps
        e = []
        for sign in (1.0, -1.0):
            cc = np_rocc.ROCC(c["g"], c["f"] + sign * x, o)
            cc.t1, cc.t2 = c["t1"].copy(), c["t2"].copy()
            e.append(cc.solve(200, 1e-13, 1e-13)[1])
        fd = 0.5 * (e[0] - e[1]) / (2.0 * eps)
        print((p, q), d[p, q], fd, abs(d[p, q] - fd))
        assert abs(d[p, q] - fd) < 1e-7, (p, q)


def test_trace_and_spin_blocks(case):
    c = case
    o = c["o"]
    d = np_lambda.density_explicit(c["cc"], c["t1"], c["t2"], c["l1"], c["l2"])
    assert abs(np.trace(d[:o, :o]) + np.trace(d[o:, o:])) < 1e-12
    _, spin = np_ucc.so_order(c["n"], c["na"], c["nb"])
    assert not np.any(d[spin[:, None] != spin[None, :]])
    assert np.array_equal(d, d.T)
    da, db = density.spatial_blocks(d, c["n"], c["na"], c["nb"], False)
    occ = density.natural_occupations(da, db)
    assert abs(np.trace(da) - c["na"]) < 1e-12 and abs(np.trace(db) - c["nb"]) < 1e-12
    assert abs(np.sum(occ) - (c["na"] + c["nb"])) < 1e-12 and np.all(np.diff(occ) <= 0.0)
    assert abs(density.expectation(da, db, np.eye(c["n"])) - (c["na"] + c["nb"])) < 1e-12
    # beta orbitals that differ from the alpha ones: the occupations are those of the common basis, whatever rotation describes beta
    r = np_rocc.random_orthogonal(np.random.default_rng(4), c["n"], 0.4)
    assert np.max(np.abs(density.natural_occupations(da, r @ db @ r.T, r) - occ)) < 1e-12
    if c["na"] != c["nb"]:
        assert np.max(np.abs(density.natural_occupations(da, r @ db @ r.T) - occ)) > 1e-6


def test_two_electron_density_is_the_fci_density():
    n = 3
    h, chem, fa, fb = np_lambda.two_electron_model(n, 21)
    cc = np_rocc.rocc_from_blocks(chem, chem, chem, fa, fb, 1, 1)
    assert np.max(np.abs(cc.f_ov)) > 1e-2
    _, e_cc = cc.solve(200, 1e-13, 1e-13)
    l1, l2 = np_lambda.lambda_solve(cc, cc.t1, cc.t2)
    d = np_lambda.density_explicit(cc, cc.t1, cc.t2, l1, l2)
    da, db = density.spatial_blocks(d, n, 1, 1, False)
    e_fci, ra, rb = np_lambda.fci_two_electron_density(h, chem)
    assert abs(np_rocc.e_ref_elec(h, fa, fb, 1, 1) + e_cc - e_fci) < 1e-10
    err = max(np.max(np.abs(da - ra)), np.max(np.abs(db - rb)))
    print("two-electron density against FCI", err)
    assert err < 1e-10


def test_jacobi_iteration_converges_to_the_solved_lambda(case):
    c = case
    l1, l2, it = np_lambda.jacobi(c["cc"], c["t1"], c["t2"], 200, 1e-10)
    print("Jacobi iterations", it)
    assert it < 100
    assert np.max(np.abs(l1 - c["l1"])) < 1e-8 and np.max(np.abs(l2 - c["l2"])) < 1e-8


def test_spatial_blocks_cover_both_spin_orbital_orders():
    rng = np.random.default_rng(2)
    n, na = 3, 2
    d = rng.standard_normal((2 * n, 2 * n))
    d = d + d.T
    da, db = density.spatial_blocks(d, n, na, na, True)          # interleaved: spin orbital 2 P + spin
    ref = d + np.diag((np.arange(2 * n) < 2 * na).astype(float))
    assert np.array_equal(da, ref[0::2, 0::2]) and np.array_equal(db, ref[1::2, 1::2])
    orb, spin = np_ucc.so_order(n, 2, 1)                         # block order
    da, db = density.spatial_blocks(d, n, 2, 1, False)
    ref = d + np.diag((np.arange(2 * n) < 3).astype(float))
    ia, ib = np.where(spin == 0)[0], np.where(spin == 1)[0]
    assert np.array_equal(da[np.ix_(orb[ia], orb[ia])], ref[np.ix_(ia, ia)])
    assert np.array_equal(db[np.ix_(orb[ib], orb[ib])], ref[np.ix_(ib, ib)])
    with pytest.raises(ValueError):
        density.spatial_blocks(d, n, 2, 1, True)


def test_library_exports_the_lambda_entry_points():
    names = ("afesp_ccsd_so_lambda_init", "afesp_ccsd_so_lambda_iterate", "afesp_ccsd_so_lambda_energy", "afesp_ccsd_so_lambda_diis",
             "afesp_ccsd_so_get_lambda", "afesp_ccsd_so_set_lambda", "afesp_ccsd_so_density")
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in names:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS
        assert getattr(capi.load_library(), s).argtypes is not None, s
    assert lib.afesp_version() >= 2
    for m in ("so_lambda_init", "so_lambda_iterate", "so_lambda_energy", "so_lambda_diis", "so_lambda", "so_set_lambda", "so_density"):
        assert callable(getattr(capi.Engine, m))
    assert lib.afesp_ccsd_so_lambda_init(None, 8) == 1           # a NULL context is an argument error, as everywhere
    for name in ("H_ov", "H_oo", "H_vv", "H_oooo", "H_vovv", "H_ooov", "H_ovvo", "H_vvvo", "H_ovoo", "lam_tau", "G_vv", "G_oo"):
        assert len(capi.Engine.SO_SHAPES[name]) in (2, 4), name  # (afesp_ccsd_so_get_tensor serves them from a live Lambda state)
    assert (capi.Engine.SO_SHAPES["H_vvvo"], capi.Engine.SO_SHAPES["H_ovoo"]) == ("ovvv", "ovoo")   # H_abei as (i,e,a,b), H_mbij as (m,b,i,j)


def test_cc_density_key_is_refused_on_the_types_that_run_no_spin_orbital_ccsd(tmp_path):
    def write(body):
        (tmp_path / "els.in").write_text("&elsinput\n" + body + "\n/\n")
        return str(tmp_path / "els.in")
    assert inputs.read_els_in(write('calc_type="UCCSD"')).cc_density is False
    for calc in inputs.CC_DENSITY_TYPES:
        assert inputs.read_els_in(write(f'calc_type="{calc}",\ncc_density=.true.')).cc_density is True
    bad = ("CCSD_spatial", "CCSD(T)_spatial", "CRCCSD(T)_spatial", "MP2_spinorb", "UMP2", "RHF")
    for calc in bad:
        with pytest.raises(ValueError, match="takes no cc_density"):
            inputs.read_els_in(write(f'calc_type="{calc}",\ncc_density=.true.'))
    with pytest.raises(ValueError):
        inputs.read_els_in(write('calc_type="UCCSD",\ncc_density=3'))
    with pytest.raises(ValueError, match="UHF FCIDUMP"):
        inputs.read_els_in(write('calc_type="UCCSD",\ncc_density=.true.,\nfcidump_in=.true.'))
    if not os.path.exists(HOST_EXE):
        pytest.skip("els_amd not built")
    res = subprocess.run([HOST_EXE], cwd=tmp_path, capture_output=True, text=True, timeout=120)      # (the input just written)
    assert res.returncode != 0 and "cc_density on a UHF FCIDUMP" in res.stderr, res.stderr
    for calc in bad + ("ROHF-MP2",):
        write(f'calc_type="{calc}",\ncc_density=.true.' + (",\nfcidump_in=.true." if calc.startswith("ROHF") else ""))
        res = subprocess.run([HOST_EXE], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert res.returncode != 0 and f"{calc} takes no cc_density" in res.stderr, (calc, res.stderr)
        assert "system::read_system_in" in res.stderr
