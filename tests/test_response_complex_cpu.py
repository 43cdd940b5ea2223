"""CPU checks of the complex-frequency response reference (np_response_complex) that the GPU tests lean on, of the host-side pieces of
afesp_amd.response (the signed list, the Casimir-Polder grid, C6, the cross-section) and of what the built library exports.

Tolerances: 10 tol |R| for the restated solver against dense complex solves (|error| <= |rho| / sigma_min(A - z), and sigma_min is
above 0.1 on these models at these z); 1e-9 against FCI at amplitudes converged to 1e-14, the bound test_response_cpu holds; 1e-6 relative
for the C6 quadrature against its closed form (the accuracy the default grid is chosen for: it is the smallest that meets it)."""
import ctypes
import os

import numpy as np
import pytest

import np_eom
import np_lambda
import np_response
import np_response_complex as npc
from afesp_amd import capi, inputs, response
from test_eom_left_cpu import two_electron_case
from test_response_cpu import converged, random_symmetric, two_electron_operators


def _setup(n, na, nb, seed):
    c = converged(n, na, nb, seed)
    cc, t1, t2 = c["cc"], c["t1"], c["t2"]
    I = np_lambda.hbar(cc, t1, t2)
    sigma = lambda a, b: np_eom.sigma_explicit(cc, t1, t2, a, b, I)
    rng = np.random.default_rng(seed)
    ops = [random_symmetric(rng, c["o"] + c["v"]) for _ in range(3)]
    xis = [np_response.xi_explicit(t1, t2, X) for X in ops]
    w1 = float(np.min(np.linalg.eigvals(c["A"]).real))
    return c, sigma, ops, xis, w1


@pytest.mark.parametrize("n,na,nb,seed", [(5, 2, 2, 72), (6, 3, 2, 74)])
def test_restated_complex_solver_against_dense_complex_solves(n, na, nb, seed):
    c, sigma, ops, xis, w1 = _setup(n, na, nb, seed)
    cc, A, o, v = c["cc"], c["A"], c["o"], c["v"]
    zs = [0.3j, 0.5 * w1 + 0.02j, -0.5 * w1 - 0.02j, w1 + 0.05j, -w1 - 0.05j]
    rhs, shifts = [xi for _ in zs for xi in xis], [z for z in zs for _ in xis]
    tol = 1e-8
    for max_space in (None, 4 * len(rhs)):                                   # the second: as small as the unit takes, so it collapses
        x, info = npc.linear_davidson_complex(sigma, cc.D1, cc.D2, rhs, shifts, tol=tol, max_space=max_space, maxiter=300)
        print((o, v), "max_space", max_space, {k: info[k] for k in ("iterations", "nsigma", "collapses", "dropped")})
        assert np.all(info["resnorm"] < tol)
        if max_space is not None:
            assert info["collapses"] > 0
        for j in range(len(rhs)):
            ref = npc.solve_dense(A, o, v, rhs[j], shifts[j])
            ref = np_lambda.pack(ref[0].real, ref[1].real) + 1j * np_lambda.pack(ref[0].imag, ref[1].imag)
            err, bound = np.linalg.norm(x[j] - ref), 10.0 * tol * np.linalg.norm(ref)
            assert err < bound, (j, err, bound)
            assert np.linalg.norm(x[j].imag) > 1e-3 * np.linalg.norm(x[j].real)   # (a solution with both parts)


def test_complex_solver_at_gamma_zero_is_the_real_solver():
    """no imaginary vector survives the orthonormalisation: the sigma builds of the real solver, step for step, and its solutions"""
    c, sigma, ops, xis, w1 = _setup(5, 2, 2, 72)
    cc = c["cc"]
    rhs, omegas = xis + xis, [0.5 * w1] * 3 + [-0.5 * w1] * 3
    tol = 1e-8
    n = len(np_lambda.pack(cc.D1, cc.D2))
    xr, ri = np_response.linear_davidson(sigma, cc.D1, cc.D2, rhs, omegas, tol=tol, max_space=n)          # (no collapse: the counts of
    xc, ci = npc.linear_davidson_complex(sigma, cc.D1, cc.D2, rhs, omegas, tol=tol, max_space=2 * n)      #  pending vectors differ)
    print("real", ri["iterations"], ri["nsigma"], "complex", ci["iterations"], ci["nsigma"], "dropped", ci["dropped"])
    assert ri["collapses"] == ci["collapses"] == 0
    assert (ci["iterations"], ci["nsigma"]) == (ri["iterations"], ri["nsigma"])
    assert ci["dropped"] >= ci["nsigma"]                                       # the imaginary partner of every vector that was kept
    for a, b in zip(xr, xc):
        assert np.all(b.imag == 0.0)
        assert np.linalg.norm(a - b.real) < 10.0 * tol


def _two_electron_points(c):
    w1 = float(np.min(np.linalg.eigvals(c["A"]).real))
    return w1, [0.3j, w1 + 0.05j, 0.5 * w1 + 0.01j]


def test_two_electron_complex_response_is_fci():
    c = two_electron_case()
    cc, t1, t2, lam, A = c["cc"], c["t1"], c["t2"], c["lam"], c["A"]
    ms, ops = two_electron_operators(c)
    w1, zs = _two_electron_points(c)
    for z in zs:
        got = npc.response_dense(cc, t1, t2, lam, A, ops, z)
        ref = np.array([[npc.fci_response(c["fci_w"], c["fci_c"], x, y, z) for y in ms] for x in ms])
        print("z", z, "alpha", -got, "FCI", -ref)
        assert np.max(np.abs(got - ref)) < 1e-9
    # the real axis is the function of np_response
    real = npc.response_dense(cc, t1, t2, lam, A, ops, 0.5 * w1)
    assert np.max(np.abs(real.imag)) == 0.0
    assert np.max(np.abs(real.real - np_response.response_dense(cc, t1, t2, lam, A, ops, 0.5 * w1))) < 1e-12
    assert abs(npc.fci_response(c["fci_w"], c["fci_c"], ms[0], ms[1], 0.1) - np_response.fci_response(c["fci_w"], c["fci_c"], ms[0], ms[1], 0.1)) < 1e-14


def test_identities():
    c = converged(5, 2, 2, 72)
    cc, t1, t2, lam, A = c["cc"], c["t1"], c["t2"], c["lam"], c["A"]
    rng = np.random.default_rng(7)
    ops = [random_symmetric(rng, c["o"] + c["v"]) for _ in range(2)]
    z = 0.21 + 0.04j
    f, fbar, fminus = (npc.response_dense(cc, t1, t2, lam, A, ops, x) for x in (z, z.conjugate(), -z))
    scale = float(np.max(np.abs(f)))
    assert np.max(np.abs(fbar - f.conj())) < 1e-12 * scale                  # alpha(conj z) = conj alpha(z)
    assert np.max(np.abs(f - fminus.T)) < 1e-12 * scale                     # <<X;Y>>_z = <<Y;X>>_-z
    assert abs(f[0, 1] - f[1, 0]) > 1e-8                                    # (and not symmetric in X, Y)
    # alpha_XX(i gamma) is real, exactly: R(-z) = conj R(z) for an imaginary z, taken as the conjugate of the one solve
    o, v = c["o"], c["v"]
    xis = [np_response.xi_explicit(t1, t2, X) for X in ops]
    Rp = [npc.solve_dense(A, o, v, xi, 0.3j) for xi in xis]
    Rm = [(r[0].conj(), r[1].conj()) for r in Rp]
    g = npc.response_from_vectors(cc, t1, t2, lam, ops, Rp, Rm)
    assert g[0, 0].imag == 0.0 and g[1, 1].imag == 0.0 and abs(g[0, 0].real) > 1e-3
    assert np.max(np.abs(g - npc.response_dense(cc, t1, t2, lam, A, ops, 0.3j))) < 1e-12 * scale


def test_c6_quadrature_meets_the_closed_form_with_the_default_grid():
    c = two_electron_case()
    rng = np.random.default_rng(83)
    ms = [random_symmetric(rng, c["n"]) for _ in range(3)]
    gaps, f = npc.fci_strengths(c["fci_w"], c["fci_c"], ms)
    exact = npc.c6_closed_form(gaps, f)
    alpha = lambda u: np.array([np.sum(f / (gaps ** 2 + x ** 2)) for x in u])
    # alpha-bar(iu) of the strengths is the mean of the FCI response function at iu
    iso = -np.mean([npc.fci_response(c["fci_w"], c["fci_c"], m, m, 0.7j) for m in ms])
    assert abs(iso - alpha([0.7])[0]) < 1e-13 * abs(iso) and abs(iso.imag) == 0.0
    errs = {}
    for n in range(2, response.C6_NPTS + 1):
        u, w = response.casimir_polder_grid(n)
        errs[n] = abs(response.c6_coefficient(alpha(u), alpha(u), w) / exact - 1.0)
    print("C6", exact, "relative error by number of points", errs)
    assert errs[response.C6_NPTS] < 1e-6
    assert all(errs[n] >= 1e-6 for n in range(2, response.C6_NPTS))          # the default is the smallest that meets it
    u, w = response.casimir_polder_grid()
    assert len(u) == response.C6_NPTS and np.all(u > 0.0) and np.all(w > 0.0) and np.all(np.diff(u) > 0.0)
    assert abs(np.sum(w / (1.0 + u * u)) - 0.5 * np.pi) < 1e-6               # int_0^inf du / (1 + u^2)


def test_host_side_pieces():
    assert response.signed_complex_frequencies([0.3j, 0.1 + 0.02j, 0.3j, -0.1 - 0.02j]) == [0.3j, 0.1 + 0.02j, -0.1 - 0.02j]
    assert response.signed_complex_frequencies([0.0]) == [0.0j] and response.signed_complex_frequencies([0.2]) == [0.2 + 0j, -0.2 + 0j]
    w = np.array([0.1, 0.2])
    a = np.array([1.0 + 0.5j, 2.0 + 0.25j])
    s = response.absorption_cross_section(w, 0.02, a)
    assert np.allclose(s, 4.0 * np.pi * w / 137.035999084 * a.imag, rtol=1e-15)
    t = np.array([np.diag([x, x, x]) for x in a])
    assert np.allclose(response.absorption_cross_section(w, 0.02, t), s, rtol=1e-15)
    with pytest.raises(ValueError, match="gamma must be positive"):
        response.absorption_cross_section(w, 0.0, a)
    text = response.table_complex(w, 0.02, t, dict(nsigma=7, resnorm=np.array([1e-9])))
    assert "Re mean" in text and "sigma builds: 7" in text and text.count("omega =") == 2


def test_lu_solve_complex_restatement_and_library():
    rng = np.random.default_rng(2)
    m = rng.standard_normal((7, 7)) + 1j * rng.standard_normal((7, 7))
    r = rng.standard_normal(7) + 1j * rng.standard_normal(7)
    assert np.max(np.abs(npc.lu_solve_complex(m, r) - np.linalg.solve(m, r))) < 1e-12
    assert np.allclose(npc.lu_solve_complex(np.array([[0.0, 2.0j], [1.0, 1.0]]), np.array([2.0j, 2.0])), [1.0, 1.0])
    sing = np.array([[1.0, 2.0j], [2.0, 4.0j]])
    assert npc.lu_solve_complex(sing, np.ones(2)) is None
    assert npc.lu_solve_complex(sing + np.diag([0.0, 1e-12]), np.ones(2), 1e-10 * 4.0) is None
    real = npc.lu_solve_complex(m.real, r.real)
    assert np.all(real.imag == 0.0) and np.max(np.abs(real.real - np_response.lu_solve(m.real, r.real))) < 1e-13
    # the library's host LU (no context, no GPU): (re, im) pairs, column-major
    lib = ctypes.CDLL(capi.LIB_PATH)
    lib.afesp_lu_solve_complex.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_double]

    def solve(a, b, floor=0.0):
        af = np.ascontiguousarray(np.asarray(a, dtype=complex).T).view(np.float64).copy()     # column-major pairs
        bf = np.ascontiguousarray(np.asarray(b, dtype=complex).T).view(np.float64).copy()
        nrhs = 1 if np.ndim(b) == 1 else np.shape(b)[1]
        rc = lib.afesp_lu_solve_complex(len(a), af.ctypes.data, len(a), nrhs, bf.ctypes.data, len(a), floor)
        return rc, bf.view(complex).reshape(np.shape(np.asarray(b).T)).T
    r3 = rng.standard_normal((7, 3)) + 1j * rng.standard_normal((7, 3))
    rc, x = solve(m, r3)
    assert rc == 0 and np.max(np.abs(x - np.linalg.solve(m, r3))) < 1e-12
    rc, x = solve(m, r)
    assert rc == 0 and np.max(np.abs(x - npc.lu_solve_complex(m, r))) < 1e-13
    assert solve(sing, np.ones(2))[0] == 2 and solve(sing + np.diag([0.0, 1e-12]), np.ones(2), 4e-10)[0] == 2
    rc, x = solve(m.real, r.real)
    assert rc == 0 and np.all(x.imag == 0.0)                                 # a real system keeps exactly zero imaginary parts
    assert lib.afesp_lu_solve_complex(0, None, 1, 0, None, 1, 0.0) == 1


def test_polar_gamma_and_c6_keys(tmp_path):
    def write(body):
        (tmp_path / "els.in").write_text("&elsinput\n" + body + "\n/\n")
        return str(tmp_path / "els.in")
    si = inputs.read_els_in(write('calc_type="UCCSD",\ncc_polar=.true.'))
    assert si.polar_gamma == 0.0 and si.polar_c6_npts == 0
    si = inputs.read_els_in(write('calc_type="UCCSD",\ncc_polar=.true.,\npolar_omega=0.0, 0.1,\npolar_gamma=0.02,\npolar_c6_npts=12'))
    assert si.polar_gamma == 0.02 and si.polar_c6_npts == 12 and si.polar_omega == [0.0, 0.1]
    with pytest.raises(ValueError, match="polar_gamma"):
        inputs.read_els_in(write('calc_type="UCCSD",\ncc_polar=.true.,\npolar_gamma=-0.1'))
    with pytest.raises(ValueError, match="polar_c6_npts"):
        inputs.read_els_in(write('calc_type="UCCSD",\ncc_polar=.true.,\npolar_c6_npts=-1'))


def test_library_exports_the_complex_response_entry_points():
    names = ("afesp_ccsd_so_response_init_complex", "afesp_ccsd_so_response_get_vector_complex", "afesp_ccsd_so_response_function_complex")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afesp.h")).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.afesp_version() >= 5
    for s in names + ("afesp_test_davidson_linear_start_complex",):
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS and f"int {s}(afesp_ctx* ctx" in header
        assert getattr(capi.load_library(), s).argtypes is not None, s
    assert hasattr(lib, "afesp_lu_solve_complex") and "afesp_lu_solve_complex" in capi.EXPORTS and "int afesp_lu_solve_complex(int n" in header
    for m in ("so_response_init_complex", "so_response_vector_complex", "so_response_function_complex", "davidson_test_linear_start_complex"):
        assert callable(getattr(capi.Engine, m))
    for m in ("so_response_solve_complex", "polarizability_complex", "absorption_cross_section", "casimir_polder_grid", "c6_coefficient",
              "table_complex"):
        assert callable(getattr(response, m))
    assert lib.afesp_ccsd_so_response_init_complex(None, 1, None, 1, None, 8) == 1     # a NULL context is an argument error, as everywhere
    assert lib.afesp_ccsd_so_response_get_vector_complex(None, 0, 0, None, None, None, None) == 1
    assert lib.afesp_ccsd_so_response_function_complex(None, 1, None, None) == 1
    assert lib.afesp_test_davidson_linear_start_complex(None, 1, None, None, None) == 1
