"""CPU checks of the orbital relaxation of the spin-orbital CCSD density (np_relax): the explicit orbital gradient -- over
the whole arrays and block by block as the device builds it -- against the defining finite difference of the Lagrangian on rotated (f, g);
the Z-vector operator element by element and a conjugate-gradient solve against the dense one; the finite-field identity
d(E_ref + E_CCSD)/d eps = sum V (g0 + D_rel) on models whose determinant is a Hartree-Fock solution; the exact two-electron case; the
cc_relaxed input key and what the built library exports.

Tolerances are measured, not chosen: the finite difference is evaluated at two step sizes and the explicit form is held to ten times
their disagreement."""
import ctypes

import numpy as np
import pytest

import np_density2
import np_lambda
import np_relax
import np_rocc
from afesp_amd import capi, density, inputs
from test_gpu_lambda import SHAPES, _case

_POINTS = {}
H_FD = (2.0 ** -7, 2.0 ** -8)


def _point(name, kind):
    """a shape of test_gpu_lambda.py with its amplitudes (random O(0.3), or converged t and lambda), made once"""
    key = (name, kind)
    if key not in _POINTS:
        c = _case(name)
        o, v = c["o"], c["v"]
        cc = np_rocc.ROCC(c["g"], c["f"], o)
        if kind == "random":
            rng = np.random.default_rng(31)
            t = np_lambda.antisym_random(rng, o, v)
            l = np_lambda.antisym_random(rng, o, v)
        else:
            cc.solve(300, 1e-13, 1e-13)
            t = (cc.t1.copy(), cc.t2.copy())
            l = np_lambda.lambda_solve(cc, *t)
        D = np_lambda.density_explicit(cc, *t, *l)
        G = np_density2.gamma_explicit(*t, *l)
        _POINTS[key] = dict(c=c, cc=cc, o=o, v=v, t=t, l=l, D=D, G=G, F=np_density2.expand(G, o, v), L=np_lambda.lagrangian(cc, *t, *l))
    return _POINTS[key]


@pytest.mark.parametrize("kind", ["random", "converged"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_explicit_gradient_equals_the_defining_form(name, kind):
    """Measured, the larger of the two flags, random / converged amplitudes -- disagreement of the two step sizes, then explicit minus
    finite difference: rhf_fed 5.6e-9 / 1.7e-10, 3.7e-10 / 1.1e-11; uhf_fed 4.5e-9 / 1.6e-10, 3.0e-10 / 1.1e-11; fock_rotated 3.3e-9 /
    5.0e-10, 2.2e-10 / 3.3e-11; two_electron 1.5e-9 / 9.1e-11, 9.9e-11 / 6.0e-12; one_electron 3.1e-9 / 1.1e-10, 2.1e-10 / 7.2e-12.  The
    explicit form sits at 1/15 of the disagreement throughout: the h^4 error of the smaller step itself."""
    p = _point(name, kind)
    c, o = p["c"], p["o"]
    for fr in (0, 1):
        w_small, w_large = np_relax.gradient_fd(c, p["t"], p["l"], fr, H_FD)
        fd_self = float(np.max(np.abs(w_small - w_large)))
        bound = 10.0 * fd_self
        we = np_relax.gradient_explicit(c["g"], c["f"], o, p["D"], p["F"], fr)
        err = float(np.max(np.abs(we - w_small)))
        print(name, kind, "fock_response", fr, "fd disagreement", fd_self, "explicit - fd", err, "bound", bound, "max |w|", np.max(np.abs(we)))
        assert err < bound
        wb, _ = np_relax.gradient_blocks(p["cc"], c["f"], p["D"], p["G"], fr)
        assert np.max(np.abs(wb - we)) < 1e-12 * max(1.0, np.max(np.abs(we)))
    if kind == "random":
        assert np.max(np.abs(we)) > 1e-2                               # the comparison is not one of zeros


def test_two_electron_gradient_vanishes_at_convergence():
    """CCSD is exact for two electrons: E_ref + E_CCSD cannot depend on the orbitals, so the orbital gradient of the whole energy is zero.
    The model's orbitals are NOT the determinant's Hartree-Fock ones (max |f_ov| > 1e-3), so the reference energy brings its own gradient
    dE_ref/dkappa_ai = 2 f_ia, which w is the derivative of the correlation Lagrangian alone does not hold: what vanishes is w_ai + 2 f_ia
    with fock_response = 1 (w itself wherever the determinant is a Hartree-Fock solution); without the Fock response it does not"""
    p = _point("two_electron", "converged")
    c = p["c"]
    fov = c["f"][:p["o"], p["o"]:]
    assert np.max(np.abs(fov)) > 1e-3
    w1 = np_relax.gradient_explicit(c["g"], c["f"], p["o"], p["D"], p["F"], 1)
    w0 = np_relax.gradient_explicit(c["g"], c["f"], p["o"], p["D"], p["F"], 0)
    print("two-electron max |w + 2 f_ov|", np.max(np.abs(w1 + 2.0 * fov)), "without the Fock response", np.max(np.abs(w0 + 2.0 * fov)))
    assert np.max(np.abs(w1 + 2.0 * fov)) < 1e-10 and np.max(np.abs(w0 + 2.0 * fov)) > 1e-6


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_zvector_operator_and_solve(name):
    p = _point(name, "random")
    c, o, v = p["c"], p["o"], p["v"]
    g, lev = c["g"], np.diag(c["f"]).copy()
    A = np_relax.hessian_dense(g, lev, o)
    for i in range(o):                                                  # the definition, element by element
        for a in range(v):
            for j in range(o):
                for b in range(v):
                    ref = g[o + a, o + b, i, j] + g[o + a, j, i, o + b] + ((lev[o + a] - lev[i]) if (i, a) == (j, b) else 0.0)
                    assert A[i * v + a, j * v + b] == ref
    assert np.array_equal(A, A.T) or np.max(np.abs(A - A.T)) < 1e-14
    assert np.all(np.linalg.eigvalsh(0.5 * (A + A.T)) > 0.0)
    w = np_relax.gradient_explicit(g, c["f"], o, p["D"], p["F"], 1)
    z = np_relax.zvector(g, lev, o, w)
    assert np.max(np.abs(A @ z.reshape(-1) + w.reshape(-1))) < 1e-12 * max(1.0, np.max(np.abs(w)))
    zc, it, res = np_relax.pcg(A, -w.reshape(-1), (lev[None, o:] - lev[:o, None]).reshape(-1), 1e-12, 200)
    print(name, "conjugate gradients", it, "iterations, residual", res)
    assert res < 1e-12 and np.max(np.abs(zc.reshape(o, v) - z)) < 1e-10
    d = np_relax.relaxed_density(p["D"], z, o)
    assert np.array_equal(d, d.T) and np.array_equal(d[:o, :o], p["D"][:o, :o]) and np.array_equal(d[o:, o:], p["D"][o:, o:])


def _finite_field(na, nb, seed, delta=2.0 ** -11, scale=0.3):
    n = 5
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n + 2, n, n)) * 0.15
    B = B + B.transpose(0, 2, 1)
    chem = np.einsum("kpq,krs->pqrs", B, B)
    h = 0.05 * rng.standard_normal((n, n))
    h = np.diag(-2.5 + 0.8 * np.arange(n)) + h + h.T
    V = rng.uniform(-1.0, 1.0, (n, n)) * scale
    V = V + V.T

    def solve(eps):
        c = np_relax.scf_case(h + eps * V, chem, na, nb)
        e, t, l = np_relax.ccsd_and_lambda(c["cc"])
        return c, c["e_ref"] + e, t, l
    e = {k: solve(k * delta)[1] for k in (-2, -1, 1, 2)}
    d2 = (e[1] - e[-1]) / (2.0 * delta)
    d4 = (8.0 * (e[1] - e[-1]) - (e[2] - e[-2])) / (12.0 * delta)
    c, _, t, l = solve(0.0)
    r = np_relax.relaxed_reference(c["cc"], c["g"], c["f"], t, l)
    Vso = np_relax.so_operator(V, c)
    g0 = np.diag((np.arange(2 * n) < c["o"]).astype(float))
    return dict(d2=d2, d4=d4, unrelaxed=float(np.sum(Vso * (g0 + r["D"]))), relaxed=float(np.sum(Vso * (g0 + r["D_rel"]))), z=r["z"],
                w=r["w"], c=c)


@pytest.mark.parametrize("na,nb,seed", [(2, 2, 3), (3, 1, 4)])
def test_finite_field_identity_on_a_hartree_fock_model(na, nb, seed):
    """SCF, CCSD and Lambda reconverged at eps = +-delta, +-2 delta (delta = 2^-11, V random symmetric of scale 0.3): the four-point
    derivative of E_ref + E_CCSD against sum V (g0 + D_rel).  Measured: (5,2,2) two-point - four-point 3.1e-9, relaxed misses by 3.6e-12,
    unrelaxed by 8.4e-4; (5,3,1) 1.2e-7, 3.2e-13, 6.4e-4.  The multiple 1/2 of z in D_rel is what this test decides."""
    r = _finite_field(na, nb, seed)
    bound = 10.0 * abs(r["d2"] - r["d4"])
    shift = abs(r["relaxed"] - r["unrelaxed"])
    print((na, nb), "finite difference", r["d4"], "two-point - four-point", abs(r["d2"] - r["d4"]), "bound", bound, "relaxed", r["relaxed"],
          "error", abs(r["relaxed"] - r["d4"]), "unrelaxed", r["unrelaxed"], "error", abs(r["unrelaxed"] - r["d4"]), "max |z|", np.max(np.abs(r["z"])))
    assert shift > 100.0 * bound                                       # or the test shows nothing
    assert abs(r["relaxed"] - r["d4"]) < bound
    assert abs(r["unrelaxed"] - r["d4"]) > 100.0 * bound
    # a Hartree-Fock determinant: the reference itself is stationary (f_ov = 0), and the spin-flip block of z is exactly zero
    c = r["c"]
    assert np.max(np.abs(c["f"][:c["o"], c["o"]:])) == 0.0
    flip = c["spin"][:c["o"], None] != c["spin"][None, c["o"]:]
    assert np.max(np.abs(r["z"][flip])) < 1e-14


def test_rotation_is_orthogonal_and_first_order_in_kappa():
    rng = np.random.default_rng(2)
    k = rng.standard_normal((5, 5)) * 1e-4
    k = k - k.T
    u = np_relax.expm_antisymmetric(k)
    assert np.max(np.abs(u @ u.T - np.eye(5))) < 1e-14 and np.max(np.abs(u - (np.eye(5) + k + 0.5 * k @ k))) < 1e-11
    f = rng.standard_normal((5, 5))
    g = rng.standard_normal((5,) * 4)
    fr, gr = np_relax.rotate(f, g, k)
    assert np.max(np.abs(fr - u.T @ f @ u)) < 1e-14
    assert np.max(np.abs(gr - np.einsum("pqrs,pa,qb,rc,sd->abcd", g, u, u, u, u))) < 1e-13


def test_cc_relaxed_key_and_its_refusals(tmp_path):
    def write(body):
        (tmp_path / "els.in").write_text("&elsinput\n" + body + "\n/\n")
        return str(tmp_path / "els.in")
    assert inputs.read_els_in(write('calc_type="UCCSD"')).cc_relaxed is False
    for calc in inputs.CC_DENSITY_TYPES:
        assert inputs.read_els_in(write(f'calc_type="{calc}",\ncc_relaxed=.true.')).cc_relaxed is True
    for calc in ("CCSD_spatial", "CCSD(T)_spatial", "CRCCSD(T)_spatial", "MP2_spinorb", "UMP2", "RHF"):
        with pytest.raises(ValueError, match="takes no cc_relaxed"):
            inputs.read_els_in(write(f'calc_type="{calc}",\ncc_relaxed=.true.'))
    with pytest.raises(ValueError):
        inputs.read_els_in(write('calc_type="UCCSD",\ncc_relaxed=3'))
    for window in ("frozen_core=.true.", "n_frozen_core=1", "n_frozen_virt=2", "fno_n_virt=5", "fno_occ_tol=1.0d-4"):
        with pytest.raises(ValueError, match="cc_relaxed with a frozen"):
            inputs.read_els_in(write(f'calc_type="CCSD_spinorb",\ncc_relaxed=.true.,\n{window}'))
    both = inputs.read_els_in(write('calc_type="CCSD_spinorb",\ncc_rdm2=.true.,\ncc_relaxed=.true.,\nn_frozen_core=0'))
    assert both.cc_rdm2 and both.cc_relaxed


def test_library_exports_the_relaxation_entry_points():
    names = ("afesp_ccsd_so_orbital_gradient", "afesp_ccsd_so_zvector_apply", "afesp_ccsd_so_zvector_solve", "afesp_ccsd_so_relaxed_density",
             "afesp_ccsd_so_relax_pair_row")
    lib = ctypes.CDLL(capi.LIB_PATH)
    header = open(capi.LIB_PATH.split("a-fortran-electronic-structure-program_amd")[0] + "include/afesp.h").read()
    for s in names:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS
        assert f"int {s}(afesp_ctx* ctx" in header, s
        assert getattr(capi.load_library(), s).argtypes is not None, s
    assert lib.afesp_version() >= 3
    assert "#define AFESP_RELAX_NOT_HF 24" in header and "#define AFESP_RELAX_NOT_CONVERGED 25" in header
    for m in ("so_orbital_gradient", "so_zvector_apply", "so_zvector_solve", "so_relaxed_density"):
        assert callable(getattr(capi.Engine, m))
    assert lib.afesp_ccsd_so_orbital_gradient(None, 1, None, 0) == 1   # a NULL context is an argument error, as everywhere
    assert callable(density.so_relaxed_density_solve)
