"""CPU checks of the two-particle density of spin-orbital CCSD: the explicit term-by-term form the device code follows
(np_density2.gamma_explicit) against the defining finite difference in g (gamma_fd), the Lagrangian as a functional of (f, g), the partial
trace, FCI for two electrons (2-RDM, energy, <S^2>), the cc_rdm2 input key, and what the built library exports."""
import ctypes

import numpy as np
import pytest

import np_density2
import np_lambda
import np_rocc
import np_ucc
from afesp_amd import capi, density, inputs


def _model(name):
    """(g, f, o, n spatial, nalpha, nbeta, extra)"""
    if name == "o3v3":
        g, f, o, _ = np_lambda.model(3, 2, 1, 5)
        return g, f, o, 3, 2, 1, None
    if name == "o2v4":
        h, chem, fa, fb = np_lambda.two_electron_model(3, 21)
        g, _, o = np_ucc.so_integrals(chem, chem, chem, np.diag(fa).copy(), np.diag(fb).copy(), 1, 1)
        return g, np_rocc.so_fock(fa, fb, 1, 1), o, 3, 1, 1, (h, chem, fa, fb)
    g, f, o, _ = np_lambda.model(6, 3, 2, 9)      # o5v7: o, v and both pair counts (10, 21) differ
    return g, f, o, 6, 3, 2, None


_POINTS = {}


def _point(name, kind):
    """a model with its amplitudes (random O(0.3), or converged t and lambda) and the defining Gamma, made once"""
    key = (name, kind)
    if key not in _POINTS:
        g, f, o, n, na, nb, extra = _model(name)
        v = g.shape[0] - o
        cc = np_rocc.ROCC(g, f, o)
        if kind == "random":
            rng = np.random.default_rng(31)
            t1, t2 = np_lambda.antisym_random(rng, o, v)
            l1, l2 = np_lambda.antisym_random(rng, o, v)
        else:
            cc.solve(300, 1e-13, 1e-13)
            t1, t2 = cc.t1.copy(), cc.t2.copy()
            l1, l2 = np_lambda.lambda_solve(cc, t1, t2)
        _POINTS[key] = dict(g=g, f=f, o=o, v=v, n=n, na=na, nb=nb, extra=extra, cc=cc, t1=t1, t2=t2, l1=l1, l2=l2,
                            fd=np_density2.gamma_fd(g, f, o, t1, t2, l1, l2))
    return _POINTS[key]


def _close(x, ref, tol, what):
    err, bound = float(np.max(np.abs(x - ref))) if ref.size else 0.0, tol * max(1.0, float(np.max(np.abs(ref))) if ref.size else 1.0)
    print(what, err, bound)
    assert err < bound, what


@pytest.mark.parametrize("kind", ["random", "converged"])
@pytest.mark.parametrize("name", ["o3v3", "o2v4", "o5v7"])
def test_explicit_form_equals_the_defining_form(name, kind):
    c = _point(name, kind)
    o, v = c["o"], c["v"]
    assert (o, v) == dict(o3v3=(3, 3), o2v4=(2, 4), o5v7=(5, 7))[name]
    G = np_density2.gamma_explicit(c["t1"], c["t2"], c["l1"], c["l2"])
    ref = np_density2.blocks_of(c["fd"], o)
    for k in np_density2.BLOCKS:
        _close(G[k], ref[k], 1e-12, f"{name} {kind} {k}")
    full = np_density2.expand(G, o, v)
    _close(full, c["fd"], 1e-12, f"{name} {kind} full")
    # the symmetry of real integrals, to the bit (the symmetrisers are sums over images), and the pair form of vvvv
    assert np.array_equal(full, -full.transpose(1, 0, 2, 3)) and np.array_equal(full, -full.transpose(0, 1, 3, 2))
    assert np.array_equal(full, full.transpose(2, 3, 0, 1))
    assert np.array_equal(np_density2.unpair(np_density2.pairs_of(G["vvvv"]), v), G["vvvv"])


@pytest.mark.parametrize("name", ["o3v3", "o5v7"])
def test_lagrangian_is_the_functional_of_f_and_g(name):
    """sum f' D + 1/4 sum g' Gamma = L(g', f') for a random antisymmetric, pair-symmetric g' and a random symmetric f': D and Gamma do not
    depend on (f, g)"""
    c = _point(name, "random")
    o, n = c["o"], c["g"].shape[0]
    t = (c["t1"], c["t2"], c["l1"], c["l2"])
    G = np_density2.expand(np_density2.gamma_explicit(*t), o, c["v"])
    D = np_lambda.density_explicit(c["cc"], *t)
    rng = np.random.default_rng(17)
    g2 = rng.uniform(-1.0, 1.0, (n,) * 4)
    g2 = g2 - g2.transpose(1, 0, 2, 3)
    g2 = g2 - g2.transpose(0, 1, 3, 2)
    g2 = g2 + g2.transpose(2, 3, 0, 1)
    f2 = rng.uniform(-1.0, 1.0, (n, n))
    f2 = f2 + f2.T
    for gg, ff in ((c["g"], c["f"]), (g2, f2)):
        L = np_lambda.lagrangian(np_rocc.ROCC(gg, ff, o), *t)
        val = float(np.sum(ff * D) + 0.25 * np.sum(gg * G))
        print(name, "L", L, "density side", val, abs(val - L))
        assert abs(val - L) < 1e-11 * max(1.0, abs(L))
    fam = np_density2.family_energies(np_density2.gamma_explicit(*t), c["g"], o)
    assert abs(np.sum(fam) - 0.25 * np.sum(c["g"] * G)) < 1e-12


@pytest.mark.parametrize("name", ["o3v3", "o2v4", "o5v7"])
def test_partial_trace_of_the_full_density(name):
    """sum_q Gtot_pqrq = (N - 1) gamma_pr at ANY t and lambda: the number operator commutes with T"""
    c = _point(name, "random")
    o = c["o"]
    t = (c["t1"], c["t2"], c["l1"], c["l2"])
    D = np_lambda.density_explicit(c["cc"], *t)
    gt = np_density2.total_rdm2(D, np_density2.expand(np_density2.gamma_explicit(*t), o, c["v"]), o)
    assert np.array_equal(gt, density.total_rdm2(D, np_density2.expand(np_density2.gamma_explicit(*t), o, c["v"]), o))
    gamma = D + np.diag((np.arange(D.shape[0]) < o).astype(float))
    _close(np.einsum("pqrq->pr", gt), (o - 1) * gamma, 1e-12, f"{name} partial trace")
    assert abs(np.einsum("pqpq->", gt) - o * (o - 1)) < 1e-11


def test_two_electron_model_against_fci():
    """CCSD is exact for two electrons: Gtot is the 2-RDM of the FCI vector, h gamma + 1/4 g Gtot = E_FCI, <S^2> = 0"""
    c = _point("o2v4", "converged")
    h, chem, fa, fb = c["extra"]
    n, o, v = 3, c["o"], c["v"]
    t = (c["t1"], c["t2"], c["l1"], c["l2"])
    D = np_lambda.density_explicit(c["cc"], *t)
    gt = np_density2.total_rdm2(D, np_density2.expand(np_density2.gamma_explicit(*t), o, v), o)
    Hm = (np.einsum("pr,qs->pqrs", h, np.eye(n)) + np.einsum("pr,qs->pqrs", np.eye(n), h) + chem.transpose(0, 2, 1, 3)).reshape(n * n, n * n)
    w, vec = np.linalg.eigh(Hm)
    cf = vec[:, 0].reshape(n, n)                                   # over |p alpha, q beta>
    orb, spin = np_ucc.so_order(n, 1, 1)
    ia, ib = np.where(spin == 0)[0], np.where(spin == 1)[0]
    ref = np.zeros((2 * n,) * 4)
    x = np.einsum("pq,rs->pqrs", cf, cf)[np.ix_(orb[ia], orb[ib], orb[ia], orb[ib])]
    ref[np.ix_(ia, ib, ia, ib)] = x
    ref[np.ix_(ib, ia, ib, ia)] = x.transpose(1, 0, 3, 2)
    ref[np.ix_(ib, ia, ia, ib)] = -x.transpose(1, 0, 2, 3)
    ref[np.ix_(ia, ib, ib, ia)] = -x.transpose(0, 1, 3, 2)
    _close(gt, ref, 1e-10, "two-electron 2-RDM against FCI")
    hso = np.where(spin[:, None] == spin[None, :], h[np.ix_(orb, orb)], 0.0)
    gamma = D + np.diag((np.arange(2 * n) < o).astype(float))
    e = float(np.sum(hso * gamma) + 0.25 * np.sum(c["g"] * gt))
    print("h gamma + 1/4 g Gtot", e, "E_FCI", w[0])
    assert abs(e - w[0]) < 1e-10
    # the density-side correlation energy is the CCSD energy
    e_cc = c["cc"].energy_step()[0]
    assert abs(np.sum(c["f"] * D) + 0.25 * np.sum(c["g"] * (gt - np_density2.total_rdm2(D, 0.0, o))) - e_cc) < 1e-10
    s2 = np_density2.s_squared(gt, orb, spin, 1, 1)
    print("<S^2>", s2)
    assert abs(s2) < 1e-10


def test_s_squared_of_determinants_and_of_a_doublet():
    """the reference determinant alone: Ms (Ms + 1) + nbeta - sum <b|a>^2; the converged doublet of the canonical model stays within 1e-5 of
    0.75, and different alpha / beta orbital sets enter through their overlap only"""
    n, na, nb = 3, 2, 1
    assert abs(density.s_squared_reference(n, na, nb, False) - 0.75) < 1e-14
    assert abs(density.s_squared_reference(n, 2, 2, True)) < 1e-14
    r = np_rocc.random_orthogonal(np.random.default_rng(3), n, 0.3)
    expect = 0.75 + nb - float(np.sum(r[:nb, :na] ** 2))
    assert abs(density.s_squared_reference(n, na, nb, False, r) - expect) < 1e-13
    g, f, o, _ = np_lambda.model(n, na, nb, 5, canonical=True)
    cc = np_rocc.ROCC(g, f, o)
    cc.solve(300, 1e-13, 1e-13)
    l1, l2 = np_lambda.lambda_solve(cc, cc.t1, cc.t2)
    t = (cc.t1, cc.t2, l1, l2)
    D = np_lambda.density_explicit(cc, *t)
    gt = np_density2.total_rdm2(D, np_density2.expand(np_density2.gamma_explicit(*t), o, cc.v), o)
    orb, spin = np_ucc.so_order(n, na, nb)
    s2 = np_density2.s_squared(gt, orb, spin, na, nb)
    print("<S^2> of the converged doublet", s2)
    assert abs(s2 - 0.75) < 1e-5


def test_cc_rdm2_key_and_its_refusals(tmp_path):
    def write(body):
        (tmp_path / "els.in").write_text("&elsinput\n" + body + "\n/\n")
        return str(tmp_path / "els.in")
    assert inputs.read_els_in(write('calc_type="UCCSD"')).cc_rdm2 is False
    for calc in inputs.CC_DENSITY_TYPES:
        assert inputs.read_els_in(write(f'calc_type="{calc}",\ncc_rdm2=.true.')).cc_rdm2 is True
    for calc in ("CCSD_spatial", "CCSD(T)_spatial", "CRCCSD(T)_spatial", "MP2_spinorb", "UMP2", "RHF"):
        with pytest.raises(ValueError, match="takes no cc_rdm2"):
            inputs.read_els_in(write(f'calc_type="{calc}",\ncc_rdm2=.true.'))
    with pytest.raises(ValueError):
        inputs.read_els_in(write('calc_type="UCCSD",\ncc_rdm2=3'))
    with pytest.raises(ValueError, match="UHF FCIDUMP"):
        inputs.read_els_in(write('calc_type="UCCSD",\ncc_rdm2=.true.,\nfcidump_in=.true.'))
    both = inputs.read_els_in(write('calc_type="CCSD_spinorb",\ncc_rdm2=.true.,\ncc_density=.true.'))
    assert both.cc_rdm2 and both.cc_density


def test_library_exports_the_density2_entry_points():
    names = ("afesp_ccsd_so_density2_build", "afesp_ccsd_so_density2_get", "afesp_ccsd_so_density2_energy", "afesp_ccsd_so_density2_expect")
    lib = ctypes.CDLL(capi.LIB_PATH)
    header = open(capi.LIB_PATH.split("a-fortran-electronic-structure-program_amd")[0] + "include/afesp.h").read()
    for s in names:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS
        assert f"int {s}(afesp_ctx* ctx" in header, s
        assert getattr(capi.load_library(), s).argtypes is not None, s
    for m in ("so_density2_build", "so_density2_get", "so_density2_energy", "so_density2_expect"):
        assert callable(getattr(capi.Engine, m))
    assert lib.afesp_ccsd_so_density2_build(None) == 1              # a NULL context is an argument error, as everywhere
    for f in ("total_rdm2", "s_squared", "s_squared_reference", "energy_from_densities"):
        assert callable(getattr(density, f))
