"""CPU checks of EOM-IP-CCSD and EOM-EA-CCSD (tests/np_eom_ipea.py): the explicit sigma builds the device code follows against the ghost-
orbital definition, the two-electron model against the one-electron spectrum, Koopmans' theorem at t = 0, the reference Davidson
iteration against the eigenvalues of the sector matrices, and what the built library, the Engine and the input reader export.

The guesses of the Davidson iteration are the device's (np_eom_ipea.guess_vector): unit vectors with a fixed 1e-3 admixture of every unique
amplitude.  With bare unit vectors IP with 6 roots on o4v6, o4v6_canonical and o4v8 converges on eigenvalues 1-4, 6 and 7: the fifth is the
Ms = -3/2 component of a 2h1p quartet, a block that holds none of the six smallest diagonal elements and that sigma never couples to the
others (errors 1.8e-2, 3.0e-2, 9.0e-3 then; test_bare_unit_guesses_miss_a_block keeps that on record)."""
import ctypes

import numpy as np
import pytest

import np_eom
import np_eom_ipea as X
import np_lambda
import np_rocc
from afesp_amd import capi, eom, inputs

SECTORS = {"IP": X.IP, "EA": X.EA}


def _close(x, ref, tol, what):
    err, bound = float(np.max(np.abs(x - ref))), tol * max(1.0, float(np.max(np.abs(ref))))
    print(what, "error", err, "bound", bound)
    assert err < bound, what


def _antisymmetry_defect(sector, x2):
    return float(np.max(np.abs(x2 + (x2.transpose(1, 0, 2) if sector == X.IP else x2.transpose(0, 2, 1)))))


@pytest.mark.parametrize("sector", sorted(SECTORS))
@pytest.mark.parametrize("n,na,nb,seed", [(5, 2, 2, 31), (5, 2, 1, 32), (4, 1, 1, 33), (6, 3, 2, 34)])
def test_explicit_sigma_equals_the_ghost_orbital_definition(n, na, nb, seed, sector):
    """(o,v) = (4,6), (3,7), (2,6), (5,7); at random O(0.3) t and at the converged t; nothing leaks out of the ghost components"""
    sec = SECTORS[sector]
    g, f, o, _ = np_lambda.model(n, na, nb, seed)
    cc = np_rocc.ROCC(g, f, o)
    v = cc.v
    assert (o, v) in ((4, 6), (3, 7), (2, 6), (5, 7))
    rng = np.random.default_rng(seed)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    cc.solve(300, 1e-13, 1e-13)
    for a1, a2, where in ((t1, t2, "random t"), (cc.t1.copy(), cc.t2.copy(), "converged t")):
        r1, r2 = X.random_vector(rng, sec, o, v)
        d1, d2, leak = X.sigma_definition(sec, g, f, o, a1, a2, r1, r2)
        e1, e2 = X.sigma_explicit(sec, cc, a1, a2, r1, r2)
        _close(e1, d1, 1e-12, f"{sector} sigma1 {where}")
        _close(e2, d2, 1e-12, f"{sector} sigma2 {where}")
        assert leak == 0.0
        assert _antisymmetry_defect(sec, e2) < 1e-13 and _antisymmetry_defect(sec, d2) < 1e-13


@pytest.mark.parametrize("sector", sorted(SECTORS))
def test_pack_and_unpack_are_inverse_on_the_unique_amplitudes(sector):
    sec = SECTORS[sector]
    for o, v in ((4, 6), (3, 5), (1, 5), (2, 2)):
        s, d = X.unique(sec, o, v)
        assert len(s) + len(d) == eom.ipea_nunique(sec, o, v)
        r1, r2 = X.random_vector(np.random.default_rng(3), sec, o, v)
        x = X.pack(sec, r1, r2)
        y1, y2 = X.unpack(sec, x, o, v)
        assert np.array_equal(y1, r1) and np.array_equal(y2, r2)
        assert abs(np.dot(x, x) - X.dot(r1, r2, r1, r2)) < 1e-14             # the plain dot of packed vectors is the (1, 1/2) inner product
    assert X.unique(X.IP, 1, 5)[1] == []                                     # one occupied spin orbital: no 2h1p amplitude


def test_two_electron_ips_are_the_one_electron_levels():
    """CCSD is exact for two electrons and the ionised system has one: E(N) + omega_IP runs over the eigenvalues of h, each twofold"""
    n = 4
    h, chem, fa, fb = np_lambda.two_electron_model(n, 21)
    cc = np_rocc.rocc_from_blocks(chem, chem, chem, fa, fb, 1, 1)
    assert np.array_equal(np.diag(np_rocc.so_fock(fa, fb, 1, 1)), np.concatenate([cc.eo, cc.ev]))
    cc.solve(300, 1e-14, 1e-14)
    A = X.matrix(X.IP, cc, cc.t1, cc.t2)
    w = np.linalg.eigvals(A)
    assert A.shape == (8, 8) and np.max(np.abs(w.imag)) < 1e-12
    e0 = np_lambda.fci_two_electron_density(h, chem)[0]
    got, ref = np.sort(e0 + w.real), np.sort(np.repeat(np.linalg.eigvalsh(h), 2))
    print("E(N) + IP against eig(h)", np.max(np.abs(got - ref)))
    assert np.max(np.abs(got - ref)) < 1e-10


def test_koopmans_at_zero_amplitudes():
    g, f, o, _ = np_lambda.model(5, 2, 2, 4, canonical=True)
    cc = np_rocc.ROCC(g, f, o)
    t1, t2 = np.zeros((o, cc.v)), np.zeros((o, o, cc.v, cc.v))
    for i in range(o):
        s1, _ = X.ip_sigma_explicit(cc, t1, t2, *X.unit_vector(X.IP, o, cc.v, (i,)))
        assert abs(s1[i] + cc.eo[i]) < 1e-14 and np.count_nonzero(s1) == 1
    for a in range(cc.v):
        s1, _ = X.ea_sigma_explicit(cc, t1, t2, *X.unit_vector(X.EA, o, cc.v, (a,)))
        assert abs(s1[a] - cc.ev[a]) < 1e-14 and np.count_nonzero(s1) == 1


def test_guess_order_follows_the_diagonal_and_the_flat_index():
    c = np_eom.converged_model("o4v6_canonical")
    cc = c["cc"]
    for sec in (X.IP, X.EA):
        order = X.guess_order(sec, cc)
        d1, d2 = X.diagonal(sec, cc)
        vals = [d1[k] if len(k) == 1 else d2[k] for k in order]
        assert vals == sorted(vals) and len(order) == eom.ipea_nunique(sec, cc.o, cc.v)
        x1, x2 = X.unit_vector(sec, cc.o, cc.v, order[-1])
        assert abs(X.dot(x1, x2, x1, x2) - 1.0) < 1e-15 and _antisymmetry_defect(sec, x2) == 0.0
    assert [k for k in X.guess_order(X.IP, cc)[:4]] == sorted(X.guess_order(X.IP, cc)[:4], key=lambda k: -cc.eo[k[0]])   # Koopmans order


@pytest.mark.parametrize("sector", sorted(SECTORS))
@pytest.mark.parametrize("name", sorted(np_eom.MODELS))
@pytest.mark.parametrize("nroots", [4, 6])
def test_reference_davidson_finds_the_lowest_roots(name, nroots, sector):
    sec = SECTORS[sector]
    c = X.converged_sector(name, sec)
    cc, t1, t2, w = c["cc"], c["t1"], c["t2"], c["w"]
    o, v = cc.o, cc.v
    assert np.max(np.abs(w[:8].imag)) < 1e-12
    I = np_lambda.hbar(cc, t1, t2)
    sigma = lambda x: X.pack(sec, *X.sigma_explicit(sec, cc, t1, t2, *X.unpack(sec, x, o, v), I))
    guesses = [X.pack(sec, *X.guess_vector(sec, o, v, k)) for k in X.guess_order(sec, cc)[:nroots]]
    max_space, collapses = X.davidson_case(name, sec, nroots)
    omega, V, info = X.davidson(sigma, X.pack(sec, *X.diagonal(sec, cc)), guesses, nroots, tol=1e-8, max_space=max_space, maxiter=1000)
    print(sector, name, nroots, "max_space", max_space, info["iterations"], "iterations", info["nsigma"], "sigma builds", info["collapses"],
          "collapses, omega - w", np.max(np.abs(omega - w[:nroots].real)), "omega", omega, "w", w[:nroots + 2].real)
    assert (info["collapses"] > 0) == collapses
    for k in range(nroots):
        assert np.linalg.norm(c["A"] @ V[k] - omega[k] * V[k]) < 1e-7
    assert np.max(np.abs(omega - w[:nroots].real)) < 1e-8


def test_bare_unit_guesses_miss_a_block():
    """why the guesses carry an admixture: on o4v6 the fifth IP eigenvalue is an Ms = -3/2 quartet component, which six bare unit guesses
    never reach -- the iteration converges, on eigenvalues 1-4, 6, 7"""
    sec = X.IP
    c = X.converged_sector("o4v6", sec)
    cc, t1, t2, w = c["cc"], c["t1"], c["t2"], c["w"].real
    o, v = cc.o, cc.v
    I = np_lambda.hbar(cc, t1, t2)
    sigma = lambda x: X.pack(sec, *X.sigma_explicit(sec, cc, t1, t2, *X.unpack(sec, x, o, v), I))
    guesses = [X.pack(sec, *X.unit_vector(sec, o, v, k)) for k in X.guess_order(sec, cc)[:6]]
    omega, V, _ = X.davidson(sigma, X.pack(sec, *X.diagonal(sec, cc)), guesses, 6, tol=1e-8, max_space=24, maxiter=300)
    assert np.max(np.abs(omega - w[[0, 1, 2, 3, 5, 6]])) < 1e-8
    x1, x2 = X.unpack(sec, np.linalg.eig(c["A"])[1][:, np.argsort(np.linalg.eigvals(c["A"]).real)[4]].real, o, v)
    assert np.max(np.abs(x1)) < 1e-10                                        # the missed root: no 1h component at all


def test_library_engine_and_driver_export_the_ip_and_ea_entry_points():
    names = ("afesp_ccsd_so_eom_ipea_init", "afesp_ccsd_so_eom_ipea_sigma", "afesp_ccsd_so_eom_ipea_guess", "afesp_ccsd_so_eom_ipea_set_guess",
             "afesp_ccsd_so_eom_ipea_iterate", "afesp_ccsd_so_eom_ipea_get_vector")
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in names:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS
        assert getattr(capi.load_library(), s).argtypes is not None, s
    for m in ("so_eom_ipea_init", "so_eom_ipea_sigma", "so_eom_ipea_guess", "so_eom_ipea_set_guess", "so_eom_ipea_iterate", "so_eom_ipea_vector"):
        assert callable(getattr(capi.Engine, m))
    assert (capi.Engine.EOM_IP, capi.Engine.EOM_EA) == (1, 2) == (eom.SECTOR_IP, eom.SECTOR_EA)
    assert callable(eom.so_eom_ip_solve) and callable(eom.so_eom_ea_solve) and callable(eom.label_ipea_root)
    for sector in (1, 2, 3):                                                 # a NULL context is an argument error, as everywhere
        assert lib.afesp_ccsd_so_eom_ipea_init(None, sector, 1, 2) == 1
        assert lib.afesp_ccsd_so_eom_ipea_guess(None, sector) == 1
        assert lib.afesp_ccsd_so_eom_ipea_sigma(None, sector, 1, None, None, None, None) == 1
        assert lib.afesp_ccsd_so_eom_ipea_set_guess(None, sector, 0, None, None) == 1
        assert lib.afesp_ccsd_so_eom_ipea_iterate(None, sector, ctypes.c_double(1e-8), None, None, None, None, None) == 1
        assert lib.afesp_ccsd_so_eom_ipea_get_vector(None, sector, 0, None, None) == 1


def test_label_ipea_root_reads_the_spin_from_the_spin_order():
    n, na, nb = 4, 2, 1                                                      # block order: occ a a b | virt a a b b b
    o, v = na + nb, 2 * n - na - nb
    x1, x2 = np.zeros(o), np.zeros((o, o, v))
    x1[2] = 0.9                                                              # a beta electron leaves orbital 0: Ms + 1/2
    lab = eom.label_ipea_root(eom.SECTOR_IP, x1, x2, n, na, nb, False)
    assert (lab["kind"], lab["occ"], lab["virt"], lab["spins_occ"], lab["delta_ms"]) == ("1h", (0,), (), (1,), 0.5)
    x2[0, 1, 2] = 1.5                                                        # alpha 0 and alpha 1 leave, beta 1 arrives: Ms - 3/2
    lab = eom.label_ipea_root(eom.SECTOR_IP, x1, x2, n, na, nb, False)
    assert (lab["kind"], lab["occ"], lab["virt"], lab["spins_virt"], lab["delta_ms"]) == ("2h1p", (0, 1), (1,), (1,), -1.5)
    y1, y2 = np.zeros(v), np.zeros((o, v, v))
    y1[1] = -0.8                                                             # an alpha electron arrives in orbital 3: Ms + 1/2
    lab = eom.label_ipea_root(eom.SECTOR_EA, y1, y2, n, na, nb, False)
    assert (lab["kind"], lab["occ"], lab["virt"], lab["spins_virt"], lab["delta_ms"]) == ("1p", (), (3,), (0,), 0.5)
    y2[2, 0, 3] = 1.0                                                        # beta 0 leaves, alpha 2 and beta 2 arrive: Ms + 1/2
    lab = eom.label_ipea_root(eom.SECTOR_EA, y1, y2, n, na, nb, False)
    assert (lab["kind"], lab["occ"], lab["virt"], lab["delta_ms"]) == ("2p1h", (0,), (2, 2), 0.5)
    z1 = np.zeros(4)                                                         # interleaved, o = v = 4: virtual 1 = (orbital 2, beta)
    z1[1] = 1.0
    lab = eom.label_ipea_root(eom.SECTOR_EA, z1, np.zeros((4, 4, 4)), 4, 2, 2, True)
    assert (lab["virt"], lab["spins_virt"], lab["delta_ms"]) == ((2,), (1,), -0.5)


@pytest.mark.parametrize("key", ["eom_ip_nroots", "eom_ea_nroots"])
def test_the_els_in_keys_are_refused_on_the_types_that_run_no_spin_orbital_ccsd(tmp_path, key):
    def write(body):
        (tmp_path / "els.in").write_text("&elsinput\n" + body + "\n/\n")
        return str(tmp_path / "els.in")
    assert getattr(inputs.read_els_in(write('calc_type="UCCSD"')), key) == 0
    for calc in inputs.CC_DENSITY_TYPES:
        assert getattr(inputs.read_els_in(write(f'calc_type="{calc}",\n{key}=4')), key) == 4
    for calc in ("CCSD_spatial", "CCSD(T)_spatial", "CRCCSD(T)_spatial", "MP2_spinorb", "UMP2", "RHF"):
        with pytest.raises(ValueError, match=f"takes no {key}"):
            inputs.read_els_in(write(f'calc_type="{calc}",\n{key}=2'))
        assert getattr(inputs.read_els_in(write(f'calc_type="{calc}",\n{key}=0')), key) == 0
    for bad in ("-1", ".true.", "1.5"):
        with pytest.raises(ValueError, match=key):
            inputs.read_els_in(write(f'calc_type="UCCSD",\n{key}={bad}'))
    both = inputs.read_els_in(write('calc_type="CCSD_spinorb",\neom_nroots=2,\neom_ip_nroots=3,\neom_ea_nroots=5,\ncc_density=.true.'))
    assert (both.eom_nroots, both.eom_ip_nroots, both.eom_ea_nroots, both.cc_density) == (2, 3, 5, True)
