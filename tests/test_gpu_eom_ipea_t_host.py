"""The Fortran host with eom_ip_nroots = eom_ea_nroots = 2, eom_ipea_left and eom_ipea_triples on the bundled H2O/cc-pVDZ input as
CCSD_spinorb (AFESP_SO_FOO_AS_PUBLISHED=1, as tests/test_gpu_eom_ipea_left_host.py: o, v = 10, 38, 120 triples for IP and 45 pairs for EA):
after each sector's left table it calls the library once for all roots and prints root, omega, delta omega, omega + delta omega.  The
delta omega are those of the Python path (afesp_amd.eom.so_eom_ip_triples_correction / _ea_) on the same input, which in turn is the numpy
evaluation at the fetched vectors; two ranks add up to one rank's values; without eom_ipea_left the key is refused; without the key the
output is the one of before.

1e-9 between the two drivers: the correction is bilinear in vectors that two separately converged Davidson solves (residuals 1e-8)
deliver, and it is of the order 1e-3 Eh here.  The two members of a doublet are mixed differently by the two drivers: what is compared
is the root's delta omega, which is the same for either member."""
import dataclasses
import re

import numpy as np
import pytest

import molecules
import np_eom_ipea_t as Q
import np_triples as T
import orc
from afesp_amd import density, eom, rhf
from afesp_amd.rhf import unpack_eri
from test_gpu_eom_host import _input_text, _untimed
from test_gpu_eom_ipea_host import HEAD, TAIL
from test_gpu_frozen_host import MGPU, run_host

pytestmark = pytest.mark.gpu

T_HEAD = {"IP": " Non-iterative triples correction to the EOM-IP-CCSD roots", "EA": " Non-iterative triples correction to the EOM-EA-CCSD roots"}
T_TAIL = {"IP": "Time taken for the EOM-IP-CCSD triples correction:", "EA": "Time taken for the EOM-EA-CCSD triples correction:"}
T_ROW = re.compile(r"^\s+(\d+)\s+(-?\d+\.\d{12})\s+(-?\d+\.\d{12})\s+(-?\d+\.\d{12})\s+(-?\d+\.\d{10})\s*$", re.M)
ROOTS = ["eom_ip_nroots = 2", "eom_ea_nroots = 2"]
KEYS = ROOTS + ["eom_ipea_left = .true.", "eom_ipea_triples = .true."]
SECTORS = {"IP": eom.SECTOR_IP, "EA": eom.SECTOR_EA}


def _rows(out, sector):
    assert out.index(HEAD[sector]) < out.index(" Left eigenvectors: Davidson steps:", out.index(HEAD[sector])) < out.index(T_HEAD[sector]) \
        < out.index(T_TAIL[sector]) < out.index(TAIL[sector])
    block = out[out.index(T_HEAD[sector]):out.index(T_TAIL[sector])]
    print(block)
    return [(int(m.group(1)),) + tuple(float(m.group(q)) for q in range(2, 6)) for m in T_ROW.finditer(block)], block


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from afesp_amd.capi import Engine
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("AFESP_SO_FOO_AS_PUBLISHED", "1")
        si, ints, _, _ = molecules.load("h2o-cc-pvdz")
        si = dataclasses.replace(si, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_maxiter=200, scf_read_guess=False)
        res = rhf.do_rhf(si, ints, None)
        n, nel = ints.nbasis, ints.nel
        py = {}
        with Engine(0) as eng:
            eng.do_mp2_spatial(n, nel // 2, res.canon_coeff, res.canon_levels, ints.eri)
            eng.init_cc_spinorb(n, nel, res.canon_levels, None, 8, foo_as_published=True)
            nit, _, _ = eng.do_ccsd_spinorb(100, 1e-11, 1e-11)
            assert nit > 0 and (eng.so_o, eng.so_v) == (10, 38)
            density.so_lambda_solve(eng, 100, 1e-11, 1e-11)
            _, t2 = eng.so_amplitudes()
            for sector, solve, left, correct in (("IP", eom.so_eom_ip_solve, eom.so_eom_ip_left_solve, eom.so_eom_ip_triples_correction),
                                                 ("EA", eom.so_eom_ea_solve, eom.so_eom_ea_left_solve, eom.so_eom_ea_triples_correction)):
                omega, R, _ = solve(eng, 2)
                wl, L, _ = left(eng, R)
                L = eom.biorthonormalise_ipea(omega, L, R)
                delta, corrected, info = correct(eng, omega, L, R)
                print(sector, "python driver:\n" + eom.triples_table(omega, delta, info))
                py[sector] = dict(omega=omega, L=L, R=R, delta=delta, info=info)
        # float64 numpy at the fetched vectors
        orb, spin = T.interleaved_order(n, nel)
        g = T.so_g(unpack_eri(n, orc.ao2mo(n, res.canon_coeff, ints.eri)), orb, spin)
        for sector, p in py.items():
            p["ref"] = [Q.per_item_explicit(SECTORS[sector], g, res.canon_levels[orb], nel, t2, p["omega"][k], *p["L"][k], *p["R"][k], dtype=np.float64)
                        for k in range(2)]
        tmp = tmp_path_factory.mktemp("eom_ipea_t_host")
        one, _ = run_host(tmp / "a", "h2o-cc-pvdz", "", KEYS, text=_input_text())
        two, _ = run_host(tmp / "b", "h2o-cc-pvdz", "", KEYS, argv=[MGPU, "2", "host"], text=_input_text())
        refused, _ = run_host(tmp / "c", "h2o-cc-pvdz", "", ROOTS + ["eom_ipea_triples = .true."], text=_input_text())
        plain, _ = run_host(tmp / "d", "h2o-cc-pvdz", "", ROOTS + ["eom_ipea_left = .true."], text=_input_text())
    return dict(py=py, one=one, two=two, refused=refused, plain=plain)


def test_python_path_equals_numpy_at_the_fetched_vectors(runs):
    """both sides in double precision: each within np_eom_ipea_t.tol_factor of the exact value, so within twice that of each other"""
    for sector, p in runs["py"].items():
        for k in range(2):
            val, S = p["ref"][k]
            bound = 2 * Q.tol_factor(SECTORS[sector], 10, 38) * float(np.sum(S))
            print(sector, "root", k + 1, "omega", p["omega"][k], "delta", p["delta"][k], "numpy", float(np.sum(val)), "bound", bound)
            assert len(val) == (120 if sector == "IP" else 45) and abs(p["delta"][k] - float(np.sum(val))) <= bound
        assert abs(p["delta"][0] - p["delta"][1]) < 1e-9                    # the two members of the lowest doublet


def test_host_prints_the_corrections_of_the_python_path(runs):
    host = runs["one"]
    assert host.returncode == 0, host.stdout + host.stderr
    for sector, p in runs["py"].items():
        rows, block = _rows(host.stdout, sector)
        assert [r[0] for r in rows] == [1, 2], block
        got = np.array([r[2] for r in rows])
        print(sector, "host", got, "python driver", p["delta"])
        assert np.max(np.abs(np.array([r[1] for r in rows]) - p["omega"])) < 1e-8
        assert np.max(np.abs(got - p["delta"])) < 1e-9
        for r in rows:
            assert abs(r[3] - (r[1] + r[2])) < 2e-12 and abs(r[4] - r[3] * eom.HARTREE_EV) < 1e-9
        assert ("not reliable" in block) == bool(p["info"]["intruder"])
        assert host.stdout.count(T_HEAD[sector]) == 1                       # one call, one table: not one per root


def test_one_rank_and_two_ranks_agree(runs):
    two = runs["two"]
    assert two.returncode == 0, two.stdout + two.stderr
    assert "Ranks: 2, transport host" in two.stdout
    for sector in SECTORS:
        a, b = _rows(runs["one"].stdout, sector)[0], _rows(two.stdout, sector)[0]
        assert len(a) == len(b) == 2
        assert max(abs(x[2] - y[2]) for x, y in zip(a, b)) < 1e-9


def test_host_refuses_the_key_without_eom_ipea_left(runs):
    host = runs["refused"]
    assert host.returncode != 0 and "eom_ipea_triples needs eom_ipea_left" in host.stdout + host.stderr


def test_without_the_key_the_output_is_the_one_of_before(runs):
    """the run with the key, its two triples tables taken out, against the run without: the same lines, numbers to the parity bar of two
    separately converged solves"""
    plain, out = runs["plain"], runs["one"].stdout
    assert plain.returncode == 0 and "triples correction" not in plain.stdout
    for sector in SECTORS:
        lo = out.index(T_HEAD[sector])
        hi = out.index("\n", out.index(T_TAIL[sector])) + 1
        out = out[:lo] + out[hi:]
    a, b = _untimed(out), _untimed(plain.stdout)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty), (x, y)
        for p, q in zip(tx, ty):
            if p != q:
                assert abs(float(p) - float(q)) < 1e-8, (x, y)
