"""The Fortran host with cc_lambda_t = .true. on the bundled H2O/cc-pVDZ input as CCSD(T)_spinorb (AFESP_SO_FOO_AS_PUBLISHED=1, as Lambda
needs): o, v = 10, 38, 120 triples.  The Lambda table is printed once, the Lambda-CCSD(T) correction beside the (T) lines; it is the value
of Engine.so_lambda_t on the same input and the numpy evaluation at the fetched amplitudes; two ranks add up to it.

The host prints nine digits on this branch (the format of its (T) line), and the two drivers converge their SCF, CCSD and Lambda
separately (1e-12 / 1e-11 / 1e-11): 'to the digits printed' is one unit of the ninth digit, 1e-9."""
import dataclasses
import re

import numpy as np
import pytest

import molecules
import np_lambda_t as LT
import np_triples as T
import orc
from afesp_amd import density, rhf
from afesp_amd.rhf import unpack_eri
from test_gpu_eom_host import _input_text
from test_gpu_fcidump_in_host import run_from_file
from test_gpu_frozen_host import MGPU, run_host
from test_gpu_rohf_host import TIGHT as ROHF_TIGHT, cation_file  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

CORRECTION = re.compile(r"E\(ΛCCSD\(T\)\) correction \(Hartree\):\s+(-?\d+\.\d{9})\s*$", re.M)
TOTAL = re.compile(r"Unrestricted ΛCCSD\(T\) correlation energy \(Hartree\):\s+(-?\d+\.\d{9})\s*$", re.M)
PT = re.compile(r"Unrestricted CCSD\(T\) correlation energy \(Hartree\):\s+(-?\d+\.\d{9})\s*$", re.M)
FINAL = re.compile(r"Final CCSD Energy \(Hartree\):\s+(-?\d+\.\d+)")
FINAL_ROHF = re.compile(r"Final ROHF-CCSD Energy \(Hartree\):\s+(-?\d+\.\d+)")
DIGIT = 1.0e-9


def _text():
    return _input_text().replace("CCSD_spinorb", "CCSD(T)_spinorb")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    """els_amd with cc_lambda_t alone, once for the module"""
    mp = pytest.MonkeyPatch()
    mp.setenv("AFESP_SO_FOO_AS_PUBLISHED", "1")
    try:
        return run_host(tmp_path_factory.mktemp("lt") / "a", "h2o-cc-pvdz", "", ["cc_lambda_t = .true."], text=_text())
    finally:
        mp.undo()


def test_host_prints_the_correction_of_the_python_path_and_of_numpy(tmp_path, monkeypatch, host_run):
    from afesp_amd.capi import Engine
    monkeypatch.setenv("AFESP_SO_FOO_AS_PUBLISHED", "1")
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_maxiter=200, scf_read_guess=False)
    res = rhf.do_rhf(si, ints, None)
    n, nel = ints.nbasis, ints.nel
    with Engine(0) as eng:
        eng.do_mp2_spatial(n, nel // 2, res.canon_coeff, res.canon_levels, ints.eri)
        eng.init_cc_spinorb(n, nel, res.canon_levels, None, 8, foo_as_published=True)
        nit, en, _ = eng.do_ccsd_spinorb(100, 1e-11, 1e-11)
        assert nit > 0 and (eng.so_o, eng.so_v) == (10, 38)
        e_lt, e_t = density.so_lambda_t_correction(eng, maxiter=100, e_tol=1e-11, l_tol=1e-11)
        t1, t2 = eng.so_amplitudes()
        l1, l2 = eng.so_lambda()
    # float64 numpy at the fetched amplitudes (120 triples: the products through BLAS)
    orb, spin = T.interleaved_order(n, nel)
    g = T.so_g(unpack_eri(n, orc.ao2mo(n, res.canon_coeff, ints.eri)), orb, spin)
    val, S = LT.lt_per_triple(g, res.canon_levels[orb], nel, t1, t2, l1, l2, dtype=np.float64)
    bound = T.tol_factor(10, 38) * float(np.sum(S))
    print("E(Lambda-T)", e_lt, "numpy", float(np.sum(val)), "bound", bound, "E(T)", e_t)
    assert len(val) == 120 and abs(e_lt - float(np.sum(val))) <= bound

    host, got = host_run
    assert host.returncode == 0, host.stdout + host.stderr
    out = host.stdout
    assert out.count("CCSD Lambda") == 1 and "Natural occupation" not in out
    assert out.index("Final CCSD Energy") < out.index("CCSD Lambda") < out.index("\n CCSD(T)\n ----------") < out.index("\n Lambda-CCSD(T)\n")
    corr, total, pt, e_cc = (float(r.search(out).group(1)) for r in (CORRECTION, TOTAL, PT, FINAL))
    print("host", corr, total, pt, e_cc)
    assert abs(corr - e_lt) <= DIGIT
    assert abs(total - (e_cc + corr)) <= 2 * DIGIT and abs(pt - (e_cc + e_t)) <= 2 * DIGIT
    assert abs(got["lambda_ccsd_pt_corr"] - total) <= 2 * DIGIT and abs(got["ccsd_pt_corr"] - pt) <= 2 * DIGIT
    # (T) beside it is the one of a run without the key
    plain, got0 = run_host(tmp_path / "b", "h2o-cc-pvdz", "", [], text=_text())
    assert plain.returncode == 0 and "Lambda" not in plain.stdout and "Λ" not in plain.stdout
    assert float(PT.search(plain.stdout).group(1)) == pt and got0["ccsd_pt_corr"] == got["ccsd_pt_corr"]
    # two ranks: each its shard of the 120 triples, one flagged sum
    two, got2 = run_host(tmp_path / "c", "h2o-cc-pvdz", "", ["cc_lambda_t = .true."], argv=[MGPU, "2", "host"], text=_text())
    assert two.returncode == 0, two.stdout + two.stderr
    assert "Ranks: 2, transport host" in two.stdout
    corr2 = float(CORRECTION.search(two.stdout).group(1))
    assert abs(corr2 - corr) <= 2 * bound + DIGIT
    assert abs(float(PT.search(two.stdout).group(1)) - pt) <= DIGIT


def test_one_lambda_solve_serves_density_eom_and_the_correction(tmp_path, monkeypatch, host_run):
    monkeypatch.setenv("AFESP_SO_FOO_AS_PUBLISHED", "1")
    host, _ = run_host(tmp_path / "a", "h2o-cc-pvdz", "", ["cc_lambda_t = .true.", "cc_density = .true.", "eom_ip_nroots = 1"], text=_text())
    assert host.returncode == 0, host.stdout + host.stderr
    out = host.stdout
    assert out.count("CCSD Lambda\n") == 1 and out.count("L = T") == 1
    assert out.index("Natural occupation numbers") < out.index("\n Lambda-CCSD(T)\n")
    alone, _ = host_run
    assert alone.returncode == 0
    # the EOM sector borrowed the H-bar elements and left Lambda as converged: the same correction
    assert abs(float(CORRECTION.search(out).group(1)) - float(CORRECTION.search(alone.stdout).group(1))) <= DIGIT


def test_host_rohf_branch_prints_the_correction_of_the_python_path(tmp_path, cation_file):  # noqa: F811
    """The open-shell branch of the host on a restricted doublet FCIDUMP (H2O+, semicanonical orbitals, f_ov in the left factor), twelve
    digits printed; 1e-9: two separately converged solves at 1e-11, the bar of test_gpu_rohf_host.py."""
    from afesp_amd import rohf
    from afesp_amd.capi import Engine
    with Engine(0) as eng:
        ref = rohf.rohf_cc(eng, cation_file, 200, 1e-11, 1e-11)
        assert np.max(np.abs(eng.so_tensor("f_ov"))) > 1e-4
        e_lt, e_t = density.so_lambda_t_correction(eng, maxiter=200, e_tol=1e-11, l_tol=1e-11)
    assert abs(e_t - ref.e_t) <= 1e-12
    res, _ = run_from_file(tmp_path / "a", cation_file, "ROHF-CCSD(T)", ROHF_TIGHT + ",\ncc_lambda_t = .true.")
    assert res.returncode == 0, res.stdout + res.stderr
    out = res.stdout

    def printed(label):
        m = re.search(re.escape(label) + r"\s+(-?\d+\.\d{12})\s*$", out, re.M)
        assert m, label
        return float(m.group(1))
    corr, total = printed("E(ΛCCSD(T)) correction (Hartree):"), printed("ROHF-ΛCCSD(T) correlation energy (Hartree):")
    pt, e_cc = printed("ROHF-CCSD(T) correlation energy (Hartree):"), float(FINAL_ROHF.search(out).group(1))
    print("python", e_lt, e_t, "host", corr, total, pt, e_cc)
    assert abs(corr - e_lt) < 1e-9 and abs(pt - e_cc - e_t) < 1e-9 and abs(total - (e_cc + corr)) < 2e-12
    assert out.count("CCSD Lambda\n") == 1 and "Natural occupation" not in out
    assert "ROHF-ΛCCSD(T) correlation energy:" in out[out.index("Final energy breakdown"):]
