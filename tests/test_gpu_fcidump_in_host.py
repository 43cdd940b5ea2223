"""The Fortran host with fcidump_in = .true.: els_amd writes an active space (fcidump_active), then a second run in a directory that holds
nothing but els.in and that FCIDUMP -- no SCF, no transform -- must print the same total energies.  1e-8 Eh: the parity bar of README.md
(the F15.10 printout level of the other host tests)."""
import shutil
import subprocess

import pytest

from afesp_amd import inputs
from test_gpu_fcidump_host import H2O_IN
from test_gpu_frozen_host import EXE, run_host
from test_uhf_cpu import H2O_CATION_IN

pytestmark = pytest.mark.gpu
FILE_IN = ('&elsinput\ncalc_type="{calc}",\nccsd_e_tol=1e-10,\nccsd_t_tol=1e-10,\nccsd_diis_n_errmat=8,\nccsd_maxiter=200,\n'
           'fcidump_in = .true.{more}\n/\n')


def run_from_file(tmp_path, dump, calc, more=""):
    tmp_path.mkdir(exist_ok=True)
    if dump is not None:
        shutil.copy(dump, tmp_path / "FCIDUMP")
    (tmp_path / "els.in").write_text(FILE_IN.format(calc=calc, more=more))
    res = subprocess.run([EXE], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    (tmp_path / "els.out").write_text(res.stdout)
    return res, inputs.parse_els_out(str(tmp_path / "els.out"))


def test_host_closed_shell_from_the_file_it_wrote(tmp_path):
    text = H2O_IN.format(calc="CCSD(T)_spatial", more="").replace("ccsd_e_tol=1e-8", "ccsd_e_tol=1e-10").replace("ccsd_t_tol=1e-8", "ccsd_t_tol=1e-10")
    res, got = run_host(tmp_path / "a", "h2o-cc-pvdz", "", ["n_frozen_core = 1", "fcidump_active = .true."], text=text)
    assert res.returncode == 0, res.stdout + res.stderr
    res2, got2 = run_from_file(tmp_path / "b", tmp_path / "a" / "FCIDUMP", "CCSD(T)_spatial")
    assert res2.returncode == 0, res2.stdout + res2.stderr
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["FCIDUMP", "els.in", "els.out"]
    assert "Largest off-diagonal Fock element:" in res2.stdout and "Reference determinant energy (Hartree):" in res2.stdout
    assert "Time taken for restricted Hartree-Fock" not in res2.stdout and "Performing AO to MO" not in res2.stdout
    for key in ("mp2_corr", "ccsd_corr", "ccsd_pt_corr"):
        print(key, got[key], got2[key], got["rhf_total"] + got[key], got2["rhf_total"] + got2[key])
        assert abs((got["rhf_total"] + got[key]) - (got2["rhf_total"] + got2[key])) < 1e-8
    assert abs(got["total"] - got2["total"]) < 1e-8 and got2["e_nuc"] == 0.0
    # frozen orbitals on a file: one more core orbital and two virtuals dropped through the existing window calls
    res3, got3 = run_from_file(tmp_path / "c", tmp_path / "a" / "FCIDUMP", "CCSD_spatial", ",\nn_frozen_virt = 2")
    assert res3.returncode == 0, res3.stdout + res3.stderr
    assert "Number of frozen virtual orbitals: 2" in res3.stdout and got["ccsd_corr"] < got3["ccsd_corr"] < 0.0


def test_host_open_shell_from_the_file_it_wrote(tmp_path):
    res, got = run_host(tmp_path / "a", "h2o-cc-pvdz", "", ["n_frozen_core = 1", "fcidump_active = .true."], text=H2O_CATION_IN.format(calc="UCCSD"))
    assert res.returncode == 0, res.stdout + res.stderr
    res2, got2 = run_from_file(tmp_path / "b", tmp_path / "a" / "FCIDUMP", "UCCSD")
    assert res2.returncode == 0, res2.stdout + res2.stderr
    for key in ("ump2_corr", "uccsd_corr"):
        print(key, got[key], got2[key])
        assert abs((got["uhf_total"] + got[key]) - (got2["uhf_total"] + got2[key])) < 1e-8
    # a file of the other kind, and a refused combination, fail with their own messages
    res3, _ = run_from_file(tmp_path / "c", tmp_path / "a" / "FCIDUMP", "CCSD_spatial")
    assert res3.returncode != 0 and "UHF=.TRUE." in res3.stderr, res3.stderr
    res4, _ = run_from_file(tmp_path / "d", tmp_path / "a" / "FCIDUMP", "UCCSD", ",\nfcidump_active = .true.")
    assert res4.returncode != 0 and "would overwrite it" in res4.stderr, res4.stderr
    res5, _ = run_from_file(tmp_path / "e", None, "UCCSD")
    assert res5.returncode != 0 and "FCIDUMP is missing" in res5.stderr, res5.stderr
