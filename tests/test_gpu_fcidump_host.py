"""The Fortran host with fcidump_active = .true.: the FCIDUMP els_amd leaves behind, read back as a Hamiltonian (afesp_amd/fcidump.py),
against the energies the same run printed.  1e-8: the F15.10 printout level of the other host tests (the SCF of these inputs is converged
far below it)."""
import pytest

from afesp_amd import fcidump
from test_gpu_frozen_host import run_host
from test_uhf_cpu import H2O_CATION_IN

pytestmark = pytest.mark.gpu
H2O_IN = ('&elsinput\ncalc_type="{calc}",\nscf_e_tol=1e-12,\nscf_d_tol=1e-10,\nscf_diis_n_errmat=6,\nccsd_e_tol=1e-8,\nccsd_t_tol=1e-8,\n'
          'ccsd_diis_n_errmat=8,\nscf_maxiter=200,\nccsd_maxiter=50{more}\n/\n')


def test_host_frozen_core_dump_is_the_hamiltonian_of_the_run(tmp_path):
    res, got = run_host(tmp_path, "h2o-cc-pvdz", "", ["frozen_core = .true.", "fcidump_active = .true."],
                        text=H2O_IN.format(calc="MP2_spatial", more=""))
    assert res.returncode == 0, res.stdout + res.stderr
    assert "FCIDUMP: NORB 23, NELEC 8, lines " in res.stdout and "Number of frozen core orbitals: 1" in res.stdout
    rec = fcidump.read(tmp_path / "FCIDUMP")
    assert (rec.norb, rec.nelec, rec.ms2, rec.uhf) == (23, 8, 0, False)
    assert f"lines {rec.nlines}," in res.stdout
    print(fcidump.hf_energy(rec), got["rhf_total"], fcidump.mp2_energy(rec), got["mp2_corr"])
    assert abs(fcidump.hf_energy(rec) - got["rhf_total"]) < 1e-8
    assert abs(fcidump.mp2_energy(rec) - got["mp2_corr"]) < 1e-8


def test_host_open_shell_dump_is_the_hamiltonian_of_the_run(tmp_path):
    res, got = run_host(tmp_path, "h2o-cc-pvdz", "", ["frozen_core = .true.", "fcidump_active = .true."],
                        text=H2O_CATION_IN.format(calc="UCCSD"))
    assert res.returncode == 0, res.stdout + res.stderr
    assert "FCIDUMP: NORB 46, NELEC 7, lines " in res.stdout
    rec = fcidump.read(tmp_path / "FCIDUMP")
    assert (rec.norb, rec.nelec, rec.ms2, rec.uhf) == (46, 7, 1, True)
    print(fcidump.hf_energy(rec), got["uhf_total"], fcidump.mp2_energy(rec), got["ump2_corr"], got["uccsd_corr"])
    assert abs(fcidump.hf_energy(rec) - got["uhf_total"]) < 1e-8
    assert abs(fcidump.mp2_energy(rec) - got["ump2_corr"]) < 1e-8
    assert got["uccsd_corr"] < got["ump2_corr"] < 0.0          # (the solver ran on after the dump)


def test_host_refuses_both_dump_keys(tmp_path):
    res, _ = run_host(tmp_path, "h2o-cc-pvdz", "", [], text=H2O_IN.format(
        calc="MP2_spatial", more=",\nwrite_fcidump = .true.,\nfcidump_active = .true."))
    assert res.returncode != 0 and "both write FCIDUMP" in res.stderr, res.stderr
    assert not (tmp_path / "FCIDUMP").exists()
