"""The Fortran host on a restricted open-shell FCIDUMP: els_amd with ROHF-CCSD(T) in a directory that holds nothing but els.in and the file
prints the energies of afesp_amd.rohf.rohf_cc (1e-9: two separately converged solves at e_tol = t_tol = 1e-11), and the refusals keep
their messages."""
import re

import numpy as np
import pytest

import molecules
import np_ucc
from afesp_amd import fcidump, rohf
from afesp_amd.rhf import unpack_eri
from test_gpu_fcidump_in_host import run_from_file

pytestmark = pytest.mark.gpu
TIGHT = ",\nccsd_e_tol=1e-11,\nccsd_t_tol=1e-11"      # (the namelist takes the last value of a key given twice)


@pytest.fixture(scope="module")
def cation_file(tmp_path_factory):
    """H2O+ (5, 4) on the neutral molecule's RHF orbitals as a restricted doublet FCIDUMP (MS2 = 1, no UHF flag)"""
    _, ints, res, _ = molecules.load("h2o-cc-pvdz")
    n, C = ints.nbasis, res.canon_coeff
    full = np.einsum("pi,qj,rk,sl,ijkl->pqrs", C, C, C, C, unpack_eri(n, ints.eri), optimize=True)
    path = tmp_path_factory.mktemp("rohf") / "FCIDUMP"
    fcidump.write(path, C @ ints.core_hamil @ C.T, np_ucc.pack8(full), 9, 1, 9.1)
    return path


def _printed(text, label):
    m = re.search(re.escape(label) + r"\s+(-?\d+\.\d+)", text)
    assert m, label
    return float(m.group(1))


def test_host_rohf_ccsd_t_prints_the_energies_of_rohf_cc(tmp_path, cation_file):
    from afesp_amd.capi import Engine
    with Engine(0) as eng:
        ref = rohf.rohf_cc(eng, cation_file, 200, 1e-11, 1e-11)
    res, _ = run_from_file(tmp_path / "a", cation_file, "ROHF-CCSD(T)", TIGHT)
    assert res.returncode == 0, res.stdout + res.stderr
    out = res.stdout
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["FCIDUMP", "els.in", "els.out"]
    for label in ("Largest occupied-occupied off-diagonal Fock element:", "Largest virtual-virtual off-diagonal Fock element:",
                  "Largest occupied-virtual Fock element:", "Convergence reached within tolerance."):
        assert label in out, label
    got = dict(e_ref=_printed(out, "Reference determinant energy (Hartree):"),
               e_mp2=_printed(out, "ROHF-MBPT(2) correlation energy (Hartree):"),
               e_ccsd=_printed(out, "Final ROHF-CCSD Energy (Hartree):"),
               e_pt=_printed(out, "ROHF-CCSD(T) correlation energy (Hartree):"))
    want = dict(e_ref=ref.e_ref, e_mp2=ref.e_mp2, e_ccsd=ref.e_ccsd, e_pt=ref.e_ccsd + ref.e_t)
    for k in got:
        print(k, got[k], want[k])
        assert abs(got[k] - want[k]) < 1e-9, k
    # the final table carries the same numbers at its own ten digits
    assert abs(_printed(out, "ROHF-CCSD(T) energy:") - (ref.e_ref + ref.e_ccsd + ref.e_t)) < 1e-9


def test_host_rohf_refusals(tmp_path, cation_file):
    # no ROHF SCF: the types need the file
    (tmp_path / "a").mkdir()
    text = '&elsinput\ncalc_type="ROHF-CCSD",\nccsd_maxiter=5\n/\n'
    (tmp_path / "a" / "els.in").write_text(text)
    import subprocess
    from test_gpu_frozen_host import EXE
    res = subprocess.run([EXE], cwd=tmp_path / "a", capture_output=True, text=True, timeout=600)
    assert res.returncode != 0 and "ROHF-CCSD needs fcidump_in = .true." in res.stderr, res.stderr
    for i, (more, msg) in enumerate(((",\nn_frozen_core = 1", "takes no frozen_core"), (",\nn_frozen_virt = 2", "takes no frozen_core"),
                                     (",\nfno_n_virt = 5", "takes no frozen natural orbitals"))):
        res, _ = run_from_file(tmp_path / f"b{i}", cation_file, "ROHF-CCSD", more)
        assert res.returncode != 0 and msg in res.stderr, res.stderr
    # the existing types on the restricted open-shell file: today's messages, word for word
    res, _ = run_from_file(tmp_path / "c", cation_file, "UCCSD")
    assert res.returncode != 0 and "fcidump_in: a closed-shell file takes the _spatial and _spinorb types, not UCCSD" in res.stderr, res.stderr
    res, _ = run_from_file(tmp_path / "d", cation_file, "CCSD_spinorb")
    assert res.returncode != 0, res.stderr
    assert "fcidump_in: an open shell without UHF=.TRUE. (restricted open-shell orbitals are not supported)" in res.stderr, res.stderr
