"""The Fortran host with cc_polar on the bundled H2O/cc-pVDZ input as CCSD_spinorb (AFESP_SO_FOO_AS_PUBLISHED=1, as every Lambda-state
property): the polarisability table is printed after CCSD and Lambda and equals afesp_amd.response.polarizability on the same inputs.
The three operator files are copies of t.dat, v.dat and t.dat: the program reads no dipole integrals, and any symmetric one-body
operator in the AO basis exercises the same path (the numbers are then response functions of T and V_ne, not a polarisability).

Bound: the printed digits -- one unit of the tenth decimal the table prints, between two runs of the same deterministic device code on
inputs that differ by the two SCF programs (converged to 1e-12)."""
import dataclasses
import os
import re
import shutil

import numpy as np

import molecules
import np_eom_left
import pytest
from afesp_amd import density, response, rhf
from test_gpu_eom_host import _input_text
from test_gpu_frozen_host import run_host

pytestmark = pytest.mark.gpu

ROW = re.compile(r"^\s+([xyz])\s+(-?\d+\.\d{10})\s*(-?\d+\.\d{10})\s*(-?\d+\.\d{10})\s*$", re.M)
OPERATOR_FILES = {"dipx.dat": "t.dat", "dipy.dat": "v.dat", "dipz.dat": "t.dat"}


def _with_operator_files(tmp_path, leave_out=()):
    tmp_path.mkdir(exist_ok=True)
    for dst, src in OPERATOR_FILES.items():
        if dst not in leave_out:
            shutil.copy(os.path.join(molecules.GOLDEN, "h2o-cc-pvdz", src), tmp_path / dst)


def test_host_prints_the_polarisability_of_the_python_driver(tmp_path, monkeypatch):
    from afesp_amd.capi import Engine
    monkeypatch.setenv("AFESP_SO_FOO_AS_PUBLISHED", "1")
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_maxiter=200, scf_read_guess=False)
    res = rhf.do_rhf(si, ints, None)
    n, nel = ints.nbasis, ints.nel
    omegas = [0.0, 0.05]
    ca = res.canon_coeff
    orb, spin = density.so_spin_order(n, nel // 2, nel // 2, True)
    ao = {"t.dat": ints.ke, "v.dat": ints.ele_nuc}
    ops = []
    for dst in ("dipx.dat", "dipy.dat", "dipz.dat"):
        m = ca @ ao[OPERATOR_FILES[dst]] @ ca.T
        m = 0.5 * (m + m.T)
        ops.append(np_eom_left.so_matrix(m, m, orb, spin))
    with Engine(0) as eng:
        eng.do_mp2_spatial(n, nel // 2, res.canon_coeff, res.canon_levels, ints.eri)
        eng.init_cc_spinorb(n, nel, res.canon_levels, None, 8, foo_as_published=True)
        nit, _, _ = eng.do_ccsd_spinorb(100, 1e-11, 1e-11)
        assert nit > 0
        density.so_lambda_solve(eng, 100, 1e-11, 1e-11, diis_nerr=8)
        alpha, iso, aniso, info = response.polarizability(eng, ops, omegas)
    print("python driver:\n" + response.table(omegas, alpha, iso, aniso, info))
    _with_operator_files(tmp_path / "a")
    host, _ = run_host(tmp_path / "a", "h2o-cc-pvdz", "", ["cc_polar = .true.", "polar_omega = 0.0, 0.05"], text=_input_text())
    assert host.returncode == 0, host.stdout + host.stderr
    out = host.stdout
    assert out.index("Final CCSD Energy") < out.index("\n EOM-CCSD polarisability\n ----------") < out.index("CCSD Lambda") < out.index("omega =")
    block = out[out.index("\n EOM-CCSD polarisability\n ----------"):out.index("Time taken for the EOM-CCSD polarisability:")]
    print(block)
    rows = ROW.findall(block)
    assert [r[0] for r in rows] == list("xyzxyz"), block
    got = np.array([[float(x) for x in r[1:]] for r in rows]).reshape(2, 3, 3)
    print("largest difference between the host's table and the Python driver:", np.max(np.abs(got - alpha)))
    assert np.max(np.abs(got - alpha)) <= 1.0e-10
    means = [float(x) for x in re.findall(r"mean\s+(-?\d+\.\d{10})", block)]
    anisos = [float(x) for x in re.findall(r"anisotropy\s+(-?\d+\.\d{10})", block)]
    assert np.max(np.abs(np.array(means) - iso)) <= 1.0e-10 and np.max(np.abs(np.array(anisos) - aniso)) <= 1.0e-10
    assert f"response sigma builds: {info['nsigma']}" in block
    assert float(re.search(r"largest residual:\s+(\S+)", block).group(1)) < 1e-8
    assert out.count("CCSD Lambda") == 1                                     # one Lambda solve


def test_a_missing_operator_file_is_an_input_error_naming_it(tmp_path):
    _with_operator_files(tmp_path, leave_out=("dipz.dat",))
    host, _ = run_host(tmp_path, "h2o-cc-pvdz", "", ["cc_polar = .true."], text=_input_text())
    assert host.returncode != 0
    assert "dipz.dat" in host.stderr and "does not exist" in host.stderr
    assert "Final CCSD Energy" not in host.stdout                            # it stopped before any work
