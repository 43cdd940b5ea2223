"""The Fortran host with cc_rdm2 = .true. on the bundled H2O/cc-pVDZ files: the closed-shell molecule through CCSD_spinorb and the H2O+
doublet of the other host tests through UCCSD from its own UHF.  After the Lambda table it prints the density-side correlation energy,
its difference to E(CCSD), and <S^2> of the reference determinant and of CCSD; without the key the output is the one of before.

Bounds: the density-side energy agrees with the printed E(CCSD) to the run's ccsd_e_tol; <S^2> of a closed shell is 0 within 1e-8 (every
operator of the functional is a singlet: exact at any convergence); the reference line of the doublet is the UHF determinant's own
Ms (Ms + 1) + nbeta - sum |<b|a>|^2 from this test's UHF, 1e-8 being the parity bar of the host tests for two separately converged solves."""
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import molecules
from afesp_amd import density, inputs, uhf
from test_gpu_frozen_host import EXE, run_host
from test_uhf_cpu import H2O_CATION_IN

pytestmark = pytest.mark.gpu


def _number(out, label):
    m = re.search(re.escape(label) + r"\s+(\S+)", out)
    assert m, label
    return float(m.group(1))


def _report(out):
    """(density-side energy, printed difference, <S^2> reference, <S^2> CCSD, printed E(CCSD)) with the order of the sections checked"""
    assert out.index("Final") < out.index("CCSD Lambda") < out.index("delta RMS L2") < out.index("Density-side CCSD correlation energy")
    e_cc = float(re.search(r"Final \S*CCSD Energy \(Hartree\):\s+(\S+)", out).group(1))
    return (_number(out, "Density-side CCSD correlation energy (Hartree):"), _number(out, "Difference to E(CCSD) (Hartree):"),
            _number(out, "<S^2> of the reference determinant:"), _number(out, "<S^2> of CCSD (unrelaxed two-particle density):"), e_cc)


def _untimed(text):
    text = re.sub(r"(Time taken[^:]*:|Total execution time:)\s+\S+(\s*s\b)?", r"\1", text)
    return [re.sub(r"\s+\d*\.\d{6}\s*$", "", line) for line in text.splitlines()]


def _same_but_for(out, plain):
    """`out` without its Lambda / two-particle-density block is `plain`, line for line (two runs: numbers to 1e-8)"""
    cut = out[:out.index(" ----------\n CCSD Lambda")] + out[out.index("Time taken for the CCSD two-particle density:"):].split("\n", 1)[1]
    a, b = _untimed(cut), _untimed(plain)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty), (x, y)
        for p, q in zip(tx, ty):
            if p != q:
                assert abs(float(p) - float(q)) < 1e-8, (x, y)


def test_host_closed_shell_spinorb_prints_the_density_side_energy_and_a_singlet(tmp_path):
    src = os.path.join(molecules.GOLDEN, "h2o-cc-pvdz")
    text = open(os.path.join(src, "els.in")).read().replace("CRCCSD(T)_spatial", "CCSD_spinorb").rstrip()[:-1].rstrip().rstrip(",")
    env = {**os.environ, "AFESP_SO_FOO_AS_PUBLISHED": "1"}
    runs = {}
    for tag, key in (("with", ",\ncc_rdm2 = .true."), ("without", "")):
        d = tmp_path / tag
        d.mkdir()
        for f in ("s.dat", "t.dat", "v.dat", "eri.dat", "geom.dat"):
            shutil.copy(os.path.join(src, f), d)
        (d / "els.in").write_text(text + key + "\n/\n")
        runs[tag] = subprocess.run([EXE], cwd=d, env=env, capture_output=True, text=True, timeout=600)
        assert runs[tag].returncode == 0, runs[tag].stdout + runs[tag].stderr
    out, plain = runs["with"].stdout, runs["without"].stdout
    e_d, diff, s2_ref, s2, e_cc = _report(out)
    tol = inputs.read_els_in(str(tmp_path / "with" / "els.in")).ccsd_e_tol
    print("E(CCSD)", e_cc, "density side", e_d, "printed difference", diff, "<S^2>", s2_ref, s2, "ccsd_e_tol", tol)
    assert abs(e_d - e_cc) < tol and abs(diff) < tol
    assert abs(s2_ref) < 1e-8 and abs(s2) < 1e-8
    assert "CCSD Lambda" not in plain and "Density-side" not in plain and "<S^2> of" not in plain
    _same_but_for(out, plain)


def test_host_uccsd_doublet_prints_the_determinants_own_s_squared(tmp_path):
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, charge=1, multiplicity=2, scf_maxiter=200, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_read_guess=False)
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    u = uhf.do_uhf(si, ints, na, nb)
    assert u.converged
    m = u.coeff_b @ ints.ovlp @ u.coeff_a.T                               # <beta orbital b | alpha orbital a>
    ref = 0.75 + nb - float(np.sum(m[:nb, :na] ** 2))
    assert abs(density.s_squared_reference(n, na, nb, False, m) - ref) < 1e-12
    res, got = run_host(tmp_path / "a", "h2o-cc-pvdz", "", ["cc_rdm2 = .true."], text=H2O_CATION_IN.format(calc="UCCSD"))
    assert res.returncode == 0, res.stdout + res.stderr
    e_d, diff, s2_ref, s2, e_cc = _report(res.stdout)
    tol = inputs.read_els_in(str(tmp_path / "a" / "els.in")).ccsd_e_tol
    print("E(UCCSD)", e_cc, "density side", e_d, "printed difference", diff, "ccsd_e_tol", tol)
    print("<S^2> UHF determinant", ref, "printed", s2_ref, "CCSD", s2)
    assert abs(e_d - e_cc) < tol and abs(diff) < tol
    assert abs(s2_ref - ref) < 1e-8
    assert abs(s2 - 0.75) < abs(s2_ref - 0.75) + 1e-8                      # no more contaminated than the UHF determinant
    plain, _ = run_host(tmp_path / "b", "h2o-cc-pvdz", "", [], text=H2O_CATION_IN.format(calc="UCCSD"))
    assert plain.returncode == 0
    assert "CCSD Lambda" not in plain.stdout and "Density-side" not in plain.stdout and "<S^2> of" not in plain.stdout
    # (the UHF section's own six-digit <S^2> line, there with and without the key, is the determinant's value too)
    assert abs(float(re.search(r"<S\^2>:\s+(\S+)", plain.stdout).group(1)) - ref) < 1e-6
    _same_but_for(res.stdout, plain.stdout)
