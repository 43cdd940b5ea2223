"""The Fortran host with cc_density = .true. on H2O+/cc-pVDZ (the open-shell case of the other host tests), UCCSD from its own UHF and
ROHF-CCSD from a restricted doublet FCIDUMP: the Lambda table is printed, the natural occupation numbers are those of the Python path
(Engine.so_lambda_* / afesp_amd.density) and sum to the electron count; without the key the output is the one of before.

1e-8: the parity bar of the host tests for two separately converged solves printed at ten digits."""
import dataclasses
import re

import numpy as np
import pytest

import molecules
from afesp_amd import density, fcidump, inputs, rohf, uhf
from test_gpu_fcidump_in_host import run_from_file
from test_gpu_frozen_host import run_host
from test_gpu_rohf_host import cation_file  # noqa: F401  (fixture)
from test_uhf_cpu import H2O_CATION_IN

pytestmark = pytest.mark.gpu
TIGHT = ",\nccsd_e_tol=1e-11,\nccsd_t_tol=1e-11"
CATION = H2O_CATION_IN.replace("ccsd_e_tol=1e-10", "ccsd_e_tol=1e-11").replace("ccsd_t_tol=1e-10", "ccsd_t_tol=1e-11")


def _occupations(out):
    """the printed natural occupation numbers and their printed sum"""
    assert "CCSD Lambda" in out and "delta RMS L2" in out and "L = T" in out
    block = out[out.index("Natural occupation numbers"):]
    lines = block.splitlines()
    occ = []
    for k, line in enumerate(lines[1:], 1):
        if line.strip().startswith("Sum of natural occupation numbers:"):
            return np.array(occ), float(line.split(":")[1])
        occ += [float(x) for x in line.split()]
    raise AssertionError("no sum line")


def _lambda_rows(out):
    """(iteration, pseudo energy, rms) of the Lambda table"""
    tab = out[out.index("delta RMS L2"):out.index("Natural occupation numbers")]
    return [(int(m.group(1)), float(m.group(2)), float(m.group(4)))
            for m in re.finditer(r"^\s+(\d+)\s+(-?\d+\.\d+)\s+(-?\d+\.\d+)\s+(-?\d+\.\d+)\s+\d+\.\d+\s*$", tab, re.M)]


def _python_occupations(eng, n, na, nb, beta_in_alpha):
    lit, pes, rms = density.so_lambda_solve(eng, 300, 1e-11, 1e-11)
    da, db = density.spatial_blocks(eng.so_density(), n, na, nb, False)
    return density.natural_occupations(da, db, beta_in_alpha), lit, pes


def _check(out, occ_ref, nel, pes):
    occ, total = _occupations(out)
    rows = _lambda_rows(out)
    print("Lambda iterations", len(rows), "occupations", occ[:6], "sum", total)
    assert len(rows) >= 2 and [r[0] for r in rows] == list(range(1, len(rows) + 1))
    assert abs(rows[-1][1] - pes[-1]) < 1e-8                         # the converged pseudo energy
    assert occ.size == occ_ref.size and np.all(np.diff(occ) <= 0.0)
    assert np.max(np.abs(occ - occ_ref)) < 1e-8
    assert abs(total - nel) < 1e-8 and abs(np.sum(occ) - nel) < 1e-8
    assert out.index("Final") < out.index("CCSD Lambda")              # after CCSD ...
    if "\n CCSD(T)\n ----------" in out:                               # (the section header of the triples)
        assert out.index("CCSD Lambda") < out.index("\n CCSD(T)\n ----------")      # ... and before (T)


def test_host_uccsd_prints_the_natural_occupations_of_the_python_path(tmp_path):
    from afesp_amd.capi import Engine
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, charge=1, multiplicity=2, scf_maxiter=200, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_read_guess=False)
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    u = uhf.do_uhf(si, ints, na, nb)
    assert u.converged
    with Engine(0) as eng:
        eng.do_ump2(n, na, nb, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, ints.eri, want_eri_mo=False)
        eng.init_cc_uspinorb(n, na, nb, u.levels_a, u.levels_b, 8)
        nit, _, _ = eng.do_ccsd_spinorb(300, 1e-11, 1e-11)
        assert nit > 0
        occ_ref, _, pes = _python_occupations(eng, n, na, nb, u.coeff_b @ ints.ovlp @ u.coeff_a.T)
    res, got = run_host(tmp_path / "a", "h2o-cc-pvdz", "", ["cc_density = .true."], text=CATION.format(calc="UCCSD(T)"))
    assert res.returncode == 0, res.stdout + res.stderr
    _check(res.stdout, occ_ref, na + nb, pes)
    # without the key: the output of before -- the same lines once the Lambda block and the timings are taken out
    plain, got0 = run_host(tmp_path / "b", "h2o-cc-pvdz", "", [], text=CATION.format(calc="UCCSD(T)"))
    assert plain.returncode == 0 and "Lambda" not in plain.stdout and "Natural occupation" not in plain.stdout
    out = res.stdout
    cut = out[:out.index(" ----------\n CCSD Lambda")] + out[out.index("Time taken for CCSD Lambda and density:"):].split("\n", 1)[1]

    def untimed(text):
        text = re.sub(r"(Time taken[^:]*:|Total execution time:)\s+\S+(\s*s\b)?", r"\1", text)
        return [re.sub(r"\s+\d*\.\d{6}\s*$", "", line) for line in text.splitlines()]
    a, b = untimed(cut), untimed(plain.stdout)
    assert len(a) == len(b)
    for x, y in zip(a, b):                                             # line for line: the same words, the same numbers (two runs: 1e-8)
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty), (x, y)
        for p, q in zip(tx, ty):
            if p != q:
                assert abs(float(p) - float(q)) < 1e-8, (x, y)
    assert abs(got["uccsd_pt_corr"] - got0["uccsd_pt_corr"]) < 1e-9


def test_host_rohf_ccsd_prints_the_natural_occupations_of_the_python_path(tmp_path, cation_file):  # noqa: F811
    from afesp_amd.capi import Engine
    with Engine(0) as eng:
        ref = rohf.rohf_cc(eng, cation_file, 300, 1e-11, 1e-11)
        fa, fb, _ = eng.mo_fock_ro(ref.nbasis, ref.nalpha, ref.nbeta, fcidump.read(cation_file).h)
        ua, ub, _, _ = rohf.semicanonical(fa, fb, ref.nalpha, ref.nbeta)     # (the rotations rohf_cc made: beta orbitals in the alpha ones)
        occ_ref, _, pes = _python_occupations(eng, ref.nbasis, ref.nalpha, ref.nbeta, ub @ ua.T)
    res, _ = run_from_file(tmp_path / "a", cation_file, "ROHF-CCSD", TIGHT + ",\ncc_density = .true.")
    assert res.returncode == 0, res.stdout + res.stderr
    _check(res.stdout, occ_ref, ref.nalpha + ref.nbeta, pes)


def test_host_reports_the_library_error_on_an_unpublished_spinorb_state(tmp_path):
    import os
    import shutil
    import subprocess
    from test_gpu_frozen_host import EXE
    src = os.path.join(molecules.GOLDEN, "h2o-cc-pvdz")
    for f in ("s.dat", "t.dat", "v.dat", "eri.dat", "geom.dat"):
        shutil.copy(os.path.join(src, f), tmp_path)
    text = open(os.path.join(src, "els.in")).read().replace("CRCCSD(T)_spatial", "CCSD_spinorb").rstrip()[:-1].rstrip().rstrip(",")
    (tmp_path / "els.in").write_text(text + ",\ncc_density = .true.\n/\n")
    env = {k: v for k, v in os.environ.items() if k != "AFESP_SO_FOO_AS_PUBLISHED"}
    res = subprocess.run([EXE], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode != 0 and "transposed F_mi" in res.stderr, res.stderr
    res = subprocess.run([EXE], cwd=tmp_path, env={**env, "AFESP_SO_FOO_AS_PUBLISHED": "1"}, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    occ, total = _occupations(res.stdout)
    assert abs(total - 10.0) < 1e-8 and occ.size == 24
