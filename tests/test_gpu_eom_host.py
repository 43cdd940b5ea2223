"""The Fortran host with eom_nroots = 4 on the bundled H2O/cc-pVDZ input as CCSD_spinorb (AFESP_SO_FOO_AS_PUBLISHED=1: the EOM equations need
the consistent residual, as Lambda does): the EOM-CCSD table is printed after CCSD, its excitation energies are those of the Python
driver (afesp_amd.eom) on the same input, the lowest triplet appears threefold, and without the key the output is the one of before.

1e-8: the parity bar of the host tests for two separately converged solves (SCF to 1e-12, CCSD to 1e-11, Davidson residuals to 1e-8).
No external EOM-CCSD value for this geometry is at hand: the test compares the two drivers, not a literature number."""
import dataclasses
import os
import re

import numpy as np

import molecules
import pytest
from afesp_amd import eom, rhf
from test_gpu_frozen_host import run_host

pytestmark = pytest.mark.gpu

ROW = re.compile(r"^\s+(\d+)\s+(-?\d+\.\d{12})\s+(-?\d+\.\d{10})\s+(\d\.\d{8})\s+(\d\.\d{3}E[-+]\d+)\s*$", re.M)


def _input_text():
    text = open(os.path.join(molecules.GOLDEN, "h2o-cc-pvdz", "els.in")).read()
    for old, new in (("CRCCSD(T)_spatial", "CCSD_spinorb"), ("scf_e_tol=1e-6", "scf_e_tol=1e-12"), ("scf_d_tol=1e-7", "scf_d_tol=1e-10"),
                     ("ccsd_e_tol=1e-6", "ccsd_e_tol=1e-11"), ("ccsd_t_tol=1e-7", "ccsd_t_tol=1e-11"), ("scf_maxiter = 50", "scf_maxiter = 200"),
                     ("ccsd_maxiter = 50", "ccsd_maxiter = 100"), ("scf_write_guess = .true.", "scf_write_guess = .false.")):
        assert old in text, old
        text = text.replace(old, new)
    return text


def _untimed(text):
    text = re.sub(r"(Time taken[^:]*:|Total execution time:)\s+\S+(\s*s\b)?", r"\1", text)
    return [re.sub(r"\s+\d*\.\d{6}\s*$", "", line) for line in text.splitlines()]


def test_host_prints_the_excitation_energies_of_the_python_driver(tmp_path, monkeypatch):
    from afesp_amd.capi import Engine
    monkeypatch.setenv("AFESP_SO_FOO_AS_PUBLISHED", "1")
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_maxiter=200, scf_read_guess=False)
    res = rhf.do_rhf(si, ints, None)
    n, nel = ints.nbasis, ints.nel
    with Engine(0) as eng:
        eng.do_mp2_spatial(n, nel // 2, res.canon_coeff, res.canon_levels, ints.eri)
        eng.init_cc_spinorb(n, nel, res.canon_levels, None, 8, foo_as_published=True)
        nit, _, _ = eng.do_ccsd_spinorb(100, 1e-11, 1e-11)
        assert nit > 0
        eng.so_lambda_init(0)
        omega, vectors, info = eom.so_eom_solve(eng, 4)
    print("python driver:\n" + eom.table(omega, info), "\ndegeneracy", info["degeneracy"])
    host, _ = run_host(tmp_path / "a", "h2o-cc-pvdz", "", ["eom_nroots = 4"], text=_input_text())
    assert host.returncode == 0, host.stdout + host.stderr
    out = host.stdout
    assert out.index("Final CCSD Energy") < out.index("\n EOM-CCSD\n ----------")
    block = out[out.index("\n EOM-CCSD\n ----------"):out.index("Time taken for EOM-CCSD:")]
    print(block)
    rows = [(int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5))) for m in ROW.finditer(block)]
    assert [r[0] for r in rows] == [1, 2, 3, 4], block
    got = np.array([r[1] for r in rows])
    assert np.max(np.abs(got - omega)) < 1e-8
    assert np.max(np.abs(np.array([r[2] for r in rows]) - omega * eom.HARTREE_EV)) < 1e-6
    assert all(r[4] < 1e-8 for r in rows) and f"sigma builds: {info['nsigma']}" in block
    # the lowest excited state of water is a triplet: three roots at one energy (Ms = 0, +1, -1), then a singlet; the weights of the
    # singles are those of the Python driver root by root only where the root is not degenerate
    assert np.max(np.abs(got[:3] - got[0])) < 1e-6 and got[3] - got[0] > 1e-3
    assert list(info["degeneracy"]) == [3, 3, 3, 1]
    # (<x, x> = sum x1^2 + 1/4 sum x2^2 = 1 bounds the weight by 1; how far below it lies is the molecule's business -- the bundled
    # geometry is a stretched one, r(OH) = 3.40 bohr, and the singlet carries 0.79)
    assert abs(rows[3][3] - info["r1_norm2"][3]) < 1e-6 and all(0.0 < r[3] <= 1.0 + 1e-8 for r in rows)
    # without the key: the output of before -- the same lines once the EOM block and the timings are taken out
    plain, _ = run_host(tmp_path / "b", "h2o-cc-pvdz", "", [], text=_input_text())
    assert plain.returncode == 0 and "EOM" not in plain.stdout
    cut = out[:out.index(" ----------\n EOM-CCSD")] + out[out.index("Time taken for EOM-CCSD:"):].split("\n", 1)[1]
    a, b = _untimed(cut), _untimed(plain.stdout)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty), (x, y)
        for p, q in zip(tx, ty):
            if p != q:
                assert abs(float(p) - float(q)) < 1e-8, (x, y)


def test_host_runs_eom_after_lambda_when_cc_density_is_set(tmp_path, monkeypatch):
    monkeypatch.setenv("AFESP_SO_FOO_AS_PUBLISHED", "1")
    host, _ = run_host(tmp_path, "h2o-cc-pvdz", "", ["eom_nroots = 2", "cc_density = .true."], text=_input_text())
    assert host.returncode == 0, host.stdout + host.stderr
    out = host.stdout
    assert out.index("CCSD Lambda") < out.index("Natural occupation numbers") < out.index("\n EOM-CCSD\n ----------")
    rows = ROW.findall(out[out.index("\n EOM-CCSD\n ----------"):])
    assert len(rows) == 2 and abs(float(rows[0][1]) - float(rows[1][1])) < 1e-6      # two components of the lowest triplet
