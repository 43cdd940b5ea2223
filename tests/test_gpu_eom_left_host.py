"""The Fortran host with eom_nroots = 4 and eom_left = .true. on the bundled stretched H2O/cc-pVDZ input as CCSD_spinorb
(AFESP_SO_FOO_AS_PUBLISHED=1, as tests/test_gpu_eom_host.py): after the EOM-CCSD table it solves the left problem from the right vectors
and prints one table more; its omega_left are those of the Python driver (afesp_amd.eom.so_eom_left_solve) on the same input, they are
to equal the right-hand roots, and without the key the output is the one of before.

1e-8: the parity bar of the host tests for two separately converged solves (SCF to 1e-12, CCSD to 1e-11, Davidson residuals to 1e-8);
1e-7 between a left and a right root, each converged to a residual of 1e-8.

The case is the one that made the left state follow its guesses.  As measured on an MI355X:
    right, both drivers   0.0380938897  0.0380938897  0.0380938897  0.1753927658     21 steps,  77 sigma builds
    left, els_amd         0.0380938896  0.0380938897  0.0380938898  0.1753927656     17 steps,  62 sigma builds
    left, Python driver   0.0380938897  0.0380938897  0.0380938897  0.1753927656               113 sigma builds
The four unit guesses of the right-hand solve are the four spin components of the orbital pair 4 -> 5, so it finds that pair's triplet
and singlet and stays in their spatial symmetry: A has lower roots of other symmetries (0.0474; a triplet at 0.0836) that it never
sees.  Nothing but rounding couples the symmetries, yet a Davidson iteration amplifies such a component step by step -- the converged
right vectors already carry 1e-10 of it.  Taking the lowest roots, the Python driver's left solve, which runs longer than the host's
(its amplitudes differ in the last bits, and the residuals hover at tol = 1e-8 around step 17), returned 0.0473754307 as its fourth
root after 65 steps: a true eigenvalue of A^T, lower than the singlet, and not the state asked for.  Following the Ritz values of the
guess step, both drivers return the partners of the right vectors.  The number of steps of the two left solves differs (rounding
decides when the last residual passes 1e-8), so their sigma-build counts are not compared."""
import dataclasses
import re

import numpy as np

import molecules
import pytest
from afesp_amd import eom, rhf
from test_gpu_eom_host import ROW, _input_text, _untimed
from test_gpu_frozen_host import run_host

pytestmark = pytest.mark.gpu

LEFT_ROW = re.compile(r"^\s+(\d+)\s+(-?\d+\.\d{12})\s+(-?\d+\.\d{10})\s+(\d\.\d{3}E[-+]\d+)\s+(\d\.\d{3}E[-+]\d+)\s*$", re.M)
LEFT_HEAD = " Left eigenvectors: Davidson steps:"


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the Python driver and the host with and without the key, once"""
    from afesp_amd.capi import Engine
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("AFESP_SO_FOO_AS_PUBLISHED", "1")
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
            omega, R, info = eom.so_eom_solve(eng, 4)
            omega_left, L, linfo = eom.so_eom_left_solve(eng, R)
        L = eom.biorthonormalise(omega_left, L, R)                          # the triplet's three components: one cluster
        overlap = np.array([[eom.dot(l, r) for r in R] for l in L])
        print("python driver:\n" + eom.table(omega, info) + "\n" + eom.left_table(omega_left, omega, linfo))
        tmp = tmp_path_factory.mktemp("eom_left_host")
        host, _ = run_host(tmp / "a", "h2o-cc-pvdz", "", ["eom_nroots = 4", "eom_left = .true."], text=_input_text())
        plain, _ = run_host(tmp / "b", "h2o-cc-pvdz", "", ["eom_nroots = 4"], text=_input_text())
        refused, _ = run_host(tmp / "c", "h2o-cc-pvdz", "", ["eom_left = .true."], text=_input_text())
    assert host.returncode == 0, host.stdout + host.stderr
    out = host.stdout
    assert out.index("\n EOM-CCSD\n ----------") < out.index(LEFT_HEAD) < out.index("Time taken for EOM-CCSD:")
    block = out[out.index(LEFT_HEAD):out.index("Time taken for EOM-CCSD:")]
    print(block)
    rows = [(int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5))) for m in LEFT_ROW.finditer(block)]
    right = np.array([float(m.group(2)) for m in ROW.finditer(out[out.index("\n EOM-CCSD\n ----------"):out.index(LEFT_HEAD)])])
    return dict(omega=omega, omega_left=omega_left, linfo=linfo, overlap=overlap, out=out, block=block, rows=rows, right=right, plain=plain, refused=refused)


def test_host_prints_the_left_roots_of_the_python_driver(runs):
    rows, omega_left = runs["rows"], runs["omega_left"]
    assert [r[0] for r in rows] == [1, 2, 3, 4], runs["block"]
    got = np.array([r[1] for r in rows])
    print("host", got, "python driver", omega_left)
    assert np.max(np.abs(got - omega_left)) < 1e-8
    assert np.max(np.abs(np.array([r[2] for r in rows]) - omega_left * eom.HARTREE_EV)) < 1e-6
    head = re.match(r" Left eigenvectors: Davidson steps: (\d+), sigma builds: (\d+)$", runs["block"].splitlines()[0])
    assert all(r[4] < 1e-8 for r in rows) and head and int(head.group(1)) >= 1 and int(head.group(2)) >= 4      # (at least the four guesses)
    assert runs["right"].shape == (4,) and np.max(np.abs(runs["right"] - runs["omega"])) < 1e-8
    assert np.max(np.abs(np.array([r[3] for r in rows]) - np.abs(got - runs["right"]))) < 2e-12      # the column is what it says


def test_left_roots_equal_the_right_roots(runs):
    got = np.array([r[1] for r in runs["rows"]])
    print("left", got, "right", runs["right"], "difference", np.abs(got - runs["right"]))
    assert np.max(np.abs(got - runs["right"])) < 1e-7 and all(r[3] < 1e-7 for r in runs["rows"])
    assert np.max(np.abs(runs["omega_left"] - runs["omega"])) < 1e-7
    print("<L_j, R_k> after biorthonormalise", runs["overlap"])
    assert np.max(np.abs(runs["overlap"] - np.eye(4))) < 1e-6             # (|rho| / gap of two solves at tol = 1e-8: the same four states)


def test_without_the_key_the_output_is_the_one_of_before(runs):
    """the same lines once the left block and the timings are taken out"""
    out, plain = runs["out"], runs["plain"]
    assert plain.returncode == 0 and "Left eigenvectors" not in plain.stdout and "omega left" not in plain.stdout
    cut = out[:out.index(LEFT_HEAD)] + out[out.index("Time taken for EOM-CCSD:"):]
    a, b = _untimed(cut), _untimed(plain.stdout)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty), (x, y)
        for p, q in zip(tx, ty):
            if p != q:
                assert abs(float(p) - float(q)) < 1e-8, (x, y)


def test_host_refuses_eom_left_without_roots(runs):
    host = runs["refused"]
    assert host.returncode != 0 and "eom_left needs eom_nroots > 0" in host.stdout + host.stderr
