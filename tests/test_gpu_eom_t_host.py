"""The Fortran host with eom_nroots = 4, eom_left and eom_triples on the bundled stretched H2O/cc-pVDZ input as CCSD_spinorb
(AFESP_SO_FOO_AS_PUBLISHED=1, as tests/test_gpu_eom_left_host.py: o, v = 10, 38, 120 triples): after the left table it biorthonormalises,
calls the library once for all roots and prints root, omega, delta omega, omega + delta omega.  The delta omega are those of the Python
path (afesp_amd.eom.so_eom_triples_correction) on the same input, which in turn is the numpy evaluation at the fetched vectors; two ranks
add up to one rank's values; without eom_left the key is refused.

1e-9 between the two drivers: the correction is bilinear in vectors that two separately converged Davidson solves (residuals 1e-8)
deliver, and it is of the order 1e-3 Eh here.  The three components of the triplet are mixed differently by the two drivers: what is
compared is the root's delta omega, which is the same for every component."""
import dataclasses
import re

import numpy as np
import pytest

import molecules
import np_eom_t as ET
import np_triples as T
import orc
from afesp_amd import eom, rhf
from afesp_amd.rhf import unpack_eri
from test_gpu_eom_host import _input_text
from test_gpu_frozen_host import MGPU, run_host

pytestmark = pytest.mark.gpu

HEAD = " Non-iterative triples correction to the EOM-CCSD excitation energies"
T_ROW = re.compile(r"^\s+(\d+)\s+(-?\d+\.\d{12})\s+(-?\d+\.\d{12})\s+(-?\d+\.\d{12})\s+(-?\d+\.\d{10})\s*$", re.M)
KEYS = ["eom_nroots = 4", "eom_left = .true.", "eom_triples = .true."]


def _rows(out):
    assert out.index(" Left eigenvectors: Davidson steps:") < out.index(HEAD) < out.index("Time taken for EOM-CCSD:")
    block = out[out.index(HEAD):out.index("Time taken for EOM-CCSD:")]
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
        with Engine(0) as eng:
            eng.do_mp2_spatial(n, nel // 2, res.canon_coeff, res.canon_levels, ints.eri)
            eng.init_cc_spinorb(n, nel, res.canon_levels, None, 8, foo_as_published=True)
            nit, _, _ = eng.do_ccsd_spinorb(100, 1e-11, 1e-11)
            assert nit > 0 and (eng.so_o, eng.so_v) == (10, 38)
            eng.so_lambda_init(0)
            omega, R, _ = eom.so_eom_solve(eng, 4)
            omega_left, L, _ = eom.so_eom_left_solve(eng, R)
            L = eom.biorthonormalise(omega_left, L, R)
            delta, corrected, info = eom.so_eom_triples_correction(eng, omega, L, R)
            _, t2 = eng.so_amplitudes()
        print("python driver:\n" + eom.triples_table(omega, delta, info))
        # float64 numpy at the fetched vectors (120 triples per root: the products through BLAS)
        orb, spin = T.interleaved_order(n, nel)
        g = T.so_g(unpack_eri(n, orc.ao2mo(n, res.canon_coeff, ints.eri)), orb, spin)
        ref = [ET.eom_t_per_triple(g, res.canon_levels[orb], nel, t2, omega[k], *L[k], *R[k], dtype=np.float64) for k in range(4)]
        tmp = tmp_path_factory.mktemp("eom_t_host")
        one, _ = run_host(tmp / "a", "h2o-cc-pvdz", "", KEYS, text=_input_text())
        two, _ = run_host(tmp / "b", "h2o-cc-pvdz", "", KEYS, argv=[MGPU, "2", "host"], text=_input_text())
        refused, _ = run_host(tmp / "c", "h2o-cc-pvdz", "", ["eom_nroots = 4", "eom_triples = .true."], text=_input_text())
    return dict(omega=omega, delta=delta, corrected=corrected, info=info, ref=ref, one=one, two=two, refused=refused)


def test_python_path_equals_numpy_at_the_fetched_vectors(runs):
    """both sides in double precision: each within np_eom_t.tol_factor of the exact value, so within twice that of each other"""
    for k in range(4):
        val, S = runs["ref"][k]
        bound = 2 * ET.tol_factor(10, 38) * float(np.sum(S))
        print("root", k + 1, "omega", runs["omega"][k], "delta", runs["delta"][k], "numpy", float(np.sum(val)), "bound", bound)
        assert len(val) == 120 and abs(runs["delta"][k] - float(np.sum(val))) <= bound
    assert runs["info"]["intruder"] == [] and np.all(runs["info"]["min_gap"] > 0.05)


def test_host_prints_the_corrections_of_the_python_path(runs):
    host = runs["one"]
    assert host.returncode == 0, host.stdout + host.stderr
    rows, block = _rows(host.stdout)
    assert [r[0] for r in rows] == [1, 2, 3, 4], block
    got = np.array([r[2] for r in rows])
    print("host", got, "python driver", runs["delta"])
    assert np.max(np.abs(np.array([r[1] for r in rows]) - runs["omega"])) < 1e-8
    assert np.max(np.abs(got - runs["delta"])) < 1e-9
    for r in rows:
        assert abs(r[3] - (r[1] + r[2])) < 2e-12 and abs(r[4] - r[3] * eom.HARTREE_EV) < 1e-9
    assert "not reliable" not in block
    assert host.stdout.count(HEAD) == 1          # one call, one table: not one per root


def test_one_rank_and_two_ranks_agree(runs):
    two = runs["two"]
    assert two.returncode == 0, two.stdout + two.stderr
    assert "Ranks: 2, transport host" in two.stdout
    a, b = _rows(runs["one"].stdout)[0], _rows(two.stdout)[0]
    assert len(a) == len(b) == 4
    assert max(abs(x[2] - y[2]) for x, y in zip(a, b)) < 1e-9


def test_host_refuses_eom_triples_without_eom_left(runs):
    host = runs["refused"]
    assert host.returncode != 0 and "eom_triples needs eom_nroots > 0 and eom_left" in host.stdout + host.stderr
