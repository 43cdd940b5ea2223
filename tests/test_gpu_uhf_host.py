"""The Fortran host on an open-shell input: els_amd with calc_type UCCSD(T), charge 1, multiplicity 2 on the H2O/cc-pVDZ files
prints what the Python path (numpy UHF, then the engine's UMP2 / UCCSD / (T)) computes; two host-transport ranks on one GPU give
the same (T)."""
import os

import pytest

import molecules
from afesp_amd import inputs, uhf
from test_uhf_cpu import HOST_EXE, run_host_case

pytestmark = pytest.mark.gpu
MGPU = os.path.join(os.path.dirname(HOST_EXE), "els_mgpu.sh")


def _python_path(tmp_path):
    from afesp_amd.capi import Engine
    si = inputs.read_els_in(str(tmp_path / "els.in"))
    _, ints, _, _ = molecules.load("h2o-cc-pvdz")
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    u = uhf.do_uhf(si, ints, na, nb)
    assert u.converged
    with Engine(0) as eng:
        e2, *_ = eng.do_ump2(n, na, nb, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, ints.eri, want_eri_mo=False)
        eng.init_cc_uspinorb(n, na, nb, u.levels_a, u.levels_b, si.ccsd_diis_n_errmat)
        nit, en, _ = eng.do_ccsd_spinorb(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
        assert nit > 0
        e_t = eng.do_ccsd_t_spinorb()
    return dict(uhf_total=u.e_hf + ints.e_nuc, s2=u.s2, ump2_corr=e2, uccsd_corr=en[nit], uccsd_pt_corr=en[nit] + e_t)


def test_host_uccsd_t_cation_matches_the_python_path(tmp_path):
    res, got = run_host_case(tmp_path, "UCCSD(T)")
    assert res.returncode == 0, res.stdout + res.stderr
    ref = _python_path(tmp_path)
    for k, v in ref.items():
        assert abs(got[k] - v) < 1e-9, (k, got[k], v)
    assert abs(got["total"] - ref["uccsd_pt_corr"] - (got["uhf_total"])) < 1e-9


def test_host_uccsd_t_cation_two_ranks_give_the_same_triples(tmp_path):
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir(); two.mkdir()
    res1, got1 = run_host_case(one, "UCCSD(T)")
    assert res1.returncode == 0, res1.stdout + res1.stderr
    res2, got2 = run_host_case(two, "UCCSD(T)", argv=[MGPU, "2", "host"])
    assert res2.returncode == 0, res2.stdout + res2.stderr
    assert "Ranks: 2, transport host" in res2.stdout
    assert abs(got2["uccsd_pt_corr"] - got1["uccsd_pt_corr"]) < 1e-11
    assert abs(got2["uccsd_corr"] - got1["uccsd_corr"]) < 1e-12
