"""The Fortran host with the frozen-orbital keys (frozen_core, n_frozen_core, n_frozen_virt): what els_amd prints against the CPU
restatements on the window that np_window cuts out of the MO integrals.  1e-8: the F15.10 printout level of the other host tests."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import molecules
import np_ucc
import np_window
import orc
from afesp_amd import inputs, uhf
from test_uhf_cpu import H2O_CATION_IN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "a-fortran-electronic-structure-program_amd", "host")
EXE, MGPU = os.path.join(HOST, "els_amd"), os.path.join(HOST, "els_mgpu.sh")
TABLE = ("rhf_total", "mp2_corr", "ccsd_corr", "ccsd_bt_corr", "ccsd_pt_corr", "r_ccsd_bt_corr", "r_ccsd_pt_corr", "d_bt", "d_pt",
         "t1_diag", "total")


def run_host(tmp_path, name, calc_type, keys, argv=None, text=None):
    """els_amd on the bundled files of `name` with calc_type and the extra namelist lines `keys`"""
    tmp_path.mkdir(exist_ok=True)
    src = os.path.join(molecules.GOLDEN, name)
    for f in ("s.dat", "t.dat", "v.dat", "eri.dat", "geom.dat", "guess_in.dat"):
        if os.path.exists(os.path.join(src, f)):
            shutil.copy(os.path.join(src, f), tmp_path)
    if text is None:
        text = open(os.path.join(src, "els.in")).read().replace("CRCCSD(T)_spatial", calc_type)
    assert "frozen" not in text and text.rstrip().endswith("/")
    text = text.rstrip()[:-1].rstrip().rstrip(",") + "".join(",\n" + k for k in keys) + "\n/\n"
    (tmp_path / "els.in").write_text(text)
    res = subprocess.run(argv or [EXE], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    (tmp_path / "els.out").write_text(res.stdout)
    return res, inputs.parse_els_out(str(tmp_path / "els.out"))


def _oracle_rccsd_t(name, nfc, nfv):
    si, ints, res, _ = molecules.load(name)
    n, o = ints.nbasis, ints.nel // 2
    oa, va = o - nfc, n - o - nfv
    ew = np_window.window_levels(n, nfc, nfv, res.canon_levels)
    win = np_window.window_packed(n, nfc, nfv, orc.ao2mo(n, res.canon_coeff, ints.eri))
    cc = orc.OracleCC(oa, va, win, ew, si.ccsd_diis_n_errmat)
    nit, en, _ = cc.solve(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    t = cc.triples(ew)
    ec = en[nit]
    return dict(mp2_corr=orc.mp2_energy(oa + va, oa, win, ew), ccsd_corr=ec, ccsd_bt_corr=ec + t[0], ccsd_pt_corr=ec + t[1],
                r_ccsd_bt_corr=ec + t[0] / t[2], r_ccsd_pt_corr=ec + t[1] / t[3], d_bt=t[2], d_pt=t[3],
                t1_diag=float(np.sqrt(np.sum(cc.t1 ** 2) / (ints.nel - 2 * nfc)))), nit


def test_host_frozen_core_rccsd_t_matches_the_oracle_on_the_window(tmp_path):
    res, got = run_host(tmp_path, "n2-cc-pvdz", "RCCSD(T)_spatial", ["n_frozen_core = 2"])
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Number of frozen core orbitals: 2" in res.stdout and "Number of frozen virtual orbitals: 0" in res.stdout
    assert "Number of occupied orbitals: 7" in res.stdout and "Number of virtual orbitals: 21" in res.stdout   # the full counts stay
    ref, nit = _oracle_rccsd_t("n2-cc-pvdz", 2, 0)
    assert [r[0] for r in got["cc_iters"]] == list(range(nit + 1))
    for k, v in ref.items():
        print(k, got[k], v)
        assert abs(got[k] - v) < 1e-8, (k, got[k], v)
    assert abs(got["mp2_line"] - ref["mp2_corr"]) < 1e-7          # the "MP2 correlation energy (Hartree):" line, F15.8
    assert abs(got["total"] - (got["rhf_total"] + ref["r_ccsd_pt_corr"])) < 2e-8


@pytest.mark.parametrize("name,count", [("n2-cc-pvdz", 2), ("h2o-cc-pvdz", 1)])
def test_host_frozen_core_switch_counts_the_cores(tmp_path, name, count):
    """frozen_core = .true. prints the table of n_frozen_core = <the counted cores>; an explicit count wins over the switch."""
    res_a, a = run_host(tmp_path / "a", name, "RCCSD(T)_spatial", ["frozen_core = .true."])
    res_b, b = run_host(tmp_path / "b", name, "RCCSD(T)_spatial", [f"n_frozen_core = {count}"])
    res_c, c = run_host(tmp_path / "c", name, "MP2_spatial", ["frozen_core = .true.", "n_frozen_core = 0"])
    assert res_a.returncode == 0 and res_b.returncode == 0 and res_c.returncode == 0, res_a.stderr + res_b.stderr + res_c.stderr
    assert f"Number of frozen core orbitals: {count}" in res_a.stdout
    for k in TABLE:
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["cc_iters"] == b["cc_iters"]
    assert abs(a["mp2_corr"] - molecules.SURVEY_GOLD[name]["mp2_corr"]) > 1e-4          # (not the all-electron number)
    assert "frozen" not in res_c.stdout and abs(c["mp2_corr"] - molecules.SURVEY_GOLD[name]["mp2_corr"]) < 1e-8


def test_host_frozen_virtuals_spin_orbital_ccsd_t_matches_the_oracle(tmp_path):
    nfv = 3
    res, got = run_host(tmp_path, "f2-cc-pvdz", "CCSD(T)_spinorb", [f"n_frozen_virt = {nfv}"])
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Number of frozen core orbitals: 0" in res.stdout and "Number of frozen virtual orbitals: 3" in res.stdout
    si, ints, rhf_res, _ = molecules.load("f2-cc-pvdz")
    n = ints.nbasis
    ew = np_window.window_levels(n, 0, nfv, rhf_res.canon_levels)
    win = np_window.window_packed(n, 0, nfv, orc.ao2mo(n, rhf_res.canon_coeff, ints.eri))
    so = orc.OracleSO(n - nfv, ints.nel, win, ew, si.ccsd_diis_n_errmat)
    nit, en, _ = so.solve(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
    assert [r[0] for r in got["cc_iters"] if r[0] > 0] == list(range(1, nit + 1))
    assert abs(got["mp2_corr"] - orc.mp2_energy(n - nfv, ints.nel // 2, win, ew)) < 1e-8
    assert abs(got["ccsd_corr"] - so.energy) < 1e-8
    assert abs(got["ccsd_pt_corr"] - (so.energy + so.triples())) < 1e-8


def _cation_reference(tmp_path, nfc, nfv):
    si = inputs.read_els_in(str(tmp_path / "els.in"))
    _, ints, _, _ = molecules.load("h2o-cc-pvdz")
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    assert inputs.frozen_window(si, inputs.read_nuclear_charges(str(tmp_path / "geom.dat"))) == (nfc, nfv)
    u = uhf.do_uhf(si, ints, na, nb)
    assert u.converged
    aa, ab, bb = (np_window.window_full(nfc, nfv, x) for x in np_ucc.mo_blocks(n, u.coeff_a, u.coeff_b, ints.eri))
    la, lb = u.levels_a[nfc:n - nfv], u.levels_b[nfc:n - nfv]
    cc = np_ucc.UCC(*np_ucc.so_integrals(aa, ab, bb, la, lb, na - nfc, nb - nfc))
    _, ec = cc.solve(300, 1e-12, 1e-12)
    return dict(uhf_total=u.e_hf + ints.e_nuc, ump2_corr=np_ucc.ump2(aa, ab, bb, la, lb, na - nfc, nb - nfc), uccsd_corr=ec,
                uccsd_pt_corr=ec + cc.triples())


def test_host_frozen_core_uccsd_t_cation_matches_numpy(tmp_path):
    res, got = run_host(tmp_path, "h2o-cc-pvdz", "UCCSD(T)", ["frozen_core = .true."], text=H2O_CATION_IN.format(calc="UCCSD(T)"))
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Number of frozen core orbitals: 1" in res.stdout
    ref = _cation_reference(tmp_path, 1, 0)
    for k, v in ref.items():
        print(k, got[k], v)
        assert abs(got[k] - v) < 1e-8, (k, got[k], v)


def test_host_frozen_core_two_ranks_give_the_same_triples(tmp_path):
    res1, got1 = run_host(tmp_path / "one", "n2-cc-pvdz", "RCCSD(T)_spatial", ["n_frozen_core = 2"])
    assert res1.returncode == 0, res1.stdout + res1.stderr
    res2, got2 = run_host(tmp_path / "two", "n2-cc-pvdz", "RCCSD(T)_spatial", ["n_frozen_core = 2"], argv=[MGPU, "2", "host"])
    assert res2.returncode == 0, res2.stdout + res2.stderr
    assert "Ranks: 2, transport host" in res2.stdout and "Number of frozen core orbitals: 2" in res2.stdout
    for k in ("ccsd_bt_corr", "ccsd_pt_corr", "r_ccsd_bt_corr", "r_ccsd_pt_corr", "d_bt", "d_pt"):
        assert abs(got2[k] - got1[k]) < 1e-10, (k, got2[k], got1[k])
    assert got2["ccsd_corr"] == got1["ccsd_corr"] and got2["mp2_corr"] == got1["mp2_corr"]


@pytest.mark.parametrize("keys,word", [(["n_frozen_core = 7"], "no active occupied orbital"),
                                       (["n_frozen_virt = 21"], "no active virtual orbital"),
                                       (["n_frozen_core = -3"], "non-negative")])
def test_host_refuses_a_window_without_active_orbitals(tmp_path, keys, word):
    res, _ = run_host(tmp_path, "n2-cc-pvdz", "RCCSD(T)_spatial", keys)
    assert res.returncode != 0 and word in res.stderr, res.stderr
