"""The Fortran host with the frozen-natural-orbital keys (fno_n_virt, fno_occ_tol): what els_amd prints against Engine.fno_window /
Engine.ufno_window plus the Python drivers on the same input.  Every printed energy to 1e-8 (the parity bound of the host output, which
is printed to that many digits), the kept count identical, each input conflict with its message, and -- with the keys absent -- the
printout the frozen-orbital host tests already expect, without a word about natural orbitals."""
import re

import pytest

import molecules
from afesp_amd import inputs, uhf
from test_gpu_frozen_host import _oracle_rccsd_t, run_host
from test_uhf_cpu import H2O_CATION_IN

pytestmark = pytest.mark.gpu

FNO_LINES = {
    "kept": r"Number of natural virtuals kept:\s+(\d+)",
    "full": r"MP2 correlation energy, all virtuals \(Hartree\):\s+(-?\d+\.\d+)",
    "fno": r"MP2 correlation energy, natural virtuals \(Hartree\):\s+(-?\d+\.\d+)",
    "delta": r"Delta MP2 \(Hartree\):\s+(-?\d+\.\d+)",
    "delta_table": r"Delta MP2 \(full - FNO space\):\s+(-?\d+\.\d+)",
    "ccsd_plus": r"CCSD \+ Delta MP2 correlation:\s+(-?\d+\.\d+)",
    "final_plus": r"Final \+ Delta MP2 correlation:\s+(-?\d+\.\d+)",
    "occ_kept": r"Smallest kept occupation:\s+(\S+)",
    "occ_dropped": r"Largest discarded occupation:\s+(\S+)",
}


def _fno_lines(stdout):
    out = {}
    for k, pat in FNO_LINES.items():
        m = re.search(pat, stdout)
        if m:
            out[k] = int(m.group(1)) if k == "kept" else float(m.group(1))
    return out


def _python_closed_shell(tmp_path, name, spinorb):
    from afesp_amd.capi import Engine
    si = inputs.read_els_in(str(tmp_path / "els.in"))
    _, ints, res, _ = molecules.load(name)
    n, o = ints.nbasis, ints.nel // 2
    nfc, _ = inputs.frozen_window(si, inputs.read_nuclear_charges(str(tmp_path / "geom.dat")))
    inputs.check_fno_count(si, n - o)
    with Engine(0) as eng:
        kept, occ, lev, e_fno, delta = eng.fno_window(n, o, nfc, res.canon_coeff, res.canon_levels, ints.eri,
                                                      n_keep=si.fno_n_virt if si.fno_n_virt >= 0 else None, occ_tol=si.fno_occ_tol)
        _, e_full = None, e_fno + delta
        if spinorb:
            eng.init_cc_spinorb(o - nfc + kept, ints.nel - 2 * nfc, lev, None, si.ccsd_diis_n_errmat)
            nit, en, _ = eng.do_ccsd_spinorb(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
            assert nit > 0
            ec = en[nit]
            e_pt = ec + eng.do_ccsd_t_spinorb()
            table = dict(mp2_corr=e_fno, ccsd_corr=ec, ccsd_pt_corr=e_pt)
        else:
            eng.ccsd_init(o - nfc, kept, lev, None, si.ccsd_diis_n_errmat)
            nit, en, _ = eng.do_ccsd_spatial(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
            assert nit > 0
            ec = en[nit]
            t = eng.do_ccsd_t_spatial()
            e_pt = ec + t[1]
            table = dict(mp2_corr=e_fno, ccsd_corr=ec, ccsd_bt_corr=ec + t[0], ccsd_pt_corr=e_pt)
    lines = dict(kept=kept, full=e_full, fno=e_fno, delta=delta, delta_table=delta, ccsd_plus=ec + delta, final_plus=e_pt + delta,
                 occ_kept=occ[kept - 1], occ_dropped=occ[kept])
    return table, lines


def _compare(res, got, table, lines):
    found = _fno_lines(res.stdout)
    print(found, lines, {k: got.get(k) for k in table}, table)
    assert found["kept"] == lines["kept"]
    for k, v in lines.items():
        if k == "kept":
            continue
        tol = 1e-8 if not k.startswith("occ") else 2e-8 * abs(v)   # (ES15.8: nine significant digits)
        assert abs(found[k] - v) < tol, (k, found[k], v)
    for k, v in table.items():
        assert abs(got[k] - v) < 1e-8, (k, got[k], v)


@pytest.mark.parametrize("name,keys", [("h2o-cc-pvdz", ["fno_n_virt = 13", "frozen_core = .true."]), ("f2-cc-pvdz", ["fno_n_virt = 10"]),
                                       ("n2-cc-pvdz", ["fno_n_virt = 12"]),
                                       ("h2o-cc-pvdz", ["fno_occ_tol = 5.0d-4"])])
def test_host_fno_ccsd_t_spatial_matches_the_python_path(tmp_path, name, keys):
    """H2O, F2 with a count; N2 with a count that splits a pi pair (both sides widen it to 13); H2O with a threshold"""
    res, got = run_host(tmp_path, name, "CCSD(T)_spatial", keys)
    assert res.returncode == 0, res.stdout + res.stderr
    table, lines = _python_closed_shell(tmp_path, name, False)
    _compare(res, got, table, lines)
    if name == "n2-cc-pvdz":
        assert lines["kept"] == 13 and "asked for 12" in res.stdout


def test_host_fno_spin_orbital_ccsd_t_matches_the_python_path(tmp_path):
    res, got = run_host(tmp_path, "h2o-cc-pvdz", "CCSD(T)_spinorb", ["fno_n_virt = 13", "n_frozen_core = 1"])
    assert res.returncode == 0, res.stdout + res.stderr
    table, lines = _python_closed_shell(tmp_path, "h2o-cc-pvdz", True)
    _compare(res, got, table, lines)


def test_host_fno_uccsd_t_cation_matches_the_python_path(tmp_path):
    from afesp_amd.capi import Engine
    res, got = run_host(tmp_path, "h2o-cc-pvdz", "UCCSD(T)", ["fno_n_virt = 11", "frozen_core = .true."],
                        text=H2O_CATION_IN.format(calc="UCCSD(T)"))
    assert res.returncode == 0, res.stdout + res.stderr
    si = inputs.read_els_in(str(tmp_path / "els.in"))
    _, ints, _, _ = molecules.load("h2o-cc-pvdz")
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    nfc, _ = inputs.frozen_window(si, inputs.read_nuclear_charges(str(tmp_path / "geom.dat")))
    inputs.check_fno_count(si, n - max(na, nb))
    u = uhf.do_uhf(si, ints, na, nb)
    assert u.converged
    with Engine(0) as eng:
        kept, (occ_a, _), (la, lb), e_fno, delta = eng.ufno_window(n, na, nb, nfc, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, ints.eri,
                                                                   n_keep=si.fno_n_virt)
        eng.init_cc_uspinorb(len(la), na - nfc, nb - nfc, la, lb, si.ccsd_diis_n_errmat)
        nit, en, _ = eng.do_ccsd_spinorb(si.ccsd_maxiter, si.ccsd_e_tol, si.ccsd_t_tol)
        assert nit > 0
        e_pt = en[nit] + eng.do_ccsd_t_spinorb()
    table = dict(uhf_total=u.e_hf + ints.e_nuc, ump2_corr=e_fno, uccsd_corr=en[nit], uccsd_pt_corr=e_pt)
    lines = dict(kept=kept, full=e_fno + delta, fno=e_fno, delta=delta, delta_table=delta, ccsd_plus=en[nit] + delta,
                 final_plus=e_pt + delta, occ_kept=occ_a[kept - 1], occ_dropped=occ_a[kept])
    _compare(res, got, table, lines)


def test_host_fno_two_ranks_give_the_same_numbers(tmp_path):
    """rank mode: every rank builds the same orbitals from the same D; the (T) shards add up to the one-rank value"""
    from test_gpu_frozen_host import MGPU
    keys = ["fno_n_virt = 13", "n_frozen_core = 2"]
    res1, got1 = run_host(tmp_path / "one", "n2-cc-pvdz", "CCSD(T)_spatial", keys)
    res2, got2 = run_host(tmp_path / "two", "n2-cc-pvdz", "CCSD(T)_spatial", keys, argv=[MGPU, "2", "host"])
    assert res1.returncode == 0 and res2.returncode == 0, res1.stderr + res2.stderr
    assert "Ranks: 2, transport host" in res2.stdout
    a, b = _fno_lines(res1.stdout), _fno_lines(res2.stdout)
    assert a["kept"] == b["kept"] == 13
    for k in ("full", "fno", "delta", "ccsd_plus", "final_plus"):
        assert abs(a[k] - b[k]) < 1e-9, (k, a[k], b[k])
    assert got2["ccsd_corr"] == got1["ccsd_corr"] and abs(got2["ccsd_pt_corr"] - got1["ccsd_pt_corr"]) < 1e-9


@pytest.mark.parametrize("keys,word", [(["fno_n_virt = 10", "fno_occ_tol = 1.0d-4"], "exclude each other"),
                                       (["fno_n_virt = 10", "n_frozen_virt = 2"], "n_frozen_virt exclude each other"),
                                       (["fno_occ_tol = 1.0d-4", "n_frozen_virt = 1"], "n_frozen_virt exclude each other"),
                                       (["fno_n_virt = 0"], "leaves no active virtual orbital"),
                                       (["fno_n_virt = 22"], "exceeds the number of virtual orbitals"),
                                       (["fno_n_virt = -4"], "non-negative"),
                                       (["fno_occ_tol = 0.9"], "leaves no natural virtual")])
def test_host_refuses_conflicting_fno_keys(tmp_path, keys, word):
    res, _ = run_host(tmp_path, "n2-cc-pvdz", "CCSD(T)_spatial", keys)
    assert res.returncode != 0 and word in res.stderr, res.stderr


def test_host_without_the_keys_prints_what_it_printed_before(tmp_path):
    """no FNO key: the frozen-core run of test_gpu_frozen_host.py, its lines and its table, and no line about natural orbitals"""
    res, got = run_host(tmp_path, "n2-cc-pvdz", "RCCSD(T)_spatial", ["n_frozen_core = 2"])
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Number of frozen core orbitals: 2" in res.stdout and "Number of frozen virtual orbitals: 0" in res.stdout
    assert "Number of occupied orbitals: 7" in res.stdout and "Number of virtual orbitals: 21" in res.stdout
    for word in ("natural", "Delta MP2", "occupation"):
        assert word not in res.stdout, word
    ref, nit = _oracle_rccsd_t("n2-cc-pvdz", 2, 0)
    assert [r[0] for r in got["cc_iters"]] == list(range(nit + 1))
    for k, v in ref.items():
        assert abs(got[k] - v) < 1e-8, (k, got[k], v)
    res0, _ = run_host(tmp_path / "plain", "h2o-cc-pvdz", "CCSD(T)_spatial", [])
    assert res0.returncode == 0 and "natural" not in res0.stdout and "Delta MP2" not in res0.stdout and "frozen" not in res0.stdout
