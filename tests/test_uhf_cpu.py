"""Open-shell path, host side: the numpy UHF, the dense spin-orbital restatement (np_ucc) and the new input keys."""
import dataclasses
import os

import numpy as np
import pytest

import molecules
import np_ucc
import orc
from afesp_amd import inputs, uhf


def _uhf(name, charge=0, mult=1, swap=False):
    si, ints, res, gold = molecules.load(name)
    if (charge, mult) != (0, 1):
        si = dataclasses.replace(si, charge=charge, multiplicity=mult, scf_maxiter=200, scf_e_tol=1e-12, scf_d_tol=1e-10)
    na, nb = inputs.spin_counts(si, ints.nel, ints.nbasis)
    if swap:
        na, nb = nb, na
    guess = inputs.read_scf_guess(os.path.join(molecules.GOLDEN, name, "guess_in.dat"), ints.nbasis) if si.scf_read_guess else None
    return ints, res, gold, na, nb, uhf.do_uhf(si, ints, na, nb, guess)


@pytest.mark.parametrize("name", ["h2o-cc-pvdz", "n2-cc-pvdz", "f2-cc-pvdz"])
def test_singlet_uhf_stays_on_the_rhf_solution(name):
    ints, res, gold, na, nb, u = _uhf(name)
    assert (na, nb) == (ints.nel // 2, ints.nel // 2)
    assert u.converged
    assert np.array_equal(u.coeff_a, u.coeff_b) and np.array_equal(u.levels_a, u.levels_b)
    ref = gold.get("rhf_total", molecules.SURVEY_GOLD[name]["rhf_total"])
    assert abs(u.e_hf + ints.e_nuc - ref) < 2e-9
    assert abs(u.s2) < 1e-10


def test_restatement_matches_the_spin_orbital_oracle_in_the_closed_shell_limit():
    """np_ucc on doubled RHF orbitals (blocked spin order) against the compiled spin-orbital oracle (interleaved order) with
    F_mi in Stanton's published order: CCSD and (T) at tight tolerances."""
    si, ints, res, _ = molecules.load("h2o-cc-pvdz")
    n, o = ints.nbasis, ints.nel // 2
    eri_mo = orc.ao2mo(n, res.canon_coeff, ints.eri)
    so = orc.OracleSO(n, ints.nel, eri_mo, res.canon_levels, 8, foo_as_published=True)
    nit, en, _ = so.solve(100, 1e-11, 1e-11)
    full = np_ucc.unpack_eri(n, eri_mo)
    cc = np_ucc.UCC(*np_ucc.so_integrals(full, full, full, res.canon_levels, res.canon_levels, o, o))
    _, e = cc.solve(100, 1e-11, 1e-11)
    assert abs(e - en[nit]) < 1e-10
    assert abs(cc.triples() - so.triples()) < 1e-10


def _h_mo(ints, C):
    return C @ ints.core_hamil @ C.T


@pytest.mark.parametrize("mult", [3, 1])
def test_two_electrons_uccsd_is_fci_and_triples_vanish(mult):
    ints, _, _, na, nb, u = _uhf("h2o-cc-pvdz", charge=8, mult=mult)
    assert (na, nb) == ((2, 0) if mult == 3 else (1, 1))
    assert u.converged
    n = ints.nbasis
    aa, ab, bb = np_ucc.mo_blocks(n, u.coeff_a, u.coeff_b, ints.eri)
    cc = np_ucc.UCC(*np_ucc.so_integrals(aa, ab, bb, u.levels_a, u.levels_b, na, nb))
    _, e = cc.solve(200, 1e-12, 1e-12)
    fci = np_ucc.fci_two_electron(n, aa, ab, _h_mo(ints, u.coeff_a), _h_mo(ints, u.coeff_b), mult == 3)
    assert abs(u.e_hf + e - fci) < 1e-10
    assert abs(cc.triples()) < 1e-12


def test_doublet_alpha_and_beta_excess_give_the_same_energies():
    out = []
    for swap in (False, True):
        ints, _, _, na, nb, u = _uhf("h2o-cc-pvdz", charge=1, mult=2, swap=swap)
        assert u.converged and (na, nb) == ((4, 5) if swap else (5, 4))
        aa, ab, bb = np_ucc.mo_blocks(ints.nbasis, u.coeff_a, u.coeff_b, ints.eri)
        e2 = np_ucc.ump2(aa, ab, bb, u.levels_a, u.levels_b, na, nb)
        cc = np_ucc.UCC(*np_ucc.so_integrals(aa, ab, bb, u.levels_a, u.levels_b, na, nb))
        _, ec = cc.solve(200, 1e-12, 1e-12)
        out.append((u.e_hf, e2, ec, u.s2))
    assert np.max(np.abs(np.subtract(*out))) < 1e-10
    assert 0.75 < out[0][3] < 0.77          # a doublet with little contamination


def _els_in(tmp_path, body):
    p = tmp_path / "els.in"
    p.write_text("&elsinput\n" + body + "\n/\n")
    return str(p)


def test_read_els_in_open_shell_keys(tmp_path):
    si = inputs.read_els_in(_els_in(tmp_path, 'calc_type="UCCSD(T)",\ncharge=1,\nmultiplicity=2'))
    assert (si.calc_type, si.level, si.restricted, si.charge, si.multiplicity) == ("UCCSD(T)", "UCCSD(T)", False, 1, 2)
    assert inputs.spin_counts(si, 10, 24) == (5, 4)
    for t in ("UHF_scf", "UMP2", "UCCSD"):
        assert inputs.read_els_in(_els_in(tmp_path, f'calc_type="{t}"')).level == t.replace("_scf", "")
    for name in ("h2o-cc-pvdz", "n2-cc-pvdz", "f2-cc-pvdz"):
        old = inputs.read_els_in(os.path.join(molecules.GOLDEN, name, "els.in"))
        assert (old.charge, old.multiplicity) == (0, 1)
    uhf_old = inputs.read_els_in(_els_in(tmp_path, 'calc_type="UHF"'))
    assert (uhf_old.level, uhf_old.restricted) == ("RHF", False)


def test_read_els_in_rejects_bad_charge_and_multiplicity(tmp_path):
    si = inputs.read_els_in(_els_in(tmp_path, 'calc_type="UHF_scf",\ncharge=0,\nmultiplicity=2'))
    with pytest.raises(ValueError):
        inputs.spin_counts(si, 10, 24)          # 10 electrons cannot form a doublet
    with pytest.raises(ValueError):
        inputs.spin_counts(inputs.read_els_in(_els_in(tmp_path, 'calc_type="UMP2",\ncharge=11')), 10, 24)
    for t in ("UHF", "CCSD(T)_spinorb", "CCSD(T)_spatial", "RHF"):
        with pytest.raises(ValueError):
            inputs.read_els_in(_els_in(tmp_path, f'calc_type="{t}",\ncharge=1'))
        with pytest.raises(ValueError):
            inputs.read_els_in(_els_in(tmp_path, f'calc_type="{t}",\nmultiplicity=3'))
    with pytest.raises(ValueError):
        inputs.read_els_in(_els_in(tmp_path, 'calc_type="UCCSD",\nmultiplicity=0'))


HOST_EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "a-fortran-electronic-structure-program_amd",
                        "host", "els_amd")
H2O_CATION_IN = ('&elsinput\ncalc_type="{calc}",\ncharge=1,\nmultiplicity=2,\nscf_e_tol=1e-11,\nscf_d_tol=1e-9,\n'
                 'scf_diis_n_errmat=6,\nccsd_e_tol=1e-10,\nccsd_t_tol=1e-10,\nccsd_diis_n_errmat=8,\nscf_maxiter=200,\n'
                 'ccsd_maxiter=200\n/\n')


def run_host_case(tmp_path, calc, env=None, argv=None):
    """els_amd on the H2O/cc-pVDZ files with the cation input -> (CompletedProcess, parsed final table)"""
    import shutil
    import subprocess
    src = os.path.join(molecules.GOLDEN, "h2o-cc-pvdz")
    for f in ("s.dat", "t.dat", "v.dat", "eri.dat", "geom.dat"):
        shutil.copy(os.path.join(src, f), tmp_path)
    (tmp_path / "els.in").write_text(H2O_CATION_IN.format(calc=calc))
    res = subprocess.run(argv or [HOST_EXE], cwd=tmp_path, env={**os.environ, **(env or {})}, capture_output=True, text=True,
                         timeout=600)
    (tmp_path / "els.out").write_text(res.stdout)
    return res, inputs.parse_els_out(str(tmp_path / "els.out"))


def test_fortran_host_uhf_scf_on_cpu(tmp_path):
    res, got = run_host_case(tmp_path, "UHF_scf")
    assert res.returncode == 0, res.stderr
    si = inputs.read_els_in(str(tmp_path / "els.in"))
    _, ints, _, _ = molecules.load("h2o-cc-pvdz")
    u = uhf.do_uhf(si, ints, *inputs.spin_counts(si, ints.nel, ints.nbasis))
    assert u.converged
    assert abs(got["uhf_total"] - (u.e_hf + ints.e_nuc)) < 1e-9
    assert abs(got["s2"] - u.s2) < 1e-9
    assert abs(got["total"] - (u.e_hf + ints.e_nuc)) < 1e-9


def test_fortran_host_rejects_charge_on_a_closed_shell_type(tmp_path):
    res, _ = run_host_case(tmp_path, "CCSD(T)_spinorb")
    assert res.returncode != 0 and "open-shell" in res.stderr
