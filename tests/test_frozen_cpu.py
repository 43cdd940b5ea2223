"""Frozen core / frozen virtuals, host side: the numpy restatement of the orbital window (np_window) pinned on the CPU oracle,
the three new input keys, and the core count."""
import os

import numpy as np
import pytest

import molecules
import np_ucc
import np_window
import orc
from afesp_amd import inputs


def test_window_of_the_whole_basis_is_the_identity():
    si, ints, res, _ = molecules.load("n2-cc-pvdz")
    n = ints.nbasis
    eri_mo = orc.ao2mo(n, res.canon_coeff, ints.eri)
    assert np.array_equal(np_window.window_packed(n, 0, 0, eri_mo), eri_mo)
    assert np.array_equal(np_window.window_levels(n, 0, 0, res.canon_levels), res.canon_levels)


@pytest.mark.parametrize("n,nfc,nfv", [(5, 1, 0), (7, 2, 1), (9, 0, 3)])
def test_packed_window_is_the_window_of_the_full_array(n, nfc, nfv):
    """packed -> packed against slicing the full n^4 array and packing again (np_ucc.pack8); the pair matrix likewise."""
    rng = np.random.default_rng(n)
    packed = rng.standard_normal(inputs.neri(n))
    full = np_ucc.unpack_eri(n, packed)
    assert np.array_equal(np_window.window_packed(n, nfc, nfv, packed), np_ucc.pack8(np_window.window_full(nfc, nfv, full)))
    g = rng.standard_normal((n, n, n, n))
    g = g + g.transpose(1, 0, 2, 3)
    g = g + g.transpose(0, 1, 3, 2)          # (pq|rs) symmetric within each pair only: an alpha-beta block
    assert np.array_equal(np_window.window_pair_matrix(n, nfc, nfv, np_ucc.pair_matrix(g)),
                          np_ucc.pair_matrix(np_window.window_full(nfc, nfv, g)))


def test_decoupled_orbitals_full_run_equals_windowed_run_on_the_oracle():
    """Every packed integral that touches orbital 0 or orbital n - 1 set to zero: those two orbitals then carry no amplitude, and the
    full oracle run equals the run on the window [1, n - 1) -- MP2, every CCSD iteration, [T]/(T) and the D sums.  An invariant
    that needs no re-packing code to be right by construction: it fails if the window picks the wrong elements or levels."""
    o, v = 4, 7
    n, e, eri = molecules.synthetic_system(o, v, scale=0.05)
    eri = np_window.decouple(n, eri, [0, n - 1])
    win = np_window.window_packed(n, 1, 1, eri)
    ew = np_window.window_levels(n, 1, 1, e)
    assert abs(orc.mp2_energy(n, o, eri, e) - orc.mp2_energy(n - 2, o - 1, win, ew)) <= 1e-13
    full, act = orc.OracleCC(o, v, eri, e, 8), orc.OracleCC(o - 1, v - 1, win, ew, 8)
    nit, en, rm = full.solve(50, 1e-9, 1e-9)
    wnit, wen, wrm = act.solve(50, 1e-9, 1e-9)
    assert nit == wnit > 0
    assert np.max(np.abs(en[:nit + 1] - wen[:nit + 1])) <= 1e-13 and np.max(np.abs(rm[:nit + 1] - wrm[:nit + 1])) <= 1e-13
    assert np.max(np.abs(full.t1[1:, :-1] - act.t1)) <= 1e-13 and np.max(np.abs(full.t2[1:, 1:, :-1, :-1] - act.t2)) <= 1e-13
    assert np.max(np.abs(full.t1[0])) == 0.0 and np.max(np.abs(full.t2[..., -1])) == 0.0
    assert np.max(np.abs(full.triples(e) - act.triples(ew))) <= 1e-13


def _els_in(tmp_path, body):
    p = tmp_path / "els.in"
    p.write_text("&elsinput\n" + body + "\n/\n")
    return str(p)


def test_namelist_frozen_orbital_keys(tmp_path):
    si = inputs.read_els_in(_els_in(tmp_path, 'calc_type="CCSD(T)_spatial"'))
    assert (si.frozen_core, si.n_frozen_core, si.n_frozen_virt) == (False, -1, 0)
    assert inputs.frozen_window(si, [7, 7]) == (0, 0)
    for name in ("h2o-cc-pvdz", "n2-cc-pvdz", "f2-cc-pvdz"):      # the bundled inputs: every orbital correlated, as before
        old = inputs.read_els_in(os.path.join(molecules.GOLDEN, name, "els.in"))
        assert (old.frozen_core, old.n_frozen_core, old.n_frozen_virt) == (False, -1, 0)
    si = inputs.read_els_in(_els_in(tmp_path, 'calc_type="RCCSD(T)_spatial",\nfrozen_core=.true.,\nn_frozen_virt=3'))
    assert (si.frozen_core, si.n_frozen_core, si.n_frozen_virt) == (True, -1, 3)
    assert inputs.frozen_window(si, [9, 9]) == (2, 3)
    si = inputs.read_els_in(_els_in(tmp_path, 'calc_type="UCCSD(T)",\ncharge=1,\nmultiplicity=2,\nfrozen_core=.true.,\nn_frozen_core=0'))
    assert inputs.frozen_window(si, [8, 1, 1]) == (0, 0)          # the explicit count wins
    si = inputs.read_els_in(_els_in(tmp_path, 'calc_type="CCSD_spinorb",\nn_frozen_core=2,\nn_frozen_virt=-1'))
    assert inputs.frozen_window(si, [7, 7]) == (2, 0)             # -1: not given
    for bad in ("n_frozen_core=-2", "n_frozen_virt=-3", "n_frozen_core=1.5", "n_frozen_virt=2.0", "n_frozen_core=.true.",
                'frozen_core="yes"', "frozen_core=1"):
        with pytest.raises(ValueError):
            inputs.read_els_in(_els_in(tmp_path, 'calc_type="CCSD(T)_spatial",\n' + bad))


@pytest.mark.parametrize("name,count", [("h2o-cc-pvdz", 1), ("n2-cc-pvdz", 2), ("f2-cc-pvdz", 2)])
def test_frozen_core_count_of_the_bundled_geometries(name, count):
    z = inputs.read_nuclear_charges(os.path.join(molecules.GOLDEN, name, "geom.dat"))
    assert sum(z) == molecules.load(name)[1].nel
    assert inputs.frozen_core_count(z) == count


def test_frozen_core_count_rule():
    assert [inputs.frozen_core_count([z]) for z in (1, 2, 3, 10, 11, 18, 19, 36)] == [0, 0, 1, 1, 5, 5, 9, 9]
    assert inputs.frozen_core_count([6, 1, 1, 1, 17]) == 6
    with pytest.raises(ValueError):
        inputs.frozen_core_count([8, 37])
