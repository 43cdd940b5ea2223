"""The Fortran host with eom_ip_nroots = 4 and eom_ea_nroots = 4 on the bundled H2O/cc-pVDZ input as CCSD_spinorb (AFESP_SO_FOO_AS_PUBLISHED=1,
as tests/test_gpu_eom_host.py): one table per sector is printed after CCSD, the ionisation potentials and electron affinities are those
of the Python driver (afesp_amd.eom) on the same input, every doublet of the closed-shell reference appears twofold, the sectors run
after Lambda and EOM-EE where those are asked for, and without the keys the output is the one of before.

1e-8: the parity bar of the host tests for two separately converged solves.  No external IP / EA value for this geometry is at hand: the
test compares the two drivers, not a literature number.

The bundled geometry is a stretched one (r(OH) = 3.40 bohr) whose lowest ionised doublet, 0.381184 Eh, is a hole in orbital 3 of 5 (level
-0.5083) -- below the holes in orbitals 5 and 4 (0.461008 and 0.491073 Eh; levels -0.4385, -0.4498), on which the four guesses sit, and in
another irreducible representation.  The guesses' admixture of every unique amplitude is what lets both drivers find it; with bare unit
vectors it entered only as rounding noise, in one driver and not in the other."""
import dataclasses
import re

import numpy as np

import molecules
import pytest
from afesp_amd import eom, rhf
from test_gpu_eom_host import _input_text, _untimed
from test_gpu_frozen_host import run_host

pytestmark = pytest.mark.gpu

# a row of a sector's table; the two components of a doublet may come out of the projected matrix as a pair with an imaginary part at
# rounding level, which the host marks
ROW = re.compile(r"^\s+(\d+)\s+(-?\d+\.\d{12})\s+(-?\d+\.\d{10})\s+(\d\.\d{8})\s+(\d\.\d{3}E[-+]\d+)(?:\s+complex)?\s*$", re.M)
HEAD = {"IP": "\n EOM-IP-CCSD\n -----------", "EA": "\n EOM-EA-CCSD\n -----------"}
TAIL = {"IP": "Time taken for EOM-IP-CCSD:", "EA": "Time taken for EOM-EA-CCSD:"}


def _rows(out, sector):
    block = out[out.index(HEAD[sector]):out.index(TAIL[sector])]
    print(block)
    return block, [(int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5))) for m in ROW.finditer(block)]


def test_host_prints_the_ips_and_eas_of_the_python_driver(tmp_path, monkeypatch):
    from afesp_amd.capi import Engine
    monkeypatch.setenv("AFESP_SO_FOO_AS_PUBLISHED", "1")
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, scf_e_tol=1e-12, scf_d_tol=1e-10, scf_maxiter=200, scf_read_guess=False)
    res = rhf.do_rhf(si, ints, None)
    n, nel = ints.nbasis, ints.nel
    ref = {}
    with Engine(0) as eng:
        eng.do_mp2_spatial(n, nel // 2, res.canon_coeff, res.canon_levels, ints.eri)
        eng.init_cc_spinorb(n, nel, res.canon_levels, None, 8, foo_as_published=True)
        nit, _, _ = eng.do_ccsd_spinorb(100, 1e-11, 1e-11)
        assert nit > 0
        eng.so_lambda_init(0)
        ref["IP"] = eom.so_eom_ip_solve(eng, 4)
        ref["EA"] = eom.so_eom_ea_solve(eng, 4)
        for sector, (omega, vectors, info) in ref.items():
            labels = [eom.label_ipea_root(eom.SECTOR_IP if sector == "IP" else eom.SECTOR_EA, x1, x2, n, nel // 2, nel // 2, True) for x1, x2 in vectors]
            print(sector, "python driver:\n" + eom.table(omega, info), "\ndegeneracy", info["degeneracy"],
                  [(l["kind"], l["occ"], l["virt"], l["delta_ms"]) for l in labels])
            assert all(l["delta_ms"] in (-0.5, 0.5) for l in labels)
    host, _ = run_host(tmp_path / "a", "h2o-cc-pvdz", "", ["eom_ip_nroots = 4", "eom_ea_nroots = 4"], text=_input_text())
    assert host.returncode == 0, host.stdout + host.stderr
    out = host.stdout
    assert out.index("Final CCSD Energy") < out.index(HEAD["IP"]) < out.index(TAIL["IP"]) < out.index(HEAD["EA"]) < out.index(TAIL["EA"])
    differ = []                                                             # (asserted last: what follows does not depend on it)
    for sector, (omega, vectors, info) in ref.items():
        block, rows = _rows(out, sector)
        assert [r[0] for r in rows] == [1, 2, 3, 4], block
        got = np.array([r[1] for r in rows])
        print(sector, "host", got, "python", omega, "largest difference", np.max(np.abs(got - omega)))
        if not np.max(np.abs(got - omega)) < 1e-8:
            differ.append((sector, got, omega))
        assert np.max(np.abs(np.array([r[2] for r in rows]) - got * eom.HARTREE_EV)) < 1e-6
        assert all(r[4] < 1e-8 for r in rows)
        # a closed-shell reference: the two Ms components of every doublet, at one energy
        assert abs(got[0] - got[1]) < 1e-6 and abs(got[2] - got[3]) < 1e-6 and got[2] - got[0] > 1e-3
        assert list(info["degeneracy"]) == [2, 2, 2, 2]
        assert all(0.0 < r[3] <= 1.0 + 1e-8 for r in rows)
    assert np.all(ref["IP"][0] > 0.0)
    # without the keys: the output of before -- the same lines once the two blocks and the timings are taken out
    plain, _ = run_host(tmp_path / "b", "h2o-cc-pvdz", "", [], text=_input_text())
    assert plain.returncode == 0 and "EOM" not in plain.stdout
    cut = out[:out.index(" -----------\n EOM-IP-CCSD")] + out[out.index(TAIL["EA"]):].split("\n", 1)[1]
    a, b = _untimed(cut), _untimed(plain.stdout)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty), (x, y)
        for p, q in zip(tx, ty):
            if p != q:
                assert abs(float(p) - float(q)) < 1e-8, (x, y)
    assert not differ, differ                                               # the omega of the Python driver to 1e-8, in both sectors


def test_host_runs_the_sectors_after_lambda_and_eom_ee(tmp_path, monkeypatch):
    monkeypatch.setenv("AFESP_SO_FOO_AS_PUBLISHED", "1")
    host, _ = run_host(tmp_path, "h2o-cc-pvdz", "", ["eom_nroots = 2", "cc_density = .true.", "eom_ip_nroots = 2", "eom_ea_nroots = 2"],
                       text=_input_text())
    assert host.returncode == 0, host.stdout + host.stderr
    out = host.stdout
    assert (out.index("CCSD Lambda") < out.index("Natural occupation numbers") < out.index("\n EOM-CCSD\n ----------") < out.index(HEAD["IP"])
            < out.index(HEAD["EA"]))
    for sector in ("IP", "EA"):
        _, rows = _rows(out, sector)
        assert len(rows) == 2 and abs(rows[0][1] - rows[1][1]) < 1e-6        # the two components of the lowest doublet
    # one sector alone, with nothing before it that made the Lambda state
    alone, _ = run_host(tmp_path / "ea", "h2o-cc-pvdz", "", ["eom_ea_nroots = 2"], text=_input_text())
    assert alone.returncode == 0, alone.stdout + alone.stderr
    assert "EOM-IP" not in alone.stdout
    _, rows_alone = _rows(alone.stdout, "EA")
    assert len(rows_alone) == 2 and abs(rows_alone[0][1] - rows[0][1]) < 1e-8
