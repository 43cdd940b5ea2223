"""The Fortran host with eom_ip_nroots = eom_ea_nroots = 4 and eom_ipea_left on the bundled H2O/cc-pVDZ input as CCSD_spinorb
(AFESP_SO_FOO_AS_PUBLISHED=1, as tests/test_gpu_eom_ipea_host.py): Lambda is converged before the sectors, each sector's table is followed
by the table of the left solve with the pole strengths, the left roots are the printed right ones, the pole strengths are those of the
Python driver (afesp_amd.eom) on the same input, equal inside every twofold cluster and in (0, 1], and without the key the output is the
one of before.

Bounds.  1e-8 for omega: the parity bar of the host tests for two separately converged solves.  1e-6 for the pole strengths of the two
drivers: both stop at residuals below 1e-8, an eigenvector is then off by at most residual / gap, the distinct roots asked for here lie
more than 1e-2 Eh apart (asserted below), and the pole strength is bilinear in vectors of norm O(1).  The two members of a cluster come out
of one solve: their strengths differ only by that same eigenvector error, the same bound.  No external pole strength for this geometry
is at hand: none is quoted."""
import dataclasses
import re

import numpy as np

import molecules
import pytest
from afesp_amd import density, eom, rhf
from test_gpu_eom_host import _input_text, _untimed
from test_gpu_eom_ipea_host import HEAD, TAIL, _rows
from test_gpu_frozen_host import run_host

pytestmark = pytest.mark.gpu

LEFT_ROW = re.compile(r"^\s+(\d+)\s+(-?\d+\.\d{12})\s+(-?\d+\.\d{10})\s+(\d\.\d{3}E[-+]\d+)\s+(\d\.\d{3}E[-+]\d+)\s+(-?\d+\.\d{14})\s*$", re.M)
LEFT_HEAD = " Left eigenvectors: Davidson steps:"


def _left_rows(block):
    return [(int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5)), float(m.group(6)))
            for m in LEFT_ROW.finditer(block[block.index(LEFT_HEAD):])]


def test_host_prints_the_left_roots_and_pole_strengths_of_the_python_driver(tmp_path, monkeypatch):
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
        density.so_lambda_solve(eng, 100, 1e-11, 1e-11)
        for sector, sec, solve, left in (("IP", eom.SECTOR_IP, eom.so_eom_ip_solve, eom.so_eom_ip_left_solve),
                                         ("EA", eom.SECTOR_EA, eom.so_eom_ea_solve, eom.so_eom_ea_left_solve)):
            omega, R, _ = solve(eng, 4)
            wl, L, linfo = left(eng, R)
            props = eom.so_eom_ipea_properties(eng, sec, eom.biorthonormalise_ipea(omega, L, R), R)
            pole = np.array([p["pole_strength"] for p in props])
            print(sector, "python driver:\n" + eom.ipea_left_table(wl, omega, linfo, pole))
            ref[sector] = (omega, wl, pole)
    keys = ["eom_ip_nroots = 4", "eom_ea_nroots = 4"]
    host, _ = run_host(tmp_path / "a", "h2o-cc-pvdz", "", keys + ["eom_ipea_left = .true."], text=_input_text())
    assert host.returncode == 0, host.stdout + host.stderr
    out = host.stdout
    assert out.index("Final CCSD Energy") < out.index("CCSD Lambda") < out.index(HEAD["IP"]) < out.index(TAIL["IP"]) < out.index(HEAD["EA"])
    for sector, (omega, wl, pole) in ref.items():
        block, rows = _rows(out, sector)
        right = np.array([r[1] for r in rows[:4]])
        left = _left_rows(block)
        assert [r[0] for r in left] == [1, 2, 3, 4], block
        got_w, got_p = np.array([r[1] for r in left]), np.array([r[5] for r in left])
        print(sector, "host omega_left - omega_right", got_w - right, "host - python: omega", got_w - wl, "pole strengths", got_p - pole, got_p)
        assert np.max(np.abs(got_w - right)) < 1e-8 and np.max(np.abs(got_w - wl)) < 1e-8
        assert all(r[3] < 1e-8 and r[4] < 1e-8 for r in left)               # the printed |left - right| and residual
        assert np.max(np.abs(np.array([r[2] for r in left]) - got_w * eom.HARTREE_EV)) < 1e-6
        assert abs(right[0] - right[1]) < 1e-6 and abs(right[2] - right[3]) < 1e-6 and right[2] - right[0] > 1e-2
        assert np.max(np.abs(got_p - pole)) < 1e-6
        assert abs(got_p[0] - got_p[1]) < 1e-6 and abs(got_p[2] - got_p[3]) < 1e-6
        assert np.all(got_p > 0.0) and np.all(got_p <= 1.0 + 1e-8)
    # without the key: the output of before -- the same lines once the Lambda block, the two left tables and the timings are taken out
    plain, _ = run_host(tmp_path / "b", "h2o-cc-pvdz", "", keys, text=_input_text())
    assert plain.returncode == 0 and "Left eigenvectors" not in plain.stdout and "CCSD Lambda" not in plain.stdout
    cut = out[:out.index(" ----------\n CCSD Lambda")] + out[out.index(" -----------\n EOM-IP-CCSD"):]
    for sector in ("IP", "EA"):
        lo = cut.index(LEFT_HEAD, cut.index(HEAD[sector]))
        cut = cut[:lo] + cut[cut.index(TAIL[sector]):]
    a, b = _untimed(cut), _untimed(plain.stdout)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty), (x, y)
        for p, q in zip(tx, ty):
            if p != q:
                assert abs(float(p) - float(q)) < 1e-8, (x, y)
