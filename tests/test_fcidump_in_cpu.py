"""A standard FCIDUMP as input, the parts that need no GPU: the new entry points are bound everywhere, afesp_fcidump_scan (host only) on
headers written every way the format allows, and the fcidump_in namelist key with the combinations it refuses."""
import os

import numpy as np
import pytest

import molecules
import np_fcidump
import np_fcidump_in
from afesp_amd import capi, inputs

ROOT = os.path.dirname(os.path.dirname(molecules.GOLDEN))
PKG = os.path.join(ROOT, "a-fortran-electronic-structure-program_amd")


def test_the_new_calls_are_bound_everywhere():
    names = ["afesp_fcidump_scan", "afesp_read_fcidump", "afesp_read_fcidump_uhf"]
    header = open(os.path.join(ROOT, "include", "afesp.h")).read()
    f90 = open(os.path.join(PKG, "host", "afesp_capi.f90")).read()
    lib = capi.load_library()
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
        assert f"int {name}(" in header and f"bind(C, name='{name}')" in f90
    assert "AFESP_FCIDUMP_CHUNK_KIB" in header and "AFESP_FCIDUMP_CHUNK_KIB" in open(os.path.join(PKG, "csrc", "knobs.h")).read()
    assert callable(capi.scan_fcidump) and callable(capi.Engine.read_fcidump)


BODY = " 0.5 1 1 1 1\n\n 0.25D0 2 1 0 0\r\n -1.0 0 0 0 0\n"


@pytest.mark.parametrize("head,want", [
    ("&FCI NORB=4,NELEC=2,MS2=0, ORBSYM=1,1,1,1, ISYM=1, &END\n", (4, 2, 0, False)),
    (" &FCI NORB=4,NELEC=2,MS2=0,\n  ORBSYM=1,1,1,1,\n  ISYM=1,\n &END\n", (4, 2, 0, False)),
    ("&fci\n nelec = 4 ,\n ms2=2,\n orbsym=1,1,1,1,1,1\n norb= 6\n&end\n", (6, 4, 2, False)),
    ("&FCI NORB=4,NELEC=2,MS2=0,\n ORBSYM=1,1,1,1,\n ISYM=1\n /\n", (4, 2, 0, False)),
    ("&FCI NORB=3,NELEC=2,ORBSYM=1,1,1,ISYM=1, &END\n", (3, 2, 0, False)),
    (" &FCI NORB=6,NELEC=3,MS2=1,\n  ORBSYM=1,1,1,1,1,1,\n  ISYM=1,\n  UHF=.TRUE.,\n &END\n", (6, 3, 1, True)),
    ("&FCI NORB=6,NELEC=3,MS2=-1, uhf = .true. /\n", (6, 3, -1, True)),
])
def test_scan_reads_the_header_however_it_is_written(tmp_path, head, want):
    path = tmp_path / "FCIDUMP"
    path.write_text(head + BODY)
    hd = capi.scan_fcidump(path)
    assert (hd.norb, hd.nelec, hd.ms2, hd.uhf) == want
    assert hd.nlines == 3                       # the blank line does not count


def test_scan_agrees_with_the_writer_and_refuses_what_is_no_fcidump(tmp_path):
    n, rng = 5, np.random.default_rng(1)
    text = np_fcidump.dump_text(n, 4, 0, np_fcidump_in.random_packed(rng, n), np_fcidump_in.sym(rng, n), -2.0)
    path = tmp_path / "FCIDUMP"
    path.write_text(text)
    hd = capi.scan_fcidump(path)
    assert (hd.norb, hd.nelec, hd.ms2, hd.uhf, hd.nlines) == (n, 4, 0, False, inputs.neri(n) + inputs.npair(n) + 1)
    path.write_text(text.rstrip("\n"))             # the last line without its newline still counts
    assert capi.scan_fcidump(path).nlines == hd.nlines
    # one definition of a blank line in the scan and in the reader: a form feed or a vertical tab alone makes none
    path.write_text(text.replace("&END\n", "&END\n \f\r\n\v\n", 1) + "\f\n")
    assert capi.scan_fcidump(path).nlines == hd.nlines
    lib = capi.load_library()
    for bad in(" 1.0 1 1 1 1\n", "NORB=4,NELEC=2 &END\n 1.0 1 1 1 1\n", "&FCI NORB=4,NELEC=2,\n 1.0 1 1 1 1\n", "&FCI NELEC=2 &END\n", ""):
        path.write_text(bad)
        assert lib.afesp_fcidump_scan(str(path).encode(), None, None, None, None, None) != 0, bad
        with pytest.raises(capi.AfespError):
            capi.scan_fcidump(path)
    assert lib.afesp_fcidump_scan(None, None, None, None, None, None) != 0
    assert lib.afesp_fcidump_scan(str(tmp_path / "missing").encode(), None, None, None, None, None) != 0


def _els_in(tmp_path, body):
    p = tmp_path / "els.in"
    p.write_text("&elsinput\n" + body + "\n/\n")
    return str(p)


def test_the_fcidump_in_key_and_what_it_refuses(tmp_path):
    assert inputs.read_els_in(os.path.join(molecules.GOLDEN, "h2o-cc-pvdz", "els.in")).fcidump_in is False
    si = inputs.read_els_in(_els_in(tmp_path, 'calc_type="CCSD(T)_spatial",\nfcidump_in=.true.,\nn_frozen_core=1,\nn_frozen_virt=2'))
    assert si.fcidump_in is True and (si.n_frozen_core, si.n_frozen_virt) == (1, 2)
    si = inputs.read_els_in(_els_in(tmp_path, 'calc_type="UCCSD(T)",\ncharge=1,\nmultiplicity=2,\nfcidump_in=.true.'))
    assert si.fcidump_in is True
    for bad, msg in (("frozen_core=.true.", "geom.dat"), ("fno_n_virt=5", "natural orbitals"), ("fno_occ_tol=1e-4", "natural orbitals"),
                     ("write_fcidump=.true.", "overwrite"), ("fcidump_active=.true.", "overwrite"), ("scf_read_guess=.true.", "no SCF"),
                     ("scf_write_guess=.true.", "no SCF")):
        with pytest.raises(ValueError, match=msg):
            inputs.read_els_in(_els_in(tmp_path, 'calc_type="CCSD(T)_spatial",\nfcidump_in=.true.,\n' + bad))
    with pytest.raises(ValueError, match="no SCF"):
        inputs.read_els_in(_els_in(tmp_path, 'calc_type="RHF",\nfcidump_in=.true.'))
    with pytest.raises(ValueError):
        inputs.read_els_in(_els_in(tmp_path, 'calc_type="MP2_spatial",\nfcidump_in=3'))
    # the Fortran host knows the key and words its refusals alike
    host = open(os.path.join(PKG, "host", "els_host.f90")).read()
    assert "fcidump_in" in host
    for piece in ("frozen_core counts atoms in geom.dat", "frozen natural orbitals need the AO integrals", "would overwrite it",
                  "fcidump_in runs no SCF"):
        assert piece in host, piece
