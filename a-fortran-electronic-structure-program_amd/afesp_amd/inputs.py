"""Readers for the reference's on-disk inputs and stdout goldens.

File formats follow the reference's readers (citations into /root/reference):
  els.in namelist ............ src/system.f90:81-167 (defaults = system_t, :43-67)
  s.dat / t.dat / v.dat ...... src/integrals.f90:94-137 (1-based "i j value", lower triangle)
  eri.dat .................... src/integrals.f90:146-161 ("i j k l value", 8-fold unique entries)
  geom.dat ................... src/geometry.f90:23-46, e_nuc :74-95
  guess_in.dat ............... src/hf.f90:153-170
  stdout energy table ........ src/main.F90:123-175 (what utils/els_wrapper.py:104-127 greps)
"""
from __future__ import annotations

import dataclasses
import os
import re

import numpy as np


@dataclasses.dataclass
class SystemIn:
    """Mirror of the user-facing part of system_t (src/system.f90:10-69)."""
    calc_type: str = "CCSD(T)_spatial"
    scf_e_tol: float = 1e-6
    scf_d_tol: float = 1e-6
    scf_diis_n_errmat: int = 6
    ccsd_e_tol: float = 1e-6
    ccsd_t_tol: float = 1e-6
    ccsd_diis_n_errmat: int = 8
    scf_maxiter: int = 50
    ccsd_maxiter: int = 50
    write_fcidump: bool = False
    fcidump_active: bool = False    # the active space as a standard FCIDUMP (afesp_amd/fcidump.py); excludes write_fcidump (same file name)
    fcidump_in: bool = False        # MO integrals from ./FCIDUMP (Engine.read_fcidump): no SCF, no transform; excludes what needs AO data
    scf_read_guess: bool = False
    scf_write_guess: bool = False
    charge: int = 0                 # open-shell types only (UHF_scf, UMP2, UCCSD, UCCSD(T))
    multiplicity: int = 1           # 2S + 1
    # active orbital window of the correlated steps (no counterpart in the reference): all three absent = every orbital correlated
    frozen_core: bool = False       # freeze the noble-gas cores counted from geom.dat (frozen_core_count)
    n_frozen_core: int = -1         # explicit number of lowest MOs to freeze; -1 = not given; wins over frozen_core
    n_frozen_virt: int = 0          # highest MOs dropped
    # frozen natural orbitals: the virtual space truncated in the basis of the MP2 natural virtuals (afesp_amd/fno.py); at most one of the two
    fno_n_virt: int = -1            # number of natural virtuals kept; -1 = off
    fno_occ_tol: float = 0.0        # keep every natural virtual whose occupation is at least this; 0 = off
    cc_density: bool = False        # after a converged spin-orbital CCSD: Lambda and the natural occupations (afesp_amd/density.py)
    cc_rdm2: bool = False           # ... Lambda, the two-particle density, the density-side energy and <S^2> (density.s_squared)
    cc_relaxed: bool = False        # ... Lambda, the two-particle density, the Z-vector and the orbital-relaxed density (density.so_relaxed_density_solve)
    cc_lambda_t: bool = False       # after a converged spin-orbital CCSD: Lambda and the Lambda-CCSD(T) correction (density.so_lambda_t_correction)
    eom_nroots: int = 0             # after a converged spin-orbital CCSD: this many EOM-EE-CCSD excitation energies (afesp_amd/eom.py); 0 = off
    cc_polar: bool = False          # ... the EOM-CCSD polarisability alpha(omega) from dipx.dat / dipy.dat / dipz.dat (afesp_amd/response.py)
    polar_omega: list = dataclasses.field(default_factory=lambda: [0.0])   # ... at these real frequencies / Eh (up to 8)
    polar_gamma: float = 0.0        # ... > 0: every polar_omega is solved at omega + i gamma (damped response: Re / Im alpha-bar and sigma(omega))
    polar_c6_npts: int = 0          # ... > 0: alpha-bar(iu) on this many Casimir-Polder grid points and the homo-dimer C6 (response.casimir_polder_grid)
    eom_left: bool = False          # ... and their left eigenvectors, from the right ones as guess (eom.so_eom_left_solve); needs eom_nroots > 0
    eom_triples: bool = False       # ... and the non-iterative triples correction to every root (eom.so_eom_triples_correction); needs eom_left
    eom_ip_nroots: int = 0         # ... this many EOM-IP-CCSD ionisation potentials; 0 = off
    eom_ea_nroots: int = 0          # ... this many EOM-EA-CCSD electron affinities; 0 = off
    eom_ipea_left: bool = False     # ... and the left eigenvectors and pole strengths of those roots (eom.so_eom_ipea_properties); needs one of the two > 0
    eom_ipea_triples: bool = False  # ... and the non-iterative triples correction to those roots (eom.so_eom_ip_triples_correction / _ea_); needs eom_ipea_left
    # derived by the calc_type switch (src/system.f90:116-165)
    level: str = "CCSD(T)"        # one of RHF, MP2, CCSD, CCSD(T)
    restricted: bool = True
    ccsd_t_paren: bool = False
    ccsd_t_renorm: bool = False
    ccsd_t_comp_renorm: bool = False


_CALC_TYPES = {
    # name: (level, restricted, paren, renorm, comp_renorm)   src/system.f90:116-165
    "RHF": ("RHF", True, False, False, False),
    "UHF": ("RHF", False, False, False, False),
    "MP2_spinorb": ("MP2", False, False, False, False),
    "MP2_spatial": ("MP2", True, False, False, False),
    "CCSD_spinorb": ("CCSD", False, False, False, False),
    "CCSD_spatial": ("CCSD", True, False, False, False),
    "CCSD(T)_spinorb": ("CCSD(T)", False, False, False, False),
    "CCSD(T)_spatial": ("CCSD(T)", True, True, False, False),
    "CCSD[T]_spatial": ("CCSD(T)", True, False, False, False),
    "RCCSD(T)_spatial": ("CCSD(T)", True, True, True, False),
    "RCCSD[T]_spatial": ("CCSD(T)", True, False, True, False),
    "CRCCSD(T)_spatial": ("CCSD(T)", True, True, False, True),
    "CRCCSD[T]_spatial": ("CCSD(T)", True, False, False, True),
    # open-shell types on canonical UHF orbitals (no counterpart in the reference, whose "UHF" runs RHF)
    "UHF_scf": ("UHF", False, False, False, False),
    "UMP2": ("UMP2", False, False, False, False),
    "UCCSD": ("UCCSD", False, False, False, False),
    "UCCSD(T)": ("UCCSD(T)", False, False, False, False),
}
OPEN_SHELL_TYPES = ("UHF_scf", "UMP2", "UCCSD", "UCCSD(T)")
CC_DENSITY_TYPES = ("CCSD_spinorb", "CCSD(T)_spinorb", "UCCSD", "UCCSD(T)")   # (the host adds its ROHF-CCSD types)


def _parse_value(text: str):
    t = text.strip().rstrip(",").strip()
    if t.lower() in (".true.", "t", "true"):
        return True
    if t.lower() in (".false.", "f", "false"):
        return False
    if t and t[0] in "\"'":
        return t.strip("\"'")
    try:
        return int(t)
    except ValueError:
        return float(t.lower().replace("d", "e"))


def read_els_in(path: str) -> SystemIn:
    """Parse the &elsinput namelist.  Keys that are absent keep the system_t defaults
    (the reference leaves them uninitialised -- SURVEY.md section 5 hazard)."""
    sysin = SystemIn()
    body = open(path).read()
    m = re.search(r"&elsinput(.*?)^\s*/", body, re.S | re.M | re.I)
    if not m:
        raise ValueError("invalid input file format!")   # system.f90:111
    for key, val in re.findall(r"(\w+)\s*=\s*(\"[^\"]*\"|'[^']*'|[^,\n]+)", m.group(1)):
        key = key.lower()
        if not hasattr(sysin, key):
            raise ValueError("invalid input file format!")
        setattr(sysin, key, _parse_value(val))
    # polar_omega is the one list-valued key: every number behind it, comma-separated (the loop above kept the first alone)
    pm = re.search(r"\bpolar_omega\s*=\s*((?:\s*[-+]?(?:\d+\.?\d*|\.\d+)(?:[eEdD][-+]?\d+)?\s*,?)+)", m.group(1), re.I)
    if pm:
        sysin.polar_omega = [float(x.lower().replace("d", "e")) for x in pm.group(1).replace(",", " ").split()]
    elif not isinstance(sysin.polar_omega, list):
        raise ValueError("invalid input file format!")
    if sysin.calc_type not in _CALC_TYPES:
        raise ValueError("Unrecognised calculation type!")   # system.f90:163
    (sysin.level, sysin.restricted, sysin.ccsd_t_paren, sysin.ccsd_t_renorm,
     sysin.ccsd_t_comp_renorm) = _CALC_TYPES[sysin.calc_type]
    if not isinstance(sysin.charge, int) or isinstance(sysin.charge, bool) or not isinstance(sysin.multiplicity, int) \
            or isinstance(sysin.multiplicity, bool) or sysin.multiplicity < 1:
        raise ValueError("invalid input file format!")
    if (sysin.charge, sysin.multiplicity) != (0, 1) and sysin.calc_type not in OPEN_SHELL_TYPES:
        raise ValueError("charge and multiplicity need an open-shell calculation type!")
    if not isinstance(sysin.frozen_core, bool) or not isinstance(sysin.fcidump_active, bool):
        raise ValueError("invalid input file format!")
    if sysin.fcidump_active and sysin.write_fcidump:
        raise ValueError("write_fcidump and fcidump_active both write FCIDUMP: choose one!")
    if not isinstance(sysin.fcidump_in, bool):
        raise ValueError("invalid input file format!")
    if sysin.fcidump_in:
        if sysin.frozen_core:
            raise ValueError("fcidump_in: frozen_core counts atoms in geom.dat, which is not read: give n_frozen_core!")
        if fno_requested(sysin):
            raise ValueError("fcidump_in: frozen natural orbitals need the AO integrals, which are not read!")
        if sysin.write_fcidump or sysin.fcidump_active:
            raise ValueError("fcidump_in reads FCIDUMP: write_fcidump / fcidump_active would overwrite it!")
        if sysin.scf_read_guess or sysin.scf_write_guess:
            raise ValueError("fcidump_in runs no SCF: scf_read_guess / scf_write_guess have nothing to act on!")
        if sysin.level in ("RHF", "UHF"):
            raise ValueError("fcidump_in runs no SCF: choose a correlated calculation type!")
    for key in ("n_frozen_core", "n_frozen_virt"):
        val = getattr(sysin, key)
        if not isinstance(val, int) or isinstance(val, bool) or val < -1:
            raise ValueError(f"{key} must be a non-negative integer!")
    if not isinstance(sysin.fno_n_virt, int) or isinstance(sysin.fno_n_virt, bool) or sysin.fno_n_virt < -1:
        raise ValueError("fno_n_virt must be a non-negative integer!")
    if isinstance(sysin.fno_occ_tol, bool) or not isinstance(sysin.fno_occ_tol, (int, float)) or sysin.fno_occ_tol < 0.0:
        raise ValueError("fno_occ_tol must be a non-negative number!")
    sysin.fno_occ_tol = float(sysin.fno_occ_tol)
    if sysin.fno_n_virt >= 0 and sysin.fno_occ_tol > 0.0:
        raise ValueError("fno_n_virt and fno_occ_tol exclude each other!")
    if fno_requested(sysin) and sysin.n_frozen_virt > 0:
        raise ValueError("frozen natural orbitals and n_frozen_virt exclude each other!")
    if sysin.fno_n_virt == 0:
        raise ValueError("fno_n_virt leaves no active virtual orbital!")
    if not isinstance(sysin.cc_density, bool):
        raise ValueError("invalid input file format!")
    if sysin.cc_density and sysin.calc_type not in CC_DENSITY_TYPES:
        raise ValueError(f"{sysin.calc_type} takes no cc_density: the Lambda equations run on the spin-orbital CCSD types!")
    if sysin.cc_density and sysin.fcidump_in and sysin.calc_type in OPEN_SHELL_TYPES:
        raise ValueError("cc_density on a UHF FCIDUMP: the file does not hold the overlap of its alpha and beta orbitals, which the "
                         "spin-summed density needs!")
    if not isinstance(sysin.cc_rdm2, bool):
        raise ValueError("invalid input file format!")
    if sysin.cc_rdm2 and sysin.calc_type not in CC_DENSITY_TYPES:
        raise ValueError(f"{sysin.calc_type} takes no cc_rdm2: the Lambda equations run on the spin-orbital CCSD types!")
    if sysin.cc_rdm2 and sysin.fcidump_in and sysin.calc_type in OPEN_SHELL_TYPES:
        raise ValueError("cc_rdm2 on a UHF FCIDUMP: the file does not hold the overlap of its alpha and beta orbitals, which <S^2> needs!")
    if not isinstance(sysin.cc_relaxed, bool):
        raise ValueError("invalid input file format!")
    if sysin.cc_relaxed and sysin.calc_type not in CC_DENSITY_TYPES:
        raise ValueError(f"{sysin.calc_type} takes no cc_relaxed: the Lambda equations run on the spin-orbital CCSD types!")
    if sysin.cc_relaxed and (sysin.frozen_core or sysin.n_frozen_core > 0 or sysin.n_frozen_virt > 0 or fno_requested(sysin)):
        raise ValueError("cc_relaxed with a frozen-core / frozen-virtual window or frozen natural orbitals: the windowed state lacks the "
                         "core-active integrals that orbital relaxation needs!")
    if not isinstance(sysin.cc_lambda_t, bool):
        raise ValueError("invalid input file format!")
    if sysin.cc_lambda_t and sysin.calc_type not in CC_DENSITY_TYPES:   # (no orbital overlap needed: a UHF FCIDUMP takes it)
        raise ValueError(f"{sysin.calc_type} takes no cc_lambda_t: the Lambda equations run on the spin-orbital CCSD types!")
    if not isinstance(sysin.eom_nroots, int) or isinstance(sysin.eom_nroots, bool) or sysin.eom_nroots < 0:
        raise ValueError("eom_nroots must be a non-negative integer!")
    if sysin.eom_nroots > 0 and sysin.calc_type not in CC_DENSITY_TYPES:
        raise ValueError(f"{sysin.calc_type} takes no eom_nroots: the EOM-CCSD equations run on the spin-orbital CCSD types!")
    if not isinstance(sysin.eom_left, bool):
        raise ValueError("invalid input file format!")
    if sysin.eom_left and sysin.eom_nroots == 0:
        raise ValueError("eom_left needs eom_nroots > 0: the left eigenvectors are those of the EOM-EE-CCSD roots it asks for!")
    if not isinstance(sysin.eom_triples, bool):
        raise ValueError("invalid input file format!")
    if sysin.eom_triples and not (sysin.eom_nroots > 0 and sysin.eom_left):
        raise ValueError("eom_triples needs eom_nroots > 0 and eom_left: the triples correction contracts the left and right vectors of "
                         "the EOM-EE-CCSD roots!")
    if not isinstance(sysin.cc_polar, bool):
        raise ValueError("invalid input file format!")
    if sysin.cc_polar and sysin.calc_type not in CC_DENSITY_TYPES:
        raise ValueError(f"{sysin.calc_type} takes no cc_polar: the response equations run on the spin-orbital CCSD types!")
    if sysin.cc_polar and sysin.fcidump_in:
        raise ValueError("cc_polar with fcidump_in: the operator files dipx.dat / dipy.dat / dipz.dat are in the AO basis, which a FCIDUMP "
                         "run does not have!")
    if not 1 <= len(sysin.polar_omega) <= 8:
        raise ValueError("polar_omega takes at most 8 frequencies!")
    if isinstance(sysin.polar_gamma, bool) or not isinstance(sysin.polar_gamma, (int, float)) or not sysin.polar_gamma >= 0.0:
        raise ValueError("polar_gamma is a damping in Eh, zero (real frequencies) or positive!")
    sysin.polar_gamma = float(sysin.polar_gamma)
    if not isinstance(sysin.polar_c6_npts, int) or isinstance(sysin.polar_c6_npts, bool) or not 0 <= sysin.polar_c6_npts <= 21:
        raise ValueError("polar_c6_npts is the number of Casimir-Polder grid points, 0 (off) to 21 (three operators each, 64 systems in one response state)!")
    for key in ("eom_ip_nroots", "eom_ea_nroots"):
        val = getattr(sysin, key)
        if not isinstance(val, int) or isinstance(val, bool) or val < 0:
            raise ValueError(f"{key} must be a non-negative integer!")
        if val > 0 and sysin.calc_type not in CC_DENSITY_TYPES:
            raise ValueError(f"{sysin.calc_type} takes no {key}: the EOM-CCSD equations run on the spin-orbital CCSD types!")
    if not isinstance(sysin.eom_ipea_left, bool):
        raise ValueError("invalid input file format!")
    if sysin.eom_ipea_left and sysin.eom_ip_nroots == 0 and sysin.eom_ea_nroots == 0:
        raise ValueError("eom_ipea_left needs eom_ip_nroots > 0 or eom_ea_nroots > 0: the left eigenvectors and pole strengths are those of "
                         "the EOM-IP-CCSD / EOM-EA-CCSD roots they ask for!")
    if not isinstance(sysin.eom_ipea_triples, bool):
        raise ValueError("invalid input file format!")
    if sysin.eom_ipea_triples and not (sysin.eom_ipea_left and (sysin.eom_ip_nroots > 0 or sysin.eom_ea_nroots > 0)):
        raise ValueError("eom_ipea_triples needs eom_ipea_left and eom_ip_nroots > 0 or eom_ea_nroots > 0: the triples correction contracts "
                         "the left and right vectors of the EOM-IP-CCSD / EOM-EA-CCSD roots!")
    return sysin


def fno_requested(sysin: SystemIn) -> bool:
    """True if the input asks for frozen natural orbitals (either key)."""
    return sysin.fno_n_virt >= 0 or sysin.fno_occ_tol > 0.0


def check_fno_count(sysin: SystemIn, nvirt: int) -> None:
    """fno_n_virt against the number of virtuals of the system (the smaller of the two spins' for an open shell): 1 ... nvirt."""
    if sysin.fno_n_virt >= 0 and not 1 <= sysin.fno_n_virt <= nvirt:
        raise ValueError("fno_n_virt leaves no active virtual orbital or exceeds the number of virtual orbitals!")


def frozen_core_count(z_list) -> int:
    """Number of doubly occupied core orbitals of the atoms with these nuclear charges: the noble-gas core below each atom's valence
    shell (Z <= 2: 0, <= 10: 1 (He), <= 18: 5 (Ne), <= 36: 9 (Ar)); heavier atoms are refused."""
    total = 0
    for z in z_list:
        z = int(z)
        if z < 1 or z > 36:
            raise ValueError("frozen_core: no core count for atoms beyond Kr!")
        total += 0 if z <= 2 else 1 if z <= 10 else 5 if z <= 18 else 9
    return total


def frozen_window(sysin: SystemIn, z_list) -> tuple[int, int]:
    """(nfc, nfv) an input asks for: n_frozen_core where given, else the counted cores if frozen_core, else 0; -1 for n_frozen_virt
    reads as its default."""
    nfc = sysin.n_frozen_core if sysin.n_frozen_core >= 0 else (frozen_core_count(z_list) if sysin.frozen_core else 0)
    return nfc, max(sysin.n_frozen_virt, 0)


def read_nuclear_charges(path: str) -> list[int]:
    """The nuclear charges of geom.dat (src/geometry.f90:23-46), in file order."""
    with open(path) as fh:
        natoms = int(fh.readline().split()[0])
        return [int(float(fh.readline().split()[0])) for _ in range(natoms)]


def spin_counts(sysin: SystemIn, nuclear_charge: int, nbasis: int) -> tuple[int, int]:
    """(n_alpha, n_beta) of nel = sum Z - charge electrons at multiplicity 2S + 1."""
    nel = nuclear_charge - sysin.charge
    twice_a = nel + sysin.multiplicity - 1
    if nel < 0 or twice_a % 2:
        raise ValueError("charge and multiplicity do not fit the electron count!")
    na, nb = twice_a // 2, (nel - sysin.multiplicity + 1) // 2
    if nb < 0 or na > nbasis:
        raise ValueError("charge and multiplicity do not fit the electron count!")
    return na, nb


def eri_index(i, j, k, l):
    """0-based packed index of (ij|kl): src/integrals.f90:196-210 composed twice."""
    def tri(a, b):
        a, b = np.maximum(a, b), np.minimum(a, b)
        return a * (a + 1) // 2 + b
    return tri(tri(i, j), tri(k, l))


def npair(n: int) -> int:
    return n * (n + 1) // 2


def neri(n: int) -> int:
    npr = npair(n)
    return npr * (npr + 1) // 2


@dataclasses.dataclass
class Integrals:
    nbasis: int
    ovlp: np.ndarray
    ke: np.ndarray
    ele_nuc: np.ndarray
    core_hamil: np.ndarray
    eri: np.ndarray          # packed, length neri(nbasis)
    e_nuc: float = 0.0
    nel: int = 0
    natoms: int = 0


def _read_two_index(path: str, n: int | None = None):
    dat = np.loadtxt(path, ndmin=2)
    i = dat[:, 0].astype(np.int64) - 1
    j = dat[:, 1].astype(np.int64) - 1
    if n is None:
        n = int(max(i.max(), j.max())) + 1      # integrals.f90:82-91
    mat = np.zeros((n, n))
    mat[i, j] = dat[:, 2]
    mat[j, i] = dat[:, 2]
    return mat, n


def read_integrals(directory: str) -> Integrals:
    """s.dat, t.dat, v.dat, eri.dat, geom.dat from `directory` (hard-coded names, integrals.f90:69-73)."""
    ovlp, n = _read_two_index(os.path.join(directory, "s.dat"))
    ke, _ = _read_two_index(os.path.join(directory, "t.dat"), n)
    en, _ = _read_two_index(os.path.join(directory, "v.dat"), n)
    dat = np.loadtxt(os.path.join(directory, "eri.dat"), ndmin=2)
    idx = dat[:, :4].astype(np.int64) - 1
    eri = np.zeros(neri(n))
    eri[eri_index(idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3])] = dat[:, 4]
    ints = Integrals(n, ovlp, ke, en, ke + en, eri)
    # geometry.f90:23-46, :74-95
    with open(os.path.join(directory, "geom.dat")) as fh:
        natoms = int(fh.readline().split()[0])
        charges, coords = [], []
        for _ in range(natoms):
            w = fh.readline().split()
            charges.append(int(float(w[0])))
            coords.append([float(x) for x in w[1:4]])
    coords = np.array(coords)
    e_nuc = 0.0
    for b in range(1, natoms):
        for a in range(b):
            e_nuc += charges[a] * charges[b] / np.linalg.norm(coords[a] - coords[b])
    ints.e_nuc, ints.nel, ints.natoms = e_nuc, int(sum(charges)), natoms
    return ints


def read_scf_guess(path: str, n: int) -> np.ndarray:
    dat = np.loadtxt(path, ndmin=2)
    g = np.zeros((n, n))
    g[dat[:, 0].astype(int) - 1, dat[:, 1].astype(int) - 1] = dat[:, 2]
    return g


_ENERGY_LINES = {
    "RHF energy": "rhf_total",
    "MP2 correlation energy": "mp2_corr",
    "CCSD correlation energy": "ccsd_corr",
    "CCSD[T] correlation energy": "ccsd_bt_corr",
    "CCSD(T) correlation energy": "ccsd_pt_corr",
    "R-CCSD[T] correlation energy": "r_ccsd_bt_corr",
    "R-CCSD(T) correlation energy": "r_ccsd_pt_corr",
    "CR-CCSD[T] correlation energy": "cr_ccsd_bt_corr",
    "CR-CCSD(T) correlation energy": "cr_ccsd_pt_corr",
    "T1 diagnostic": "t1_diag",
    "D[T]": "d_bt",
    "D(T)": "d_pt",
    "UHF energy": "uhf_total",
    "<S^2>": "s2",
    "UMP2 correlation energy": "ump2_corr",
    "UCCSD correlation energy": "uccsd_corr",
    "UCCSD(T) correlation energy": "uccsd_pt_corr",
    "ΛCCSD(T) correlation energy": "lambda_ccsd_pt_corr",       # cc_lambda_t (the host's own lines, as the open-shell ones above)
    "UΛCCSD(T) correlation energy": "lambda_uccsd_pt_corr",
    "Nuclear repulsion": "e_nuc",
    "Total energy": "total",
}


def parse_els_out(path: str) -> dict:
    """Pull the machine-readable numbers out of a reference stdout capture: the final energy table
    (main.F90:123-175), the SCF and CCSD iteration tables (hf.f90:110-113, ccsd.f90:326-331,362-363)
    and the orbital energies (hf.f90:119-122)."""
    out: dict = {"scf_iters": [], "cc_iters": [], "orbital_energies": {}}
    section = None
    final = False
    for line in open(path):
        s = line.strip()
        if s.startswith("Restricted Hartree-Fock"):
            section = "scf"
        elif s == "CCSD":
            section = "cc"
        elif s.startswith("Final energy breakdown"):
            final = True
            section = None
        if final:
            m = re.match(r"(.+?):\s+(-?\d+\.\d+)\s*$", s)
            if m and m.group(1).strip() in _ENERGY_LINES:
                out[_ENERGY_LINES[m.group(1).strip()]] = float(m.group(2))
            continue
        if section == "scf":
            w = s.split()
            if len(w) == 5 and w[0].isdigit():
                out["scf_iters"].append((int(w[0]), float(w[1]), float(w[2]), float(w[3])))
            elif len(w) == 2 and w[0].isdigit() and re.match(r"-?\d+\.\d+$", w[1]):
                out["orbital_energies"][int(w[0])] = float(w[1])
        elif section == "cc":
            w = s.split()
            if len(w) == 4 and w[0] == "MP1":
                out["cc_iters"].append((0, float(w[1]), float(w[2]), float(w[3])))
            elif len(w) == 5 and w[0].isdigit():
                out["cc_iters"].append((int(w[0]), float(w[1]), float(w[2]), float(w[3])))
            m = re.match(r"Final CCSD Energy \(Hartree\):\s+(-?\d+\.\d+)", s)
            if m:
                out["final_ccsd"] = float(m.group(1))
        m = re.match(r"MP2 correlation energy \(Hartree\):\s+(-?\d+\.\d+)", s)
        if m:
            out["mp2_line"] = float(m.group(1))
    return out
