"""Reader and sanity checks for the FCIDUMP files the engine writes (afesp_write_fcidump_active / _uactive, include/afesp.h).

Format: a namelist header (&FCI NORB=, NELEC=, MS2=, ORBSYM=, ISYM=, optionally UHF=.TRUE., closed by &END or /), then lines
"value i j k l" with 1-based indices in chemists' notation (ij|kl): two-electron integrals (each unique one once), h(i,j) i j 0 0 and the
core energy with four zeros.  With UHF=.TRUE. NORB counts spin orbitals and the indices are spin-orbital numbers: spatial orbital p
(1-based) is 2p - 1 for alpha and 2p for beta.

`read` returns the two-electron part in this project's own layouts: the 8-fold packed array (inputs.eri_index), and for an open shell the
alpha-alpha and beta-beta packed arrays plus the alpha-beta block as [npair, npair] (row: alpha pair).  `hf_energy`, `fock_diagonal` and
`mp2_energy` evaluate the file as a Hamiltonian in plain numpy: with the orbitals a canonical SCF produced, the first is that SCF's total
energy, the second its orbital energies over the active space, the third the (frozen-core) MP2 correlation energy."""
from __future__ import annotations

import dataclasses
import re

import numpy as np

from .inputs import eri_index, neri, npair


@dataclasses.dataclass
class Fcidump:
    norb: int                       # as the header says: spatial orbitals, or spin orbitals with uhf
    nelec: int
    ms2: int
    uhf: bool
    ecore: float
    h: np.ndarray | None = None     # closed shell: [n, n]
    eri: np.ndarray | None = None   # closed shell: packed, neri(n)
    h_a: np.ndarray | None = None   # open shell: [n, n] each, n = norb // 2 spatial orbitals
    h_b: np.ndarray | None = None
    eri_aa: np.ndarray | None = None
    eri_bb: np.ndarray | None = None
    eri_ab: np.ndarray | None = None   # [npair(n), npair(n)], row: alpha pair
    nlines: int = 0                 # lines after the header

    @property
    def nspatial(self) -> int:
        return self.norb // 2 if self.uhf else self.norb

    @property
    def nalpha(self) -> int:
        return (self.nelec + self.ms2) // 2

    @property
    def nbeta(self) -> int:
        return (self.nelec - self.ms2) // 2


def _header_int(text: str, key: str, default=None) -> int:
    m = re.search(r"\b" + key + r"\s*=\s*(-?\d+)", text, re.I)
    if m is None:
        if default is None:
            raise ValueError(f"FCIDUMP: no {key} in the header")
        return default
    return int(m.group(1))


def _tri(a, b):
    a, b = np.maximum(a, b), np.minimum(a, b)
    return a * (a + 1) // 2 + b


def read(path) -> Fcidump:
    with open(path) as fh:
        head = []
        for line in fh:
            s = line.strip()
            if s.upper().startswith("&END") or s == "/":
                break
            head.append(s)
        else:
            raise ValueError("FCIDUMP: no &END")
        body = fh.read()
    text = " ".join(head)
    if not text.upper().lstrip().startswith("&FCI"):
        raise ValueError("FCIDUMP: no &FCI header")
    norb, nelec, ms2 = _header_int(text, "NORB"), _header_int(text, "NELEC"), _header_int(text, "MS2", 0)
    uhf = re.search(r"\bUHF\s*=\s*\.?T", text, re.I) is not None
    dat = np.array(body.replace("D", "E").split(), dtype=np.float64).reshape(-1, 5) if body.strip() else np.zeros((0, 5))
    val = dat[:, 0]
    idx = dat[:, 1:].astype(np.int64)
    if idx.size and (idx.min() < 0 or idx.max() > norb):
        raise ValueError("FCIDUMP: index outside 0..NORB")
    i, j, k, l = idx.T
    core = (i == 0) & (j == 0) & (k == 0) & (l == 0)
    one = (i > 0) & (j > 0) & (k == 0) & (l == 0)
    two = (i > 0) & (j > 0) & (k > 0) & (l > 0)
    if not np.all(core | one | two):
        raise ValueError("FCIDUMP: a line that is neither a two-electron, a one-electron nor the core-energy line")
    rec = Fcidump(norb, nelec, ms2, uhf, float(val[core].sum()), nlines=len(val))
    if not uhf:
        n = norb
        rec.h = np.zeros((n, n))
        rec.h[i[one] - 1, j[one] - 1] = val[one]
        rec.h[j[one] - 1, i[one] - 1] = val[one]
        rec.eri = np.zeros(neri(n))
        rec.eri[eri_index(i[two] - 1, j[two] - 1, k[two] - 1, l[two] - 1)] = val[two]
        return rec
    if norb % 2:
        raise ValueError("FCIDUMP: UHF=.TRUE. with an odd NORB")
    n = norb // 2
    beta = (idx % 2 == 0) & (idx > 0)            # even spin-orbital numbers are beta
    sp = (idx + 1) // 2 - 1                      # 0-based spatial orbital (-1 for the zeros)
    rec.h_a, rec.h_b = np.zeros((n, n)), np.zeros((n, n))
    if np.any(one & (beta[:, 0] != beta[:, 1])):
        raise ValueError("FCIDUMP: a one-electron element between an alpha and a beta spin orbital")
    for h, sel in ((rec.h_a, one & ~beta[:, 0]), (rec.h_b, one & beta[:, 0])):
        h[sp[sel, 0], sp[sel, 1]] = val[sel]
        h[sp[sel, 1], sp[sel, 0]] = val[sel]
    if np.any(two & ((beta[:, 0] != beta[:, 1]) | (beta[:, 2] != beta[:, 3]))):
        raise ValueError("FCIDUMP: a spin-forbidden two-electron integral")
    rec.eri_aa, rec.eri_bb, rec.eri_ab = np.zeros(neri(n)), np.zeros(neri(n)), np.zeros((npair(n), npair(n)))
    for arr, sel in ((rec.eri_aa, two & ~beta[:, 0] & ~beta[:, 2]), (rec.eri_bb, two & beta[:, 0] & beta[:, 2])):
        arr[eri_index(sp[sel, 0], sp[sel, 1], sp[sel, 2], sp[sel, 3])] = val[sel]
    sel = two & ~beta[:, 0] & beta[:, 2]         # (alpha alpha | beta beta)
    rec.eri_ab[_tri(sp[sel, 0], sp[sel, 1]), _tri(sp[sel, 2], sp[sel, 3])] = val[sel]
    sel = two & beta[:, 0] & ~beta[:, 2]         # the same integral written as (beta beta | alpha alpha)
    rec.eri_ab[_tri(sp[sel, 2], sp[sel, 3]), _tri(sp[sel, 0], sp[sel, 1])] = val[sel]
    return rec


def write(path, h, eri, nelec, ms2=0, ecore=0.0, threshold=0.0) -> int:
    """A restricted FCIDUMP (no UHF flag; ms2 > 0: a restricted open-shell determinant) from h[n, n] and the 8-fold packed eri, every value
    with 17 significant digits (a reader gets the doubles back to the bit); elements with |x| <= threshold are left out.  -> lines after
    the header."""
    h = np.asarray(h, dtype=np.float64)
    n = h.shape[0]
    lines = []
    p, q = np.tril_indices(n)
    pq = p * (p + 1) // 2 + q
    for a in range(len(pq)):
        for b in range(a + 1):
            x = eri[pq[a] * (pq[a] + 1) // 2 + pq[b]]
            if abs(x) > threshold:
                lines.append(f"{x:24.16E} {p[a] + 1:3d} {q[a] + 1:3d} {p[b] + 1:3d} {q[b] + 1:3d}")
    for a in range(len(pq)):
        if abs(h[p[a], q[a]]) > threshold:
            lines.append(f"{h[p[a], q[a]]:24.16E} {p[a] + 1:3d} {q[a] + 1:3d}   0   0")
    lines.append(f"{ecore:24.16E}   0   0   0   0")
    with open(path, "w") as fh:
        fh.write(f" &FCI NORB={n:3d},NELEC={int(nelec):3d},MS2={int(ms2):2d},\n  ORBSYM=" + "1," * n + "\n  ISYM=1,\n &END\n")
        fh.write("\n".join(lines) + "\n")
    return len(lines)


def _coulomb_exchange(eri, n):
    """J(p,i) = (pp|ii), K(p,i) = (pi|pi) of a packed array"""
    p, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return eri[eri_index(p, p, i, i)], eri[eri_index(p, i, p, i)]


def _closed_shell_only(rec):
    if rec.ms2 != 0 or rec.nelec % 2:
        raise ValueError("FCIDUMP: an open shell without UHF=.TRUE. (restricted open-shell orbitals are not supported)")
    return rec.nelec // 2


def hf_energy(rec: Fcidump) -> float:
    """Energy of the determinant that fills the lowest orbitals of the file, core energy included."""
    if not rec.uhf:
        o = _closed_shell_only(rec)
        J, K = _coulomb_exchange(rec.eri, rec.norb)
        return float(rec.ecore + 2.0 * np.trace(rec.h[:o, :o]) + np.sum(2.0 * J[:o, :o] - K[:o, :o]))
    n, na, nb = rec.nspatial, rec.nalpha, rec.nbeta
    Ja, Ka = _coulomb_exchange(rec.eri_aa, n)
    Jb, Kb = _coulomb_exchange(rec.eri_bb, n)
    d = np.arange(n) * (np.arange(n) + 1) // 2 + np.arange(n)      # tri(p, p)
    Jab = rec.eri_ab[np.ix_(d, d)]
    return float(rec.ecore + np.trace(rec.h_a[:na, :na]) + np.trace(rec.h_b[:nb, :nb]) + 0.5 * np.sum(Ja[:na, :na] - Ka[:na, :na])
                 + 0.5 * np.sum(Jb[:nb, :nb] - Kb[:nb, :nb]) + np.sum(Jab[:na, :nb]))


def fock_diagonal(rec: Fcidump):
    """Diagonal of the Fock matrix of that determinant: [n], or ([n] alpha, [n] beta) for an open shell.  With canonical orbitals these
    are the orbital energies."""
    if not rec.uhf:
        o = _closed_shell_only(rec)
        J, K = _coulomb_exchange(rec.eri, rec.norb)
        return np.diag(rec.h) + np.sum(2.0 * J[:, :o] - K[:, :o], axis=1)
    n, na, nb = rec.nspatial, rec.nalpha, rec.nbeta
    Ja, Ka = _coulomb_exchange(rec.eri_aa, n)
    Jb, Kb = _coulomb_exchange(rec.eri_bb, n)
    d = np.arange(n) * (np.arange(n) + 1) // 2 + np.arange(n)
    Jab = rec.eri_ab[np.ix_(d, d)]                                  # (pp|QQ), p alpha, Q beta
    fa = np.diag(rec.h_a) + np.sum(Ja[:, :na] - Ka[:, :na], axis=1) + np.sum(Jab[:, :nb], axis=1)
    fb = np.diag(rec.h_b) + np.sum(Jb[:, :nb] - Kb[:, :nb], axis=1) + np.sum(Jab[:na, :], axis=0)
    return fa, fb


def _ovov(eri, n, o):
    """(ia|jb) of a packed array as [o, v, o, v]"""
    i, a, j, b = np.meshgrid(np.arange(o), np.arange(o, n), np.arange(o), np.arange(o, n), indexing="ij")
    return eri[eri_index(i, a, j, b)]


def mp2_energy(rec: Fcidump) -> float:
    """Second-order correlation energy with fock_diagonal as the orbital energies (canonical orbitals assumed: the off-diagonal Fock
    elements are not looked at)."""
    if not rec.uhf:
        n, o = rec.norb, _closed_shell_only(rec)
        e = fock_diagonal(rec)
        g = _ovov(rec.eri, n, o)
        den = e[:o, None, None, None] - e[None, o:, None, None] + e[None, None, :o, None] - e[None, None, None, o:]
        return float(np.sum(g * (2.0 * g - g.transpose(0, 3, 2, 1)) / den))
    n, na, nb = rec.nspatial, rec.nalpha, rec.nbeta
    ea, eb = fock_diagonal(rec)
    total = 0.0
    for eri, e, o in ((rec.eri_aa, ea, na), (rec.eri_bb, eb, nb)):
        g = _ovov(eri, n, o)
        den = e[:o, None, None, None] - e[None, o:, None, None] + e[None, None, :o, None] - e[None, None, None, o:]
        total += 0.5 * float(np.sum(g * (g - g.transpose(0, 3, 2, 1)) / den))
    i, a, j, b = np.meshgrid(np.arange(na), np.arange(na, n), np.arange(nb), np.arange(nb, n), indexing="ij")
    g = rec.eri_ab[_tri(i, a), _tri(j, b)]
    den = ea[:na, None, None, None] - ea[None, na:, None, None] + eb[None, None, :nb, None] - eb[None, None, None, nb:]
    return total + float(np.sum(g * g / den))
