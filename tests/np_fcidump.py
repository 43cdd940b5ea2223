"""Numpy restatement of the frozen-core operator and core energy (afesp_core_operator / afesp_ucore_operator) on packed MO integrals, and
a plain-Python writer of the FCIDUMP format of afesp_write_fcidump_active / _uactive.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

from afesp_amd.inputs import eri_index, npair
from np_window import _pairs, tri


def core_operator(n, nfc, nfv, h_mo, packed, one_spin=False):
    """-> (h_act, e_core): closed shell h_mo + sum_c [2 (pq|cc) - (pc|qc)], 2 sum_c h_cc + sum_cd [2 (cc|dd) - (cd|cd)];
    one_spin: the same-spin share of an open shell, h_mo + sum_c [(pq|cc) - (pc|qc)], sum_c h_cc + 1/2 sum_cd [(cc|dd) - (cd|cd)]"""
    hi = n - nfv
    h_mo = 0.5 * (h_mo + h_mo.T)
    wj, eh, e2 = (1.0, 1.0, 0.5) if one_spin else (2.0, 2.0, 1.0)
    P, Q, C = np.meshgrid(np.arange(nfc, hi), np.arange(nfc, hi), np.arange(nfc), indexing="ij")
    h_act = h_mo[nfc:hi, nfc:hi] + np.sum(wj * packed[eri_index(P, Q, C, C)] - packed[eri_index(P, C, Q, C)], axis=2)
    c, d = np.meshgrid(np.arange(nfc), np.arange(nfc), indexing="ij")
    e_core = eh * np.trace(h_mo[:nfc, :nfc]) + e2 * np.sum(wj * packed[eri_index(c, c, d, d)] - packed[eri_index(c, d, c, d)])
    return h_act, float(e_core)


def ucore_operator(n, nfc, nfv, h_mo_a, h_mo_b, aa, ab, bb):
    """-> (h_act_a, h_act_b, e_core); ab is the [npair, npair] block, row: alpha pair"""
    hi = n - nfv
    ha, ea = core_operator(n, nfc, nfv, h_mo_a, aa, one_spin=True)
    hb, eb = core_operator(n, nfc, nfv, h_mo_b, bb, one_spin=True)
    P, Q = np.meshgrid(np.arange(nfc, hi), np.arange(nfc, hi), indexing="ij")
    cc = tri(np.arange(nfc), np.arange(nfc))
    ha = ha + np.sum(ab[tri(P, Q)[:, :, None], cc[None, None, :]], axis=2)
    hb = hb + np.sum(ab[cc[None, None, :], tri(P, Q)[:, :, None]], axis=2)
    return ha, hb, float(ea + eb + np.sum(ab[np.ix_(cc, cc)]))


def line(value, i, j, k, l):
    return "%23.15E %4d %4d %4d %4d\n" % (value, i, j, k, l)


def header(norb, nelec, ms2, uhf):
    return (f" &FCI NORB={norb},NELEC={nelec},MS2={ms2},\n  ORBSYM=" + "1," * norb + "\n  ISYM=1,\n" + ("  UHF=.TRUE.,\n" if uhf else "")
            + " &END\n")


def two_electron_lines(n, packed, threshold, block="spatial"):
    """the lines of a packed array (block "spatial", "aa", "bb") or of the [npair, npair] matrix ("ab") with |x| > threshold, in order"""
    p, q = _pairs(n)
    if block == "ab":
        flat = np.asarray(packed).ravel()
        keep = np.nonzero(np.abs(flat) > threshold)[0]
        pq, rs = keep // npair(n), keep % npair(n)
    else:
        flat = packed
        keep = np.nonzero(np.abs(flat) > threshold)[0]
        PQ, RS = _pairs(npair(n))
        pq, rs = PQ[keep], RS[keep]
    lab12 = {"spatial": lambda x: x + 1, "aa": lambda x: 2 * x + 1, "bb": lambda x: 2 * x + 2, "ab": lambda x: 2 * x + 1}[block]
    lab34 = {"spatial": lambda x: x + 1, "aa": lambda x: 2 * x + 1, "bb": lambda x: 2 * x + 2, "ab": lambda x: 2 * x + 2}[block]
    return [line(v, a, b, c, d) for v, a, b, c, d in zip(flat[keep], lab12(p[pq]), lab12(q[pq]), lab34(p[rs]), lab34(q[rs]))]


def one_electron_lines(h, threshold, spin=None):
    lab = {None: lambda x: x + 1, "a": lambda x: 2 * x + 1, "b": lambda x: 2 * x + 2}[spin]
    n = h.shape[0]
    return [line(h[i, j], lab(i), lab(j), 0, 0) for i in range(n) for j in range(i + 1) if abs(h[i, j]) > threshold]


def dump_text(n, nelec, ms2, packed, h, ecore, threshold=0.0):
    """the whole closed-shell file as afesp_write_fcidump_active writes it"""
    return (header(n, nelec, ms2, False) + "".join(two_electron_lines(n, packed, threshold)) + "".join(one_electron_lines(h, threshold))
            + line(ecore, 0, 0, 0, 0))


def udump_text(n, nalpha, nbeta, aa, ab, bb, h_a, h_b, ecore, threshold=0.0):
    """the whole open-shell file as afesp_write_fcidump_uactive writes it"""
    return (header(2 * n, nalpha + nbeta, nalpha - nbeta, True) + "".join(two_electron_lines(n, aa, threshold, "aa"))
            + "".join(two_electron_lines(n, bb, threshold, "bb")) + "".join(two_electron_lines(n, ab, threshold, "ab"))
            + "".join(one_electron_lines(h_a, threshold, "a")) + "".join(one_electron_lines(h_b, threshold, "b")) + line(ecore, 0, 0, 0, 0))
