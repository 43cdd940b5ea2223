"""Numpy restatement of the active orbital window [lo, hi) = [nfc, n - nfv) of MO integrals (frozen core / frozen virtuals).

With canonical orbitals the Fock matrix of the active space is diagonal with the same orbital energies, so a frozen-core
MP2 / CCSD / (T) calculation is the unchanged solver on the MO integrals whose four indices all lie in the window, with
levels[lo:hi].  Test infrastructure only."""
from __future__ import annotations

import numpy as np


def tri(p, q):
    p, q = np.maximum(p, q), np.minimum(p, q)
    return p * (p + 1) // 2 + q


def npair(n):
    return n * (n + 1) // 2


def neri(n):
    return npair(npair(n))


def _pairs(n):
    """(p, q) of every pair index tri(p, q), p >= q, in order."""
    p = np.repeat(np.arange(n), np.arange(1, n + 1))
    q = np.arange(npair(n)) - p * (p + 1) // 2
    return p, q


def window_packed(n, nfc, nfv, eri_packed):
    """8-fold packed over n orbitals -> 8-fold packed over the n - nfc - nfv active ones: dst[ijkl(p,q,r,s)] = src[ijkl(p+lo, ...)]."""
    na = n - nfc - nfv
    assert na > 0 and eri_packed.shape == (neri(n),)
    p, q = _pairs(na)
    big = tri(p + nfc, q + nfc)                   # the pair indices of the active pairs in the full basis
    pq, rs = _pairs(npair(na))                    # (PQ, RS), PQ >= RS, of every packed element
    return np.ascontiguousarray(eri_packed[tri(big[pq], big[rs])])


def window_full(nfc, nfv, full):
    """The same on a full n^4 array (np_ucc.mo_blocks): every index restricted to the window."""
    hi = full.shape[0] - nfv
    return np.ascontiguousarray(full[nfc:hi, nfc:hi, nfc:hi, nfc:hi])


def window_pair_matrix(n, nfc, nfv, ab):
    """The [npair x npair] alpha-beta matrix (np_ucc.pair_matrix) over n orbitals -> over the active ones."""
    na = n - nfc - nfv
    p, q = _pairs(na)
    big = tri(p + nfc, q + nfc)
    return np.ascontiguousarray(ab[np.ix_(big, big)])


def window_levels(n, nfc, nfv, levels):
    return np.ascontiguousarray(np.asarray(levels)[nfc:n - nfv])


def decouple(n, eri_packed, orbitals):
    """A copy of the packed integrals with every element that touches one of `orbitals` set to zero: those orbitals then take no
    part in the correlation, and the full calculation equals the one on the window without them."""
    out = eri_packed.copy()
    pq, rs = _pairs(npair(n))
    p, q = _pairs(n)
    hit = np.isin(p, orbitals) | np.isin(q, orbitals)
    out[hit[pq] | hit[rs]] = 0.0
    return out
