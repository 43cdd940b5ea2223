"""Numpy side of the FCIDUMP-reader tests: the Fock operator of a file's determinant as plain einsums on the unpacked arrays, and writers
that produce the liberties the reader must accept (index arrangements, separators, exponents, line order)."""
from __future__ import annotations

import numpy as np

import np_fcidump
import np_ucc
from afesp_amd.inputs import npair
from afesp_amd.rhf import unpack_eri


def fock_closed(n, o, h, packed):
    """F(p,q) = h(p,q) + sum_{i < o} [2 (pq|ii) - (pi|qi)]"""
    g = unpack_eri(n, packed)
    return h + 2.0 * np.einsum("pqii->pq", g[:, :, :o, :o]) - np.einsum("piqi->pq", g[:, :o, :, :o])


def fock_open(n, na, nb, h_a, h_b, aa, ab, bb):
    """F_a = h_a + sum_{i in alpha} [(pq|ii) - (pi|qi)]_aa + sum_{I in beta} (pq|II)_ab, F_b the mirror image; ab: [npair, npair]"""
    ga, gb, gab = unpack_eri(n, aa), unpack_eri(n, bb), np_ucc.unpair_matrix(n, ab)
    fa = h_a + np.einsum("pqii->pq", ga[:, :, :na, :na]) - np.einsum("piqi->pq", ga[:, :na, :, :na]) + np.einsum("pqii->pq", gab[:, :, :nb, :nb])
    fb = h_b + np.einsum("pqii->pq", gb[:, :, :nb, :nb]) - np.einsum("piqi->pq", gb[:, :nb, :, :nb]) + np.einsum("iipq->pq", gab[:na, :na, :, :])
    return fa, fb


def chop(x, threshold):
    """what a writer with this threshold leaves of x: everything with |x| <= threshold is zero"""
    return np.where(np.abs(x) > threshold, x, 0.0)


def random_packed(rng, n, scale=1.0):
    from afesp_amd.inputs import neri
    return scale * rng.standard_normal(neri(n))


def sym(rng, n):
    a = rng.standard_normal((n, n))
    return 0.5 * (a + a.T)


def arrangements(i, j, k, l):
    """the 8 equivalent arrangements of (ij|kl)"""
    return [(i, j, k, l), (j, i, k, l), (i, j, l, k), (j, i, l, k), (k, l, i, j), (l, k, i, j), (k, l, j, i), (l, k, j, i)]


def body_records(text):
    """(value string, i, j, k, l) of every body line of a file written by np_fcidump"""
    return [(f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])) for f in (ln.split() for ln in text.split("&END\n")[1].splitlines())]


def liberal_text(rng, n, nelec, records, core=True):
    """The same Hamiltonian written as freely as the format allows: lines shuffled, each two-electron line in a random one of its 8
    arrangements (one-electron lines in either order), D exponents, comma separators on some lines, blank lines (one of them a form
    feed), \\r\\n, lower-case keys over several lines in another order, a / terminator; core=False drops the core-energy line."""
    out = []
    for val, i, j, k, l in records:
        if (i, j, k, l) == (0, 0, 0, 0) and not core:
            continue
        if k > 0:
            i, j, k, l = arrangements(i, j, k, l)[int(rng.integers(8))]
        elif i > 0 and rng.integers(2):
            i, j = j, i
        val = val.replace("E", "D") if rng.integers(2) else val
        style = int(rng.integers(3))
        if style == 0:
            ln = f"  {val}   {i} {j}\t{k}  {l}"
        elif style == 1:
            ln = f"{val},{i},{j},{k},{l}"
        else:
            ln = f" {val} , {i} , {j} ,{k}, {l}  "
        out.append(ln)
        if rng.integers(10) == 0:
            out.append("   ")
    out.append(" \f ")
    order = rng.permutation(len(out))
    head = f"&fci\n  isym = 1,\n nelec = {nelec} ,\n  orbsym=" + "1," * n + f"\n norb={n},\n/\n"
    return (head + "\n".join(out[x] for x in order) + "\n").replace("\n", "\r\n")


def all_arrangements_text(n, nelec, packed, h, ecore):
    """every one of the n^4 arrangements of the two-electron part (agreeing duplicates), h in both triangles"""
    g = unpack_eri(n, packed)
    lines = [np_fcidump.line(g[i, j, k, l], i + 1, j + 1, k + 1, l + 1) for i in range(n) for j in range(n) for k in range(n) for l in range(n)]
    lines += [np_fcidump.line(h[i, j], i + 1, j + 1, 0, 0) for i in range(n) for j in range(n)]
    return np_fcidump.header(n, nelec, 0, False) + "".join(lines) + np_fcidump.line(ecore, 0, 0, 0, 0)
