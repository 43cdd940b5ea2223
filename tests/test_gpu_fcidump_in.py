"""A standard FCIDUMP as input on the GPU (afesp_read_fcidump / _uhf, Engine.read_fcidump): round trips through the engine's own writer,
the Fock kernels against plain einsums (np_fcidump_in.py), the parser and the scatter on hand-written files in every liberty the format
allows, duplicates, refusals, and three-digit indices.  afesp_amd/fcidump.py (numpy) is the independent statement of the format."""
import dataclasses
import os

import numpy as np
import pytest

import molecules
import np_fcidump
import np_fcidump_in as nfi
from afesp_amd import capi, fcidump, inputs, rhf, uhf
from test_gpu_frozen import _random_system, _v_oovv

pytestmark = pytest.mark.gpu
TIGHT = dict(scf_e_tol=1e-13, scf_d_tol=1e-11, scf_maxiter=300, scf_read_guess=False)


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def water():
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    res = rhf.do_rhf(dataclasses.replace(si, **TIGHT), ints)
    assert res.converged
    return ints, res


@pytest.mark.parametrize("nfc,windowed", [(1, True), (0, False)])
def test_closed_shell_round_trip(eng, water, tmp_path, nfc, windowed):
    """H2O/cc-pVDZ written by afesp_write_fcidump_active (threshold 0) and read back: arrays to the bit against fcidump.read; levels and
    e_ref against the SCF to 1e-9 (what the SCF convergence leaves, as in test_gpu_fcidump.py); then CCSD and (T) from the file against the
    direct route to 1e-8 Eh (the parity bar of README.md)."""
    ints, res = water
    n, o, lev = ints.nbasis, ints.nel // 2, res.canon_levels
    v = n - o
    eng.do_mp2_spatial(n, o, res.canon_coeff, lev, ints.eri, want_eri_mo=False)
    h_act, e_core = eng.core_operator(n, nfc, 0, res.canon_coeff, ints.core_hamil)
    if windowed:
        eng.mo_window(n, o, nfc, 0, lev, want_eri=False)
    eng.ccsd_init(o - nfc, v, lev[nfc:], None, 8)                     # the direct route
    nit, en, _ = eng.do_ccsd_spatial(60, 1e-10, 1e-10)
    e_direct, t_direct = en[nit], eng.do_ccsd_t_spatial()
    path = tmp_path / "FCIDUMP"
    nw = eng.write_fcidump_active(path, n - nfc, ints.nel - 2 * nfc, 0, h_act, e_core + ints.e_nuc, 0.0)
    rec = fcidump.read(path)
    got = eng.read_fcidump(path, want_eri=True)
    assert (got.norb, got.nelec, got.ms2, got.uhf, got.nread) == (n - nfc, ints.nel - 2 * nfc, 0, False, nw)
    assert np.array_equal(got.eri, rec.eri) and np.array_equal(got.h, rec.h) and got.e_core == rec.ecore
    print(f"nfc={nfc}: levels {np.max(np.abs(got.levels - lev[nfc:])):.2e}, e_ref {abs(got.e_ref - (res.e_hf + ints.e_nuc)):.2e}, "
          f"fock_offdiag {got.fock_offdiag:.2e}")
    assert np.max(np.abs(got.levels - lev[nfc:])) < 1e-9
    assert abs(got.e_ref - (res.e_hf + ints.e_nuc)) < 1e-9
    assert np.array_equal(got.fock, got.fock.T) and np.array_equal(np.diag(got.fock), got.levels)
    assert got.fock_offdiag < 1e-6
    eng.ccsd_init(o - nfc, v, got.levels, None, 8)                     # from the file
    nit2, en2, _ = eng.do_ccsd_spatial(60, 1e-10, 1e-10)
    t_file = eng.do_ccsd_t_spatial()
    print(f"nfc={nfc}: E(CCSD) gap {abs(en2[nit2] - e_direct):.2e}, E[T] gap {abs(t_file[0] - t_direct[0]):.2e}, "
          f"E(T) gap {abs(t_file[1] - t_direct[1]):.2e}")
    assert abs(en2[nit2] - e_direct) < 1e-8
    assert abs(t_file[0] - t_direct[0]) < 1e-8 and abs(t_file[1] - t_direct[1]) < 1e-8


def _rewrite_ab_swapped_and_shuffled(text, rng):
    head, body = text.split("&END\n")
    lines = body.splitlines()
    out = []
    for ln in lines:
        f = ln.split()
        i, j, k, l = (int(x) for x in f[1:])
        if k > 0 and i % 2 == 1 and k % 2 == 0:                        # (aa|bb) -> (bb|aa)
            ln = np_fcidump.line(0.0, k, l, i, j).replace("%23.15E" % 0.0, f[0].rjust(23)).rstrip("\n")
        out.append(ln)
    return head + "&END\n" + "\n".join(out[x] for x in rng.permutation(len(out))) + "\n"


def test_open_shell_round_trip(eng, tmp_path):
    """The doublet H2O+ with nfc = 1: blocks to the bit, levels and e_ref to 1e-9, E(UMP2) of a (0, 0) window and the MP1 line of the
    spin-orbital solver to 1e-10 against the direct route; the same file with (bb|aa) lines and shuffled gives the same bits."""
    nfc = 1
    si, ints, _, _ = molecules.load("h2o-cc-pvdz")
    si = dataclasses.replace(si, charge=1, multiplicity=2, **TIGHT)
    n = ints.nbasis
    na, nb = inputs.spin_counts(si, ints.nel, n)
    eng.set_eri(n, ints.eri)
    u = uhf.do_uhf(si, ints, na, nb, None, lambda da, db: eng.build_fock_uhf(n, da, db, ints.core_hamil))
    assert u.converged
    eng.do_ump2(n, na, nb, u.coeff_a, u.coeff_b, u.levels_a, u.levels_b, None, want_eri_mo=False)
    ha, hb, e_core = eng.ucore_operator(n, nfc, 0, u.coeff_a, u.coeff_b, ints.core_hamil)
    *_, e2_direct = eng.umo_window(n, na, nb, nfc, 0, u.levels_a, u.levels_b, want_eri=False)
    m, oa, ob = n - nfc, na - nfc, nb - nfc
    eng.init_cc_uspinorb(m, oa, ob, u.levels_a[nfc:], u.levels_b[nfc:])
    mp1_direct = eng.so_energy()[0]
    path = tmp_path / "FCIDUMP"
    nw = eng.write_fcidump_uactive(path, m, oa, ob, ha, hb, e_core + ints.e_nuc, 0.0)
    rec = fcidump.read(path)
    got = eng.read_fcidump(path, want_eri=True)
    assert (got.norb, got.nelec, got.ms2, got.uhf, got.nread, got.nalpha, got.nbeta) == (2 * m, oa + ob, oa - ob, True, nw, oa, ob)
    for a, b in ((got.eri_aa, rec.eri_aa), (got.eri_bb, rec.eri_bb), (got.eri_ab, rec.eri_ab), (got.h_a, rec.h_a), (got.h_b, rec.h_b)):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert got.e_core == rec.ecore
    print(f"H2O+: levels {np.max(np.abs(got.levels_a - u.levels_a[nfc:])):.2e} {np.max(np.abs(got.levels_b - u.levels_b[nfc:])):.2e}, "
          f"e_ref {abs(got.e_ref - (u.e_hf + ints.e_nuc)):.2e}, fock_offdiag {got.fock_offdiag:.2e}")
    assert np.max(np.abs(got.levels_a - u.levels_a[nfc:])) < 1e-9 and np.max(np.abs(got.levels_b - u.levels_b[nfc:])) < 1e-9
    assert abs(got.e_ref - (u.e_hf + ints.e_nuc)) < 1e-9
    assert np.array_equal(got.fock_a, got.fock_a.T) and np.array_equal(got.fock_b, got.fock_b.T)
    *_, e2_file = eng.umo_window(m, oa, ob, 0, 0, got.levels_a, got.levels_b, want_eri=False)
    eng.init_cc_uspinorb(m, oa, ob, got.levels_a, got.levels_b)
    mp1_file = eng.so_energy()[0]
    print(f"H2O+: E(UMP2) gap {abs(e2_file - e2_direct):.2e}, MP1 gap {abs(mp1_file - mp1_direct):.2e}")
    assert abs(e2_file - e2_direct) < 1e-10 and abs(mp1_file - mp1_direct) < 1e-10
    other = tmp_path / "swapped"
    other.write_text(_rewrite_ab_swapped_and_shuffled(path.read_text(), np.random.default_rng(3)))
    again = eng.read_fcidump(other, want_eri=True)
    for a, b in ((again.eri_aa, got.eri_aa), (again.eri_bb, got.eri_bb), (again.eri_ab, got.eri_ab), (again.h_a, got.h_a),
                 (again.h_b, got.h_b), (again.fock_a, got.fock_a), (again.fock_b, got.fock_b)):
        assert np.array_equal(a, b)
    assert again.e_core == got.e_core and again.e_ref == got.e_ref


@pytest.mark.parametrize("n,o,threshold", [(12, 3, 0.0), (72, 68, 0.11)])
def test_fock_kernel_against_numpy(eng, tmp_path, n, o, threshold):
    """Random 8-fold-symmetric integrals (sigma 0.05) and a random symmetric h written as a file; F against the einsum on the unpacked
    array to 1e-11 of its largest element (the bound of test_core_operator_matches_numpy: sums of <= 3 o products in a fixed order).
    n = 72, o = 68: the occupied loop passes one wave's 64 lanes; the threshold (2.2 sigma: 2.8 % of 3.5e6) keeps the file near 1e5
    lines, and the reference is evaluated on what fcidump.read makes of the same file (the thresholded array, as its 16 digits read back)."""
    rng = np.random.default_rng(n)
    packed = nfi.random_packed(rng, n, 0.05)
    i = np.arange(n)
    packed[inputs.eri_index(i[:, None], i[:, None], i[None, :], i[None, :])] += 0.5         # (pp|ii): every lane of the loop has work
    packed[inputs.eri_index(i[:, None], i[None, :], i[:, None], i[None, :])] += 0.25        # (pi|pi)
    packed, h = nfi.chop(packed, threshold), nfi.sym(rng, n)
    path = tmp_path / "FCIDUMP"
    path.write_text(np_fcidump.dump_text(n, 2 * o, 0, packed, h, 1.5, 0.0))
    got = eng.read_fcidump(path, canonical_tol=None, want_eri=True)
    rec = fcidump.read(path)
    packed, h = rec.eri, rec.h
    ref = nfi.fock_closed(n, o, h, packed)
    scale = np.max(np.abs(ref))
    print(f"n={n} o={o}: {got.nread} lines, |F - F_ref| {np.max(np.abs(got.fock - ref)) / scale:.2e} of {scale:.3f}")
    assert np.array_equal(got.eri, packed) and np.array_equal(got.h, h) and got.e_core == 1.5
    assert np.array_equal(got.fock, got.fock.T)
    assert np.max(np.abs(got.fock - ref)) < 1e-11 * scale
    e_ref = 1.5 + np.trace(h[:o, :o]) + np.trace(ref[:o, :o])
    assert abs(got.e_ref - e_ref) < 1e-11 * max(1.0, abs(e_ref)) * o
    assert got.fock_offdiag == np.max(np.abs(got.fock - np.diag(np.diag(got.fock))))


def test_open_shell_fock_kernel_against_numpy(eng, tmp_path):
    """n = 10, na = 4, nb = 2 with three independent blocks; and na = nb with equal blocks, where both spins' operators are equal to the bit"""
    n, na, nb, rng = 10, 4, 2, np.random.default_rng(10)
    aa, bb = nfi.random_packed(rng, n), nfi.random_packed(rng, n)
    ab = rng.standard_normal((inputs.npair(n), inputs.npair(n)))
    ha, hb = nfi.sym(rng, n), nfi.sym(rng, n)
    path = tmp_path / "FCIDUMP"
    path.write_text(np_fcidump.udump_text(n, na, nb, aa, ab, bb, ha, hb, -0.5))
    got = eng.read_fcidump(path, canonical_tol=None, want_eri=True)
    rec = fcidump.read(path)
    aa, bb, ab, ha, hb = rec.eri_aa, rec.eri_bb, rec.eri_ab, rec.h_a, rec.h_b
    ra, rb = nfi.fock_open(n, na, nb, ha, hb, aa, ab, bb)
    scale = max(np.max(np.abs(ra)), np.max(np.abs(rb)))
    print(f"open shell: |F_a - ref| {np.max(np.abs(got.fock_a - ra)) / scale:.2e}, |F_b - ref| {np.max(np.abs(got.fock_b - rb)) / scale:.2e}")
    assert np.array_equal(got.eri_aa, aa) and np.array_equal(got.eri_bb, bb) and np.array_equal(got.eri_ab, ab)
    assert np.max(np.abs(got.fock_a - ra)) < 1e-11 * scale and np.max(np.abs(got.fock_b - rb)) < 1e-11 * scale
    assert np.array_equal(got.fock_a, got.fock_a.T) and np.array_equal(got.fock_b, got.fock_b.T)
    e_ref = -0.5 + 0.5 * (np.trace(ha[:na, :na]) + np.trace(ra[:na, :na])) + 0.5 * (np.trace(hb[:nb, :nb]) + np.trace(rb[:nb, :nb]))
    assert abs(got.e_ref - e_ref) < 1e-11 * scale * n
    assert got.fock_offdiag == max(np.max(np.abs(f - np.diag(np.diag(f)))) for f in (got.fock_a, got.fock_b))
    import np_ucc
    pm = np_ucc.pair_matrix(rhf.unpack_eri(n, aa))
    path.write_text(np_fcidump.udump_text(n, 3, 3, aa, pm, aa, ha, ha, 0.0))
    eq = eng.read_fcidump(path, canonical_tol=None)
    assert np.array_equal(eq.fock_a, eq.fock_b) and np.array_equal(eq.levels_a, eq.levels_b)


# ---- the parser and the scatter on hand-written files, n = 7
N7, O7 = 7, 2


@pytest.fixture(scope="module")
def seven():
    rng = np.random.default_rng(7)
    packed, h = nfi.random_packed(rng, N7), nfi.sym(rng, N7)
    packed[[5, 40]] = 0.0
    text = np_fcidump.dump_text(N7, 2 * O7, 0, packed, h, -3.25)
    return packed, h, text


def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("eri", "h", "fock", "levels")) and a.e_ref == b.e_ref


@pytest.mark.parametrize("chunk_kib", [None, "1"])
def test_liberal_files_give_the_canonical_array(eng, seven, tmp_path, monkeypatch, chunk_kib):
    """(a) shuffled lines, random arrangements, D exponents, commas, blank lines, \\r\\n, a / terminator, no core-energy line; (b) all n^4
    arrangements with agreeing duplicates; (c) both again with AFESP_FCIDUMP_CHUNK_KIB=1: every chunk end cuts a line."""
    packed, h, text = seven
    canon = tmp_path / "canon"
    canon.write_text(text)
    base = eng.read_fcidump(canon, canonical_tol=None, want_eri=True)          # (the default chunk size)
    rec = fcidump.read(canon)
    assert np.array_equal(base.eri, rec.eri) and np.array_equal(base.h, rec.h) and base.e_core == -3.25
    assert np.count_nonzero(base.eri) == inputs.neri(N7) - 2
    if chunk_kib:
        monkeypatch.setenv("AFESP_FCIDUMP_CHUNK_KIB", chunk_kib)
        assert os.path.getsize(canon) > 16 * 1024
        assert _same(eng.read_fcidump(canon, canonical_tol=None, want_eri=True), base)
    lib = tmp_path / "liberal"
    lib.write_bytes(nfi.liberal_text(np.random.default_rng(70), N7, 2 * O7, nfi.body_records(text), core=False).encode())
    got = eng.read_fcidump(lib, canonical_tol=None, want_eri=True)
    assert got.e_core == 0.0 and got.nread == base.nread - 1 == capi.scan_fcidump(lib).nlines   # (the scan and the reader count alike)
    assert np.array_equal(got.eri, base.eri) and np.array_equal(got.h, base.h) and np.array_equal(got.fock, base.fock)
    assert abs(got.e_ref - (base.e_ref + 3.25)) < 1e-12
    every = tmp_path / "all"
    every.write_text(nfi.all_arrangements_text(N7, 2 * O7, packed, h, -3.25))
    got = eng.read_fcidump(every, canonical_tol=None, want_eri=True)
    assert got.nread == N7 ** 4 + N7 * N7 + 1 and _same(got, base)


def test_refusals_leave_the_resident_integrals_untouched(seven, tmp_path, monkeypatch):
    """Status 1 with a message (and the line number) for every kind of bad file, at the default chunk size and at 1 KiB; afterwards
    ccsd_init(NULL) still reads the integrals that were resident before."""
    packed, h, text = seven
    n, o = 24, 4
    eri, c, lev = _random_system(n, o, 3)
    head, body = text.split("&END\n")
    lines = body.splitlines()
    nh = head.count("\n") + 1                                       # lines of the header
    dup = lines[10].split()
    conflict = np_fcidump.line(float(dup[0]) + 1e-9, *(int(x) for x in dup[1:])).rstrip("\n")
    agree = lines[10]
    one = next(ln.split() for ln in lines if ln.split()[3] == "0" and ln.split()[1] != ln.split()[2])
    one_conflict = np_fcidump.line(float(one[0]) + 1e-9, int(one[2]), int(one[1]), 0, 0).rstrip("\n")   # h(j,i) against h(i,j), one chunk

    def at(k, ln):
        return head + "&END\n" + "\n".join(lines[:k] + [ln] + lines[k:]) + "\n"
    cases = {
        "conflict_near": (at(12, conflict), "disagrees", None),
        "conflict_far": (at(len(lines) - 3, conflict), "disagrees", None),
        "index": (at(5, np_fcidump.line(0.5, N7 + 1, 1, 1, 1).rstrip("\n")), "outside 0..NORB", nh + 6),
        "field": (at(5, "  0.5 1 x 1 1"), "malformed", nh + 6),
        "value": (at(5, "  0.5q 1 1 1 1"), "malformed", nh + 6),
        "short": (at(5, "  0.5 1 1 1"), "malformed", nh + 6),
        "overflow": (at(5, "  1E999 1 1 1 1"), "malformed", nh + 6),      # (strtod gives inf: no value)
        "one_electron": (at(len(lines) - 1, one_conflict), "disagrees", None),
        "kind": (at(5, "  0.5 1 1 1 0"), "neither", nh + 6),
        "nelec": (text.replace(f"NELEC={2 * O7}", f"NELEC={2 * O7 + 1}"), "open shell|disagrees", None),
        "two_core": (at(7, np_fcidump.line(1.0, 0, 0, 0, 0).rstrip("\n")), "more than one core-energy", len(lines) + nh + 1),
        "no_header": (body, "FCI", None),
        "no_end": (head, "FCI|header", None),
    }
    with capi.Engine(0) as e:
        e.do_mp2_spatial(n, o, c, lev, eri, want_eri_mo=False)
        e.ccsd_init(o, n - o, lev, None, 4)
        before = e.tensor("v_oovv")
        for chunk in (None, "1"):
            if chunk:
                monkeypatch.setenv("AFESP_FCIDUMP_CHUNK_KIB", chunk)
            for name, (content, msg, line) in cases.items():
                path = tmp_path / name
                path.write_text(content)
                with pytest.raises(capi.AfespError, match="status 1") as err:
                    e.read_fcidump(path, canonical_tol=None)
                import re
                assert re.search(msg, str(err.value)), (name, str(err.value))
                if line is not None:
                    assert f"line {line}:" in str(err.value), (name, line, str(err.value))
            e.ccsd_init(o, n - o, lev, None, 4)
            assert np.array_equal(e.tensor("v_oovv"), before)
        # the header disagreeing with the arguments of the C call itself; a NULL path; a missing file
        path = tmp_path / "canon"
        path.write_text(text)
        assert e.L.afesp_read_fcidump(e.h, str(path).encode(), N7, O7 + 1, None, None, None, None, None, None, None, None) == 1
        assert "disagrees" in e.L.afesp_last_error(e.h).decode()
        assert e.L.afesp_read_fcidump(e.h, None, N7, O7, None, None, None, None, None, None, None, None) == 1
        assert e.L.afesp_read_fcidump(e.h, str(tmp_path / "missing").encode(), N7, O7, None, None, None, None, None, None, None, None) == 1
        assert e.L.afesp_read_fcidump_uhf(e.h, str(path).encode(), N7, O7, O7, *([None] * 14)) == 1   # a closed-shell file
        # a UHF file with a one-electron line between an alpha and a beta spin orbital
        rng = np.random.default_rng(8)
        utext = np_fcidump.udump_text(3, 2, 1, nfi.random_packed(rng, 3), rng.standard_normal((6, 6)), nfi.random_packed(rng, 3),
                                      nfi.sym(rng, 3), nfi.sym(rng, 3), 0.5)
        up = tmp_path / "uhf"
        up.write_text(utext + np_fcidump.line(0.1, 1, 2, 0, 0))
        with pytest.raises(capi.AfespError, match="between an alpha and a beta"):
            e.read_fcidump(up, canonical_tol=None)
        up.write_text(utext + np_fcidump.line(0.1, 1, 2, 1, 1))
        with pytest.raises(capi.AfespError, match="spin-forbidden"):
            e.read_fcidump(up, canonical_tol=None)
        e.ccsd_init(o, n - o, lev, None, 4)
        assert np.array_equal(e.tensor("v_oovv"), before)
        # non-canonical orbitals: reported, refused by the caller above the tolerance -- and a good file replaces what was resident
        with pytest.raises(capi.AfespError, match="not canonical"):
            e.read_fcidump(path)
        got = e.read_fcidump(path, canonical_tol=None)
        e.ccsd_init(O7, N7 - O7, got.levels, None, 4)
        assert np.array_equal(e.tensor("v_oovv"), _v_oovv(O7, N7 - O7, fcidump.read(path).eri))
        ok = tmp_path / "ok"
        ok.write_text(at(12, agree))                                   # a duplicate that agrees is no error
        twice = e.read_fcidump(ok, canonical_tol=None, want_eri=True)
        assert twice.nread == got.nread + 1 and np.array_equal(twice.eri, fcidump.read(path).eri)


def test_conflicting_duplicates_are_found_within_and_across_chunks(seven, tmp_path, monkeypatch):
    """The two lines 2 lines apart (one chunk at any setting) and more than 16 KiB apart at the 1 KiB setting (different chunks, the
    first one's chunk long gone); the smallest offending line is named: within a chunk either of the two, across chunks the later one."""
    packed, h, text = seven
    head, body = text.split("&END\n")
    lines = body.splitlines()
    nh = head.count("\n") + 1
    f = lines[3].split()
    m, x = f[0].split("E")
    off = m[:-1] + ("1" if m[-1] == "0" else "0") + "E" + x            # the last digit written differs, in another arrangement
    assert float(off) != float(f[0])
    bad = f" {off} {f[2]} {f[1]} {f[4]} {f[3]}"
    monkeypatch.setenv("AFESP_FCIDUMP_CHUNK_KIB", "1")
    with capi.Engine(0) as e:
        for k, want in ((5, (nh + 4, nh + 6)), (len(lines) - 2, (nh + len(lines) - 1,))):
            path = tmp_path / f"dup{k}"
            path.write_text(head + "&END\n" + "\n".join(lines[:k] + [bad] + lines[k:]) + "\n")
            with pytest.raises(capi.AfespError, match="status 1") as err:
                e.read_fcidump(path, canonical_tol=None)
            assert "disagrees" in str(err.value) and any(f"line {w}:" in str(err.value) for w in want), str(err.value)


def test_three_digit_indices(eng, tmp_path):
    """n = 100, the thresholded file of test_compaction_at_three_digit_indices' kind (2.6 sigma: about 1.2e5 of 1.3e7 integrals): the array read back equals fcidump.read's to the bit."""
    n, rng = 100, np.random.default_rng(100)
    packed = 0.05 * rng.standard_normal(inputs.neri(n))
    packed[-1] = 1.0
    h = np.zeros((n, n))
    h[n - 1, 0] = h[0, n - 1] = 0.5
    lev = np.concatenate([-2.0 - np.arange(3), 1.0 + np.arange(n - 3)])
    eng.mo_window(n, 3, 0, 0, lev, eri_mo=packed, want_eri=False)
    path = tmp_path / "FCIDUMP"
    nw = eng.write_fcidump_active(path, n, 6, 0, h, 0.0, 0.13)        # 2.6 sigma: about 1.2e5 lines
    rec = fcidump.read(path)
    import time
    t0 = time.perf_counter()
    got = eng.read_fcidump(path, canonical_tol=None, want_eri=True)
    dt = time.perf_counter() - t0
    print(f"n=100: {nw} lines, {os.path.getsize(path) / 1e6:.1f} MB read in {dt * 1e3:.0f} ms")
    assert got.nread == nw and 5e4 < nw < 4e5
    assert np.array_equal(got.eri, rec.eri) and np.array_equal(got.h, rec.h) and got.e_core == 0.0
    assert got.eri[-1] == 1.0 and got.h[n - 1, 0] == 0.5
