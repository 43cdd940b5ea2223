"""Every instantiation of the gather-GEMM kernel (csrc/gett.hip) and every branch of its planner (csrc/contract.hip), one by one.

The cases come from tests/np_gett.py: integer operands, so that the result must equal an int64 einsum bit for bit in whatever order the
kernel sums, and for each case the statement of which kernel it is for -- tile code, 8- or 16-byte staging, operand layouts, K slices.
AFESP_GETT_DEBUG=1 makes the launcher print what it launched; each test parses that line and compares it with the statement, so a case
that ran on another kernel than intended fails instead of passing for the wrong reason."""
import contextlib
import re

import numpy as np
import pytest

import np_gett as G

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"gett_launch M (\d+) N (\d+) K (\d+) batch (\d+) akc (\d) bkc (\d) wide (\d) -> tm (\d+) tn (\d+) tiles (\d+) x (\d+) "
                    r"split (\d+) sk (\d) \(steps per slice (\d+)\)")
GRID = re.compile(r"gett_grid (\d+) workgroups for (\d+) tiles gm (\d+)")
_FIELDS = ("M", "N", "K", "batch", "akc", "bkc", "wide", "tm", "tn", "mtiles", "ntiles", "split", "sk", "steps")


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.set_tuning()
    e.close()


@contextlib.contextmanager
def tuning(eng, **kw):
    """afesp_set_tuning is process-wide: whatever a test sets, it puts back."""
    eng.set_tuning(**kw)
    try:
        yield
    finally:
        eng.set_tuning(0, 0, 0, 0)


def launches(capfd):
    """The launcher's lines since the last look: ([fields of each gett_launch line], [(workgroups, tiles, gm) of each gett_grid line])."""
    err = capfd.readouterr().err
    return ([dict(zip(_FIELDS, map(int, m.groups()))) for m in LAUNCH.finditer(err)], [tuple(map(int, m.groups())) for m in GRID.finditer(err)],
            err)


def one_launch(capfd):
    ls, gs, err = launches(capfd)
    assert len(ls) == 1, f"expected one gett_launch line, got: {err!r}"
    return ls[0], gs


def run_int_case(eng, capfd, c, cache):
    """One integer case through eng.contract with its forced tile code and split; the launch line against the case, the result exact."""
    sa, sb, sc = c.shapes()
    if cache.get("seed") != c.ab_seed:
        A, B = G.int_operands(sa, sb, c.ab_seed)
        cache.update(seed=c.ab_seed, A=A, B=B, prod=G.int_product(c.la, A, c.lb, B, c.lc))
    C0 = G.int_c0(sc, c.beta, c.c_seed)
    G.check_exactness_bound(c.k, c.alpha, c.beta, C0)
    ref = G.int_reference(cache["prod"], c.alpha, c.beta, C0)
    got = eng.contract(c.alpha, cache["A"], c.la, cache["B"], c.lb, c.beta, C0, c.lc, force_split=c.force_split, force_tm=c.code[0],
                       force_tn=c.code[1])
    line, _ = one_launch(capfd)
    want = dict(M=c.Mk, N=c.Nk, K=c.k, tm=c.code[0], tn=c.code[1], wide=c.wide, akc=c.akc, bkc=c.bkc, split=c.split, sk=0)
    assert {k: line[k] for k in want} == want, c
    bad = int(np.sum(got != ref))
    assert bad == 0, f"{bad} of {ref.size} elements differ (first at {np.argwhere(got != ref)[0]}): {c}"
    return line


@pytest.mark.parametrize("code,staging", [(c, w) for c in G.TILE_CODES for w in G.staging_widths(c)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"{8 * v}B")
def test_every_instantiation(eng, capfd, monkeypatch, code, staging):
    """One tile code with one staging width under all four operand layouts, both orientations of the planner's swap, a partial K step,
    two steps and a tail, whole steps, one / three / clamped K slices and beta 0 (over NaN) / -0.5 / 1: bit-exact, and each launch line
    shows the kernel the case was written for.  The 8-byte kernels run on odd extents and -- with 16-byte staging switched off -- on the
    even ones; the 16-byte kernels on the even ones (and on odd rows and columns where both operands are K-contiguous)."""
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    cs = G.cases_for(code, staging)
    seen, cache = set(), {}
    capfd.readouterr()
    for allow in (True, False):
        with tuning(eng, group_m=0 if allow else 0x10000):
            for c in cs:
                if c.allow_wide != allow:
                    continue
                if c.kind == "int":
                    line = run_int_case(eng, capfd, c, cache)
                    seen.add((line["akc"], line["bkc"]))
                    continue
                A, B, C0, ref, bound = G.float_case(c)
                got = eng.contract(c.alpha, A, c.la, B, c.lb, c.beta, C0, c.lc, force_split=c.force_split, force_tm=code[0], force_tn=code[1])
                line, _ = one_launch(capfd)
                assert (line["tm"], line["tn"], line["wide"], line["akc"], line["bkc"], line["split"]) == (code[0], code[1], c.wide, c.akc, c.bkc, c.split)
                err = np.abs(got.astype(ref.dtype) - ref)
                print(f"float case {code} staging {staging}: max error / bound = {float(np.max(err / bound)):.3f}")
                assert np.all(err <= bound), c
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}, seen


@pytest.mark.parametrize("tn", [7, 6])
def test_stream_k_against_plain_slices_exact(eng, capfd, monkeypatch, tn):
    """Stream-K on the smallest shape that takes it, against the same product in whole K slices (AFESP_GETT_SK=0): both exact.

    The launcher's condition (gett_launch; copied in np_gett.stream_k_decision, which picks the shape) for a forced (16, tn): with two
    column tiles, 24 row tiles and 121 K steps there are 48 tiles; the plain path cuts K into ceil(512 / 48) = 11 slices of 11 steps,
    528 items = 3 rounds of 256 workgroups filled to 0.6875.  Stream-K: nk' = 128 steps per tile in the sequence, j = ceil(48 / 32) = 2,
    U = 2 * 128 / 8 = 32 steps per workgroup (the least allowed), 128 / 32 + 1 = 5 pieces per tile (at most 8), and 48 / 64 = 0.75 >
    0.6875 + 0.02: taken.  One row tile fewer (46 tiles: 12 -> 11 slices, 506 items fill two rounds to 0.988) does not take it, and
    fewer than 121 steps make nk' < 128, U < 32.  Here every tile is cut into four whole pieces, so the fifth slab -- for tiles the sequence
    cuts early -- is written by nobody: the launcher zeroes it, and the reduce kernel sums all five."""
    Mk, Nk, K = G.smallest_stream_k_shape(tn)
    assert (Mk, K) == (5910, 1922) and Nk == 16 * tn + 26
    plain_split, sk, parts = G.stream_k_decision(Mk, Nk, K, tn)
    assert sk and parts == 5 and plain_split == 11
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    A, B = G.int_operands((K, Mk), (Nk, K), 4000 + tn)
    beta, alpha = -0.5, 2.0
    C0 = G.int_c0((Nk, Mk), beta, 4100 + tn)
    G.check_exactness_bound(K, alpha, beta, C0)
    ref = G.int_reference(G.int_product("km", A, "nk", B, "nm"), alpha, beta, C0)
    capfd.readouterr()
    # (whole slices first: their eleven slabs leave partial sums where stream-K's fifth slab lies, so a slab the launcher failed to zero
    # shows; the engine writes its result into the array it is handed when that is Fortran-ordered: a copy each)
    monkeypatch.setenv("AFESP_GETT_SK", "0")
    got_plain = eng.contract(alpha, A, "km", B, "nk", beta, C0.copy(order="F"), "nm", force_tm=16, force_tn=tn)
    line_plain, _ = one_launch(capfd)
    monkeypatch.delenv("AFESP_GETT_SK")
    got_sk = eng.contract(alpha, A, "km", B, "nk", beta, C0.copy(order="F"), "nm", force_tm=16, force_tn=tn)
    line_sk, _ = one_launch(capfd)
    for line in (line_sk, line_plain):
        assert (line["M"], line["N"], line["K"], line["tm"], line["tn"], line["wide"], line["akc"], line["bkc"]) == (Mk, Nk, K, 16, tn, 1, 1, 0), line
    assert (line_sk["sk"], line_sk["split"]) == (1, parts), line_sk
    assert (line_plain["sk"], line_plain["split"]) == (0, plain_split), line_plain
    for name, got in (("stream-K", got_sk), ("plain", got_plain)):
        bad = int(np.sum(got != ref))
        assert bad == 0, f"{name}: {bad} of {ref.size} elements differ"
    assert np.array_equal(got_sk, got_plain)


# (tile code, caller's form, kernel rows, kernel columns, beta, group_m): more tiles than the device holds workgroups of that kernel (a
# CU holds at most 32 waves: 8 four-wave or 4 eight-wave workgroups, 2048 / 1024 per device; LDS allows fewer), so workgroups take
# a second tile.  47 x 47 = 2209 and 33 x 33 = 1089 tiles are 1 mod 8 -- whatever multiple of eight the grid is, the last round of the
# XCD remap is partial -- and 47, 33 are no multiples of the group sizes 4 (eight or more column tiles) and 5.
WALKS = [
    ((1, 1), ("mk", "kn", "nm"), 1483, 1483, 1.0, 0),
    ((4, 4), ("km", "nk", "nm"), 4200, 4200, 0.0, 0),
    ((4, 4), ("km", "nk", "nm"), 4200, 4200, 0.0, 5),
    ((8, 8), ("mk", "nk", "mn"), 4200, 4200, -0.5, 0),
    ((16, 8), ("km", "kn", "nm"), 8400, 4200, 0.0, 0),
]
_walk_products = {}


@pytest.mark.parametrize("code,form,Mk,Nk,beta,group_m", WALKS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_persistent_walk(eng, capfd, monkeypatch, code, form, Mk, Nk, beta, group_m):
    """The in-kernel walk over many tiles: origin(), the XCD remap with a partial last round and a last group of fewer than gm row
    tiles.  The grid line shows that there were fewer workgroups than tiles."""
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    la, lb, lc = form
    K = 23
    swapped, akc, bkc = G.kernel_view(la, lb, lc)
    m, n = (Nk, Mk) if swapped else (Mk, Nk)
    d = {"m": m, "n": n, "k": K}
    key = (form, m, n)
    if key not in _walk_products:
        _walk_products.clear()
        A, B = G.int_operands(tuple(d[c] for c in la), tuple(d[c] for c in lb), 5000 + Mk + code[0])
        _walk_products[key] = (A, B, G.int_product(la, A, lb, B, lc))
    A, B, prod = _walk_products[key]
    C0 = G.int_c0(tuple(d[c] for c in lc), beta, 5100 + Mk)
    G.check_exactness_bound(K, 1.0, beta, C0)
    ref = G.int_reference(prod, 1.0, beta, C0)
    capfd.readouterr()
    with tuning(eng, group_m=group_m):
        got = eng.contract(1.0, A, la, B, lb, beta, C0, lc, force_split=1, force_tm=code[0], force_tn=code[1])
    line, grids = one_launch(capfd)
    assert (line["M"], line["N"], line["tm"], line["tn"], line["akc"], line["bkc"], line["wide"], line["split"]) == (Mk, Nk, code[0], code[1], akc, bkc, 0, 1)
    assert len(grids) == 1, grids
    wgs, tiles, gm = grids[0]
    print(f"walk {code}: {wgs} workgroups, {tiles} tiles, gm {gm}")
    assert tiles == line["mtiles"] * line["ntiles"] and wgs < tiles, "no workgroup takes a second tile"
    assert (tiles % wgs) % 8 != 0 and line["mtiles"] % gm != 0 and (group_m == 0 or gm == group_m)
    bad = int(np.sum(got != ref))
    assert bad == 0, f"{bad} of {ref.size} elements differ (first at {np.argwhere(got != ref)[0]})"


def _small_product(eng, capfd, code, m, n, k, beta, form=("mk", "kn", "nm"), seed=0, split=1):
    la, lb, lc = form
    d = {"m": m, "n": n, "k": k}
    A, B = G.int_operands(tuple(d[c] for c in la), tuple(d[c] for c in lb), 6000 + seed)
    C0 = G.int_c0(tuple(d[c] for c in lc), beta, 6100 + seed)
    ref = G.int_reference(G.int_product(la, A, lb, B, lc), 2.0, beta, C0)
    got = eng.contract(2.0, A, la, B, lb, beta, C0, lc, force_split=split, force_tm=code[0], force_tn=code[1])
    return got, ref


@pytest.mark.parametrize("tm,tn", G.UNSUPPORTED_CODES)
def test_unsupported_tile_code_is_an_error(eng, capfd, tm, tn):
    """A forced code that names no kernel used to launch nothing and report success -- with K slices the reduce kernel then summed an
    unwritten workspace into C.  Now an error that names the codes, through the call's arguments and through afesp_set_tuning; the
    engine goes on working."""
    from afesp_amd.capi import AfespError
    for split in (1, 3):
        with pytest.raises(AfespError, match=r"tile code .*\(16,7\)"):
            _small_product(eng, capfd, (tm, tn), 37, 41, 39, -0.5, split=split)
    with tuning(eng, tm=tm, tn=tn):
        with pytest.raises(AfespError, match=r"tile code .*\(16,7\)"):
            eng.gemm("N", "N", 37, 41, 39, np.ones((37, 39)), np.ones((39, 41)))
    got, ref = _small_product(eng, capfd, (2, 2), 37, 41, 39, -0.5, split=3)
    assert np.array_equal(got, ref)
    assert np.array_equal(eng.gemm("N", "N", 37, 41, 39, np.ones((37, 39)), np.ones((39, 41))), np.full((37, 41), 39.0))


@pytest.mark.parametrize("code", [(1, 1), (4, 4), (16, 8)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_degenerate_extents(eng, capfd, monkeypatch, code):
    """One row, one column, one summed element, and an empty summation.  K = 0: gett_kernel takes its `nk <= 0` branch before any
    Stager is initialised -- only origin() and store_tile() run, which index the C tables alone -- so no entry of the (empty) K tables
    is ever formed; C = beta C0 exactly, and zeros over NaN for beta = 0."""
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    capfd.readouterr()
    for i, (m, n, k) in enumerate([(1, 41, 9), (37, 1, 9), (37, 41, 1), (1, 1, 1), (1, 1, 39)]):
        for form in (("mk", "kn", "nm"), ("km", "nk", "mn")):
            for beta in (0.0, -0.5):
                got, ref = _small_product(eng, capfd, code, m, n, k, beta, form, seed=10 * i)
                line, _ = one_launch(capfd)
                assert (line["tm"], line["tn"], line["K"], {line["M"], line["N"]}) == (code[0], code[1], k, {m, n})
                assert np.array_equal(got, ref), (m, n, k, form, beta)
    for form in (("mk", "kn", "nm"), ("km", "nk", "mn")):
        for split in (1, 3):
            for beta in (0.0, -0.5):
                got, ref = _small_product(eng, capfd, code, 37, 41, 0, beta, form, seed=77, split=split)
                line, _ = one_launch(capfd)
                assert (line["tm"], line["tn"], line["K"], line["split"]) == (code[0], code[1], 0, 1)
                assert not np.isnan(got).any()
                assert np.array_equal(got, ref), (form, split, beta)
                if beta == 0.0:
                    assert np.array_equal(got, np.zeros_like(got))


def test_planner_forms_sweep(eng, capfd, monkeypatch):
    """150 label forms (np_gett.planner_forms) under AFESP_PLAN_VERIFY=1, heuristic tiles, exact: the launch line's extents and layout
    hints against the planner's rules written out in numpy, and its `wide` against a plain scan of the offset tables."""
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    monkeypatch.setenv("AFESP_PLAN_VERIFY", "1")
    capfd.readouterr()
    nwide = 0
    for i, (la, lb, lc, dims) in enumerate(G.planner_forms()):
        p = G.plan(la, lb, lc, dims)
        assert p["repack"] is None
        A, B = G.int_operands(tuple(dims[c] for c in la), tuple(dims[c] for c in lb), 7000 + i)
        beta = G.BETAS[i % 3]
        C0 = G.int_c0(tuple(dims[c] for c in lc), beta, 7500 + i)
        ref = G.int_reference(G.int_product(la, A, lb, B, lc), 1.0 + i % 2, beta, C0)
        got = eng.contract(1.0 + i % 2, A, la, B, lb, beta, C0, lc)
        line, _ = one_launch(capfd)
        want = dict(M=p["Md"], N=p["Nd"], K=p["Kd"], akc=int(p["akc"]), bkc=int(p["bkc"]), wide=int(G.scan_wide(la, lb, lc, dims)))
        assert {k: line[k] for k in want} == want, (la, lb, lc, dims)
        assert np.array_equal(got, ref), (la, lb, lc, dims)
        nwide += line["wide"]
    assert 20 <= nwide <= 130, nwide


@pytest.mark.parametrize("la,lb,lc,dims,role,swapped", G.REPACK_FORMS, ids=["kernel-A", "kernel-B", "swapped"])
def test_relayout_branch(eng, capfd, monkeypatch, la, lb, lc, dims, role, swapped):
    """The planner's re-layout branch: an operand gathered across its fastest index is copied once into (free labels, summation labels)
    order and the product planned again on the copy.  The trace line says `(repacked)`; a second call with other values must not
    find the first call's copy (these operands are not frozen)."""
    monkeypatch.setenv("AFESP_REPACK_MIN", "1")
    monkeypatch.setenv("AFESP_CONTRACT_TRACE", "1")
    p = G.plan(la, lb, lc, dims, repack_min=1)
    assert (p["repack"], p["swapped"]) == (role, swapped)
    capfd.readouterr()
    for call in range(2):
        A, B = G.int_operands(tuple(dims[c] for c in la), tuple(dims[c] for c in lb), 8000 + call)
        assert A.size > 4096 and B.size > 4096
        beta = (-0.5, 0.0)[call]
        C0 = G.int_c0(tuple(dims[c] for c in lc), beta, 8100 + call)
        ref = G.int_reference(G.int_product(la, A, lb, B, lc), 2.0, beta, C0)
        got = eng.contract(2.0, A, la, B, lb, beta, C0, lc)
        err = capfd.readouterr().err
        assert "(repacked)" in err and f"M {p['Md']:7d} N {p['Nd']:7d} K {p['Kd']:7d}" in err, err
        assert np.array_equal(got, ref), call
