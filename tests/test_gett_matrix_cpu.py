"""The case generator of the gather-GEMM matrix tests (tests/np_gett.py) checked on its own: what it claims to cover, it covers."""
import numpy as np
import pytest

import np_gett as G


@pytest.fixture(scope="module")
def all_cases():
    return {code: G.cases(code) for code in G.TILE_CODES}


def test_fourteen_tile_codes_and_their_extents():
    assert len(G.TILE_CODES) == 14 == len(set(G.TILE_CODES))
    assert [G.tile_extent(c) for c in [(1, 1), (2, 4), (4, 4), (8, 8), (16, 8), (8, 16), (16, 7), (16, 6)]] == \
        [(32, 32), (64, 128), (128, 128), (128, 128), (256, 128), (128, 256), (256, 112), (256, 96)]
    assert sum(len(G.staging_widths(c)) for c in G.TILE_CODES) == 14 + 9
    assert len(G.FORMS) == 8 == len(set(G.FORMS))


def test_every_tile_code_staging_width_and_layout_is_produced(all_cases):
    for code, cs in all_cases.items():
        got = {(c.staging, c.akc, c.bkc) for c in cs if c.kind == "int"}
        want = {(w, a, b) for w in G.staging_widths(code) for a in (0, 1) for b in (0, 1)}
        assert got == want, code
        # both orientations of the planner's swap under every layout, and all three splits / betas / K kinds
        for w in G.staging_widths(code):
            sub = [c for c in cs if c.staging == w and c.kind == "int"]
            assert {(c.akc, c.bkc, G.kernel_view(c.la, c.lb, c.lc)[0]) for c in sub} == {(a, b, s) for a in (0, 1) for b in (0, 1) for s in (False, True)}
            assert {c.force_split for c in sub} == {1, 3, 7} and {c.beta for c in sub} == {0.0, -0.5, 1.0} and {c.alpha for c in sub} == {1.0, 2.0}
            assert {c.split for c in sub} == {1, 3}
            ksteps = {(-(-c.k // 16), c.k % 16 != 0) for c in sub}
            assert {(1, True), (3, True), (3, False)} <= ksteps, (code, w, ksteps)
            assert sum(c.kind == "float" and c.staging == w for c in cs) == 1


def test_parity_and_extent_conditions(all_cases):
    for code, cs in all_cases.items():
        BM, BN = G.tile_extent(code)
        for c in cs:
            swapped, akc, bkc = G.kernel_view(c.la, c.lb, c.lc)
            assert (c.akc, c.bkc) == (int(akc), int(bkc))
            assert (c.Mk, c.Nk) == ((c.n, c.m) if swapped else (c.m, c.n))
            # rows and columns end in the second tile, in the second 16-block of it, inside that block
            for ext, B in ((c.Mk, BM), (c.Nk, BN)):
                assert B < ext < 2 * B and (ext - B) // 16 == 1 and (ext - B) % 16 != 0
            # the 16-byte kernel needs: K even; rows (columns) even unless that operand is K-contiguous; staging not switched off
            legal = c.k % 2 == 0 and (c.akc or c.Mk % 2 == 0) and (c.bkc or c.Nk % 2 == 0)
            assert c.wide == int(legal and c.allow_wide)
            assert c.staging == (2 if c.wide and G.has_wide_instantiation(code) else 1)
            if not c.allow_wide:
                assert legal and c.Mk % 2 == 0 and c.Nk % 2 == 0 and c.k % 2 == 0   # the 8-byte kernel on extents the 16-byte one would take
            assert c.split == min(c.force_split, -(-c.k // 16))
        odd8 = [c for c in cs if c.staging == 1 and c.allow_wide and c.kind == "int"]
        assert any(c.Mk % 2 and c.Nk % 2 and c.k % 2 for c in odd8)


def test_operand_size_never_ends_on_a_page():
    """The kernels read clamped -- valid -- addresses past a ragged edge; the cases keep every 16-byte-staged operand clear of sizes
    where a one-element over-read (the bug the clamps exist to prevent) would leave the allocation's last 4 KiB page."""
    for code in G.TILE_CODES:
        for c in G.cases(code):
            if c.staging == 2:
                assert (c.m * c.k) % 512 and (c.n * c.k) % 512, c


def test_integer_exactness_bound(all_cases):
    for cs in all_cases.values():
        for c in cs[::37]:
            if c.kind != "int":
                continue
            C0 = G.int_c0(c.shapes()[2], c.beta, c.c_seed)
            G.check_exactness_bound(c.k, c.alpha, c.beta, C0)
            if c.beta == 0.0:
                assert np.isnan(C0).all()
            else:
                assert np.array_equal(C0 % 2, np.zeros_like(C0)) and np.max(np.abs(C0)) <= 8
    A, B = G.int_operands((5, 7), (7, 3), 1)
    assert A.dtype == np.int64 and A.min() >= -3 and A.max() <= 3
    with pytest.raises(AssertionError):
        G.check_exactness_bound(2 ** 50, 2.0, 0.0, None)
    # the reference: alpha * prod + beta * C0 in integers
    C0 = np.array([[2.0, -4.0, 6.0]] * 5)
    ref = G.int_reference(G.int_product("mk", A, "kn", B, "mn"), 2.0, -0.5, C0)
    assert np.array_equal(ref, 2.0 * (A @ B) - 0.5 * C0)


def test_float_case_bound_holds_for_a_double_precision_product():
    c = [x for x in G.cases((2, 2)) if x.kind == "float"][0]
    A, B, C0, ref, bound = G.float_case(c)
    got = c.alpha * np.einsum(f"{c.la},{c.lb}->{c.lc}", A, B) + c.beta * C0
    assert np.all(np.abs(got - ref) <= bound) and np.max(bound) < 1e-12
    assert not np.all(np.abs(got * (1 + 1e-11) - ref) <= bound)   # a relative error of 1e-11 is outside it


def test_stream_k_shape_is_the_smallest_that_qualifies():
    for tn in (7, 6):
        Mk, Nk, K = G.smallest_stream_k_shape(tn)
        assert (Mk, Nk, K) == (5910, 16 * tn + 26, 1922)
        assert G.stream_k_decision(Mk, Nk, K, tn) == (11, True, 5)
        assert not G.stream_k_decision(Mk - 256, Nk, K, tn)[1]     # one row tile fewer
        assert not G.stream_k_decision(Mk, Nk, K - 16, tn)[1]      # one K step fewer
        assert Mk % 2 == 0 and Nk % 2 == 0 and K % 2 == 0
    # the shape of tests/test_gpu_operators.py::test_stream_k_pieces_of_long_tiles takes it as well
    assert G.stream_k_decision(7670, 206, 4806, 7)[1] and G.stream_k_decision(7670, 190, 4806, 6)[1]


def test_table_scan_wide_predictor_on_six_small_forms():
    # dense matrices: K even and the extent of an operand that is contiguous along its rows / columns even
    assert G.scan_wide("km", "kn", "nm", dict(k=4, m=3, n=5)) is True        # both K-contiguous: odd rows and columns are fine
    assert G.scan_wide("mk", "kn", "nm", dict(k=4, m=3, n=5)) is False       # A contiguous along 3 rows
    assert G.scan_wide("mk", "nk", "nm", dict(k=4, m=6, n=2)) is True
    assert G.scan_wide("mk", "nk", "nm", dict(k=3, m=6, n=2)) is False       # K odd: pairs along m, but the launcher wants K even
    # a leading odd label continued by the next one enumerates 12 consecutive elements: pairs; split by the K label it does not
    assert G.scan_wide("abp", "pi", "iab", dict(a=3, b=4, p=6, i=4)) is True
    assert G.scan_wide("apb", "pi", "iab", dict(a=3, b=4, p=6, i=4)) is False
    assert G.offset_table(["a", "b"], {"a": 1, "b": 18}, dict(a=3, b=2)) == [0, 1, 2, 18, 19, 20]
    assert G.offset_table([], {}, {}) == [0]


def test_planner_rules_on_known_forms():
    p = G.plan("mjae", "iemb", "ijab", dict(m=5, j=5, a=11, e=11, i=5, b=11))
    assert p["swapped"] is False and (p["Md"], p["Nd"], p["Kd"]) == (55, 55, 55) and p["repack"] is None
    p = G.plan("mk", "kn", "mn", dict(m=4, k=5, n=6))
    assert p["swapped"] and p["M"] == ["n"] and p["N"] == ["m"] and (p["akc"], p["bkc"]) == (True, False)
    forms = G.planner_forms()
    assert len(forms) == 150 and forms == G.planner_forms()
    assert any(not p["K"] for p in (G.plan(*f) for f in forms)) and any(not p["N"] or not p["M"] for p in (G.plan(*f) for f in forms))
    assert max(len(f[0]) for f in forms) == 4 and max(len(f[2]) for f in forms) == 4
    assert any(f[3][f[0][0]] == 1 for f in forms) and any(f[3][f[0][-1]] == 1 for f in forms)
    wides = sum(G.scan_wide(*f) for f in forms)
    assert 20 <= wides <= 130
    for la, lb, lc, dims, role, swapped in G.REPACK_FORMS:
        p = G.plan(la, lb, lc, dims, repack_min=1)
        assert (p["repack"], p["swapped"]) == (role, swapped)
        assert G.plan(la, lb, lc, dims)["repack"] is None                     # (not at the default threshold: the test lowers it)
    assert [G.plan(f[0], f[1], f[2], f[3], repack_min=1)["repacked_caller_operand"] for f in G.REPACK_FORMS] == ["A", "B", "A"]
