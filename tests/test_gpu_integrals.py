"""The integral layer (csrc/integrals.hip, csrc/integrals_kernels.hip) where its forms switch, against np_integrals.py: E(MP2) in its one-launch
and five-launch forms, the levels by value and by reference, the size-demanded blocked transform, the open-shell transform and rotation at
odd extents, at the end of the pair kernel's 64 x 64 padding and at the switch to the gather form, with a spin that has no occupied or no
virtual orbital, the Fock builds on dense and on padded columns, and sequences of calls on the temporaries all of these share.

Bounds (np_integrals.py; derived for any summation order, not tuned): every MO integral |error| <= (4 n + 64) 2^-53 majorant, every Fock
element |error| <= (n^2 + 64) 2^-53 majorant, the majorant being the same expression on absolute values; energies 1e-10 max(1, |E|), the
rule these entry points have had since test_ao2mo_pair_symmetric_transform.  Up to n = 33 the reference is longdouble and the bound is
taken once; from n = 63 on the reference is float64 (held to 1 x the bound by test_integrals_cpu.py) and the bound is taken twice.
Random coefficient matrices are general, not orthogonal; levels have a gap of at least 2 between occupied and virtual.

Measured on an MI355X (every comparison prints its own error / bound; -s shows it): LARGEST_SEEN below -- transform 0.021 (n = 2; 0.017
the next), Fock 0.0089 (n = 2), scalars 2.7e-6 -- and the wall time of the two large cases: test_mp2_beyond_256_orbitals (n = 258, 18 GB
on the device) 0.2 to 0.5 s, test_ao2mo_full_size_with_a_signed_permutation (tests/test_gpu_fullsize.py, n = 220, 1.6e7 terms summed
on the host) 0.8 s per case."""
import numpy as np
import pytest

import np_integrals as I

pytestmark = pytest.mark.gpu

# largest |engine - reference| / bound per group over everything this module compares, as measured on an MI355X.  The bounds are worst cases
# over summation orders and the roundings are of independent sign, hence the distance; nothing is tuned to these figures.
LARGEST_SEEN = {"transform": 0.021, "Fock": 0.0089, "scalars": 2.7e-6}

LD = np.longdouble


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _fresh():
    from afesp_amd.capi import Engine
    return Engine(0)


# ------------------------------------------------------------------------------------------------------------------ inputs, comparisons
def _ref_dtype(n):
    """-> (dtype of the reference, how many times the bound)"""
    assert n <= 33 or n >= 63
    return (LD, 1.0) if n <= 33 else (np.float64, 2.0)


def _levels(rng, n, o):
    """rising, occupied in [-3, -2], virtual in [0, 1]: every denominator at most -4 ... a gap of 2"""
    return np.concatenate([np.sort(-3.0 + rng.random(o)), np.sort(rng.random(n - o))])


def _system(n, seed, scale):
    """packed AO integrals of the given scale, two general coefficient matrices of entries O(n^-1/2)"""
    rng = np.random.default_rng(seed)
    eri = scale * rng.standard_normal(I.neri(n))
    Ca, Cb = rng.standard_normal((n, n)) / np.sqrt(n), rng.standard_normal((n, n)) / np.sqrt(n)
    return rng, eri, Ca, Cb


class Reference:
    """the three MO blocks of (n, Ca, Cb, eri) with their majorants, computed once"""

    def __init__(self, n, Ca, Cb, eri):
        self.n = n
        self.dtype, self.times = _ref_dtype(n)
        V = I.unpack(n, eri)
        self.aa, self.ab, self.bb = I.mo_blocks(n, Ca, Cb, V, self.dtype)
        self.major = I.mo_majorant(n, Ca, Cb, V)
        for a in (self.aa, self.ab, self.bb) + tuple(self.major):
            a.setflags(write=False)

    def check_blocks(self, aa, ab, bb, what):
        n = self.n
        worst = 0.0
        for name, got, ref, m in (("aa", I.unpack(n, aa), self.aa, self.major[0]), ("ab", I.unpair_matrix(n, ab), self.ab, self.major[1]),
                                  ("bb", I.unpack(n, bb), self.bb, self.major[2])):
            worst = max(worst, _tensor(got, ref, m, I.xform_factor(n) * self.times, f"{what} ({name}|{name})", "transform"))
        return worst


def _tensor(got, ref, major, factor, what, group):
    """every element of got against ref within factor * major -> the largest error / bound"""
    bound = factor * major
    err = np.abs(got - ref).astype(np.float64)
    assert np.all(np.isfinite(got))
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    at = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{what}: error / bound ({group}) {ratio:.3g}   largest error {float(np.max(err)):.3g}, bound there {float(bound[at]):.3g}")
    assert np.all(err <= bound), (what, at, float(err[at]), float(bound[at]))
    return ratio


def _scalar(got, ref, major, what, in_range=True):
    ref = float(ref)
    bound = I.scalar_bound(ref)
    print(f"{what}: {got:.17g} reference {ref:.17g} error / bound (scalars) {abs(got - ref) / bound:.3g}   |ref| / majorant "
          f"{abs(ref) / major if major else float('nan'):.3g}")
    if in_range:
        assert 0.1 <= abs(ref) <= 1e4, (what, ref)
    assert abs(got - ref) <= bound, (what, got, ref)


# ------------------------------------------------------------------------------------------------------------------ (a) E(MP2), every form
MP2_SHAPES = [(1, 1), (2, 3), (5, 13), (9, 55)]
MP2_SCALE = {2: 4.0, 5: 2.0, 18: 1.0, 64: 0.25}


@pytest.mark.parametrize("o,v", MP2_SHAPES)
def test_mp2_in_both_forms(eng, o, v, monkeypatch):
    """The pair transform and E(MP2) by mp2_packed_kernel<true> (default) and by slice / denominators / mp2_energy_kernel
    (AFESP_MP2_PACKED=0): each against the reference, and against each other; at (5, 13) also through the window [1, n - 2), whose levels
    enter at an offset."""
    n = o + v
    rng, eri, C, _ = _system(n, 300 + n, MP2_SCALE[n])
    e = _levels(rng, n, o)
    ref = Reference(n, C, C, eri)
    e_ref, major = I.mp2(ref.aa, e, o, ref.dtype)
    got = {}
    for form in ("one launch", "five launches"):
        if form == "five launches":
            monkeypatch.setenv("AFESP_MP2_PACKED", "0")
        got[form], mo = eng.do_mp2_spatial(n, o, C, e, eri)
        _scalar(got[form], e_ref, major, f"E(MP2) o {o} v {v}, {form}")
        _tensor(I.unpack(n, mo), ref.aa, ref.major[0], I.xform_factor(n) * ref.times, f"MO integrals n {n}, {form}", "transform")
        if (o, v) == (5, 13):
            nfc, nfv = 1, 2
            act, e_win = eng.mo_window(n, o, nfc, nfv, e)
            sl = slice(nfc, n - nfv)
            w_ref, w_major = I.mp2(ref.aa[sl, sl, sl, sl], e[sl], o - nfc, ref.dtype)
            _scalar(e_win, w_ref, w_major, f"E(MP2) window [{nfc}, {n - nfv}), {form}")
            assert np.array_equal(I.unpack(n - nfc - nfv, act), I.unpack(n, mo)[sl, sl, sl, sl])
    assert abs(got["one launch"] - got["five launches"]) <= I.scalar_bound(e_ref)


# ------------------------------------------------------------------------------------------------------------------ (b) n > 256
def test_mp2_beyond_256_orbitals():
    """n = 258, o = 2: hashed AO integrals made on the device, a signed permutation for C, nothing large crosses the host.  The transform is
    the slab-blocked one because n^2 npair >= 2^31 demands it, and with o^2 v^2 = 2^18 <= 2^22 and n > 256 the energy is
    mp2_packed_kernel<false>'s, the variant that reads the levels from device memory.  Every MO integral is one AO integral with a sign
    (exact), so E(MP2) is held to the sum formed on the host from the hash alone.  About 18 GB of device memory."""
    n, o, scale, seed = 258, 2, 0.02, 777
    rng = np.random.default_rng(258)
    perm, sign = rng.permutation(n), rng.choice([-1.0, 1.0], n)
    c = np.zeros((n, n))
    c[np.arange(n), perm] = sign
    e = _levels(rng, n, o)
    with _fresh() as eng:
        eng.synthetic_ao(n, scale, seed)
        e_mp2, mo = eng.do_mp2_spatial(n, o, c, e, None, want_eri_mo=False)
    assert mo is None
    ref, major = I.hashed_mp2(n, o, perm, sign, e, scale, seed)
    _scalar(e_mp2, ref, major, "E(MP2) n 258, blocked transform, levels by reference")


# ------------------------------------------------------------------------------------------------------------------ (d) open-shell transform
UMP2_CASES = [(1, 1, 0), (2, 1, 1), (3, 3, 1), (17, 4, 0), (33, 9, 7), (63, 5, 4), (64, 6, 5), (65, 6, 5), (66, 3, 4)]
UMP2_SCALE = {1: 1.0, 2: 4.0, 3: 1.0, 17: 1.0, 33: 0.5, 63: 0.25, 64: 0.25, 65: 0.25, 66: 0.25}


def _ump2_terms(n, na, nb):
    va, vb = n - na, n - nb
    # (same-spin lists of one occupied orbital hold only i = j: every term is the square of an exact zero)
    return (na > 1) * na * na * va * va + (nb > 1) * nb * nb * vb * vb + na * nb * va * vb


@pytest.mark.parametrize("n,na,nb", UMP2_CASES)
def test_open_shell_transform(eng, n, na, nb):
    """afesp_ao2mo_ump2: the pair form (pair_xform_kernel<3> writes the whole alpha-beta column) up to n = 64, the gather form (k_pack_cols) from
    n = 65 on; odd n, the last n inside the pair kernel's 64 x 64 padding, a spin without occupied and one without virtual orbitals."""
    rng, eri, Ca, Cb = _system(n, 400 + n, UMP2_SCALE[n])
    ea, eb = _levels(rng, n, na), _levels(rng, n, nb)
    e2, aa, ab, bb = eng.do_ump2(n, na, nb, Ca, Cb, ea, eb, eri)
    ref = Reference(n, Ca, Cb, eri)
    ref.check_blocks(aa, ab, bb, f"do_ump2 n {n}")
    e_ref, major = I.ump2(ref.aa, ref.ab, ref.bb, ea, eb, na, nb, ref.dtype)
    zero = _ump2_terms(n, na, nb) == 0
    _scalar(e2, e_ref, major, f"E(UMP2) n {n} na {na} nb {nb}", in_range=not zero)
    if zero:
        assert e2 == 0.0                                   # no term, or only squares of x - x
    if na * (n - na) == 0 and nb * (n - nb) == 0:
        assert float(e_ref) == 0.0 and major == 0.0       # every list empty
    # the resident AO integrals as the source: the same launches, the same bits
    eng.set_eri(n, eri)
    again = eng.do_ump2(n, na, nb, Ca, Cb, ea, eb, None)
    assert again[0] == e2 and all(np.array_equal(x, y) for x, y in zip(again[1:], (aa, ab, bb)))


def test_refused_extents_are_a_status_and_the_engine_answers_the_next_call(eng):
    from afesp_amd.capi import AfespError
    n = 3
    rng, eri, Ca, Cb = _system(n, 403, 1.0)
    ea = _levels(rng, n, 1)
    for na, nb in ((0, 0), (4, 1), (1, -1)):
        with pytest.raises(AfespError, match="status 1"):
            eng.do_ump2(n, na, nb, Ca, Cb, ea, ea, eri)
    with pytest.raises(AfespError, match="status 1"):
        eng.do_ump2(0, 0, 0, Ca, Cb, ea, ea, eri)
    with pytest.raises(AfespError, match="status 1"):
        eng.mo_rotate_uhf(7, np.eye(7), np.eye(7))           # (no test leaves packed MO integrals of that size)
    e2, aa, ab, bb = eng.do_ump2(n, 3, 1, Ca, Cb, ea, ea, eri)
    Reference(n, Ca, Cb, eri).check_blocks(aa, ab, bb, "do_ump2 after refusals")


# ------------------------------------------------------------------------------------------------------------------ (e) the rotation
def _resident_packed(eng, n, nocc):
    """the packed MO array resident for n (a (0, 0) window leaves it where it is, bit for bit, and hands it out)"""
    return eng.mo_window(n, nocc, 0, 0, np.arange(n, dtype=np.float64))[0]


@pytest.mark.parametrize("n", [17, 64, 65])
def test_mo_rotate_uhf(eng, n):
    """afesp_mo_rotate_uhf: the same launches as the open-shell transform with the resident packed MO array as the source -- made resident
    by an identity transform, which is exact for any order of summation (every other product is an exact zero)"""
    rng, src, Ua, Ub = _system(n, 500 + n, 1.0)
    eng.do_mp2_spatial(n, 3, np.eye(n), np.arange(n, dtype=np.float64), src, want_eri_mo=False)
    packed = _resident_packed(eng, n, 3)
    assert np.array_equal(packed, src)
    aa, ab, bb = eng.mo_rotate_uhf(n, Ua, Ub, want_eri=True)
    Reference(n, Ua, Ub, src).check_blocks(aa, ab, bb, f"mo_rotate_uhf n {n}")
    assert np.array_equal(_resident_packed(eng, n, 3), src)           # the source: bit for bit


# ------------------------------------------------------------------------------------------------------------------ (f) the Fock builds
def _fock_inputs(n, seed):
    rng = np.random.default_rng(seed)
    eri = rng.standard_normal(I.neri(n))
    H = rng.standard_normal((n, n))
    H = H + H.T
    Da, Db = rng.standard_normal((n, n)), rng.standard_normal((n, n))     # Da non-symmetric, Db symmetric, Da != Db
    Db = Db + Db.T
    return eri, H, Da, Db


def _fock_builds(eng, n, H, Da, Db):
    """-> RHF(Da), RHF(Db), UHF(Da, Db) alpha and beta, UHF(Da, Da) alpha and beta"""
    ua, ub = eng.build_fock_uhf(n, Da, Db, H)
    sa, sb = eng.build_fock_uhf(n, Da, Da, H)
    return [eng.build_fock(n, Da, H), eng.build_fock(n, Db, H), ua, ub, sa, sb]


def _check_fock(n, got, eri, H, Da, Db, what):
    dtype, times = _ref_dtype(n)
    V = I.unpack(n, eri)
    f = I.fock_factor(n) * times
    _tensor(got[0], I.fock_rhf(n, H, V, Da, dtype), I.fock_majorant(n, H, V, Da), f, f"{what} build_fock n {n}, non-symmetric D", "Fock")
    _tensor(got[1], I.fock_rhf(n, H, V, Db, dtype), I.fock_majorant(n, H, V, Db), f, f"{what} build_fock n {n}, symmetric D", "Fock")
    ref, major = I.fock_uhf(n, H, V, Da, Db, dtype), I.fock_majorant(n, H, V, Da, Db)
    for s in range(2):
        _tensor(got[2 + s], ref[s], major[s], f, f"{what} build_fock_uhf n {n}, spin {s}", "Fock")
    assert np.array_equal(got[4], got[0]) and np.array_equal(got[5], got[0])       # Da = Db: the RHF matrix bit for bit


@pytest.mark.parametrize("n", [1, 2, 10, 11, 17])
def test_fock_builds_on_dense_columns(eng, n):
    """n = 1, 2; 55 and 66 pairs against the 64 partial sums of fock_j_kernel (fewer pairs than chunks, two pairs per chunk); an odd n"""
    eri, H, Da, Db = _fock_inputs(n, 600 + n)
    eng.set_eri(n, eri)
    _check_fock(n, _fock_builds(eng, n, H, Da, Db), eri, H, Da, Db, "dense")


@pytest.mark.parametrize("n", [16, 18, 30])
def test_fock_builds_on_forced_padded_columns(eng, n, monkeypatch):
    """AFESP_AO2MO_TG=1: half_unpacked hands the Fock kernels columns of ld = 16 ceil(n / 16) doubles (n = 16: ld = n; 18, 30: ld = 32).  The
    kernels' order of summation does not depend on ld: the same bits as with AFESP_AO2MO_PAD=0."""
    eri, H, Da, Db = _fock_inputs(n, 600 + n)
    monkeypatch.setenv("AFESP_AO2MO_TG", "1")
    eng.set_eri(n, eri)
    padded = _fock_builds(eng, n, H, Da, Db)
    _check_fock(n, padded, eri, H, Da, Db, "padded")
    monkeypatch.setenv("AFESP_AO2MO_PAD", "0")
    with _fresh() as other:
        other.set_eri(n, eri)
        dense = _fock_builds(other, n, H, Da, Db)
    for a, b in zip(padded, dense):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n", [96, 98])
def test_fock_builds_on_naturally_padded_columns(eng, n, monkeypatch):
    """Even n >= 96 run their RHF transform on the LDS-DMA GEMM, so the Fock builds get ld = 16 ceil(n / 16) unasked: 96 (= n) and 112.  Bit
    equality with AFESP_AO2MO_PAD=0, and 8 sampled elements of each matrix against the defining sum over the packed array (no n^4 array
    on the host)."""
    eri, H, Da, Db = _fock_inputs(n, 600 + n)
    eng.set_eri(n, eri)
    got = _fock_builds(eng, n, H, Da, Db)
    monkeypatch.setenv("AFESP_AO2MO_PAD", "0")
    with _fresh() as other:
        other.set_eri(n, eri)
        dense = _fock_builds(other, n, H, Da, Db)
    for a, b in zip(got, dense):
        assert np.array_equal(a, b)
    assert np.array_equal(got[4], got[0]) and np.array_equal(got[5], got[0])
    f = I.fock_factor(n) * _ref_dtype(n)[1]
    k, l = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rng = np.random.default_rng(n)
    worst = 0.0
    for i, j in [(0, 0), (n - 1, n - 1), (n - 1, 0), (3, n - 2)] + [tuple(rng.integers(0, n, 2)) for _ in range(4)]:
        cj, ck = eri[I._packed(i, j, k, l)], eri[I._packed(i, k, j, l)]
        aj, ak = np.abs(cj), np.abs(ck)
        for name, g, ref, major in (
                ("build_fock D non-symmetric", got[0], H[i, j] + np.sum(Da * (2.0 * cj - ck)), abs(H[i, j]) + np.sum(np.abs(Da) * (2.0 * aj + ak))),
                ("build_fock D symmetric", got[1], H[i, j] + np.sum(Db * (2.0 * cj - ck)), abs(H[i, j]) + np.sum(np.abs(Db) * (2.0 * aj + ak))),
                ("build_fock_uhf alpha", got[2], H[i, j] + np.sum((Da + Db) * cj - Da * ck),
                 abs(H[i, j]) + np.sum((np.abs(Da) + np.abs(Db)) * aj + np.abs(Da) * ak)),
                ("build_fock_uhf beta", got[3], H[i, j] + np.sum((Da + Db) * cj - Db * ck),
                 abs(H[i, j]) + np.sum((np.abs(Da) + np.abs(Db)) * aj + np.abs(Db) * ak))):
            ratio = abs(g[i, j] - ref) / (f * major)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, i, j, g[i, j], ref, ratio)
    print(f"natural padding n {n}: 8 sampled elements of four matrices, error / bound (Fock) {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------ (g) sequences
def _same(a, b):
    """bit for bit, whatever the call returns: a number, an array, or a tuple of them (None where nothing was asked for)"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("n", [18, 66])
def test_sequence_of_every_form_on_one_engine(n, monkeypatch):
    """S1.  Under AFESP_AO2MO_TG=1 the RHF transform and both Fock builds keep padded columns (ld = 32; 80) in the two temporaries the
    open-shell form (n = 18: pair form, n = 66: gather form) writes densely.  Eight calls on one engine; every result is, bit for bit, what
    the same call returns in a fresh engine that did only set_eri (and, for the rotation, the transform) before it."""
    monkeypatch.setenv("AFESP_AO2MO_TG", "1")
    rng, eri, Ca, Cb = _system(n, 700 + n, 1.0 if n == 18 else 0.25)
    _, H, Da, Db = _fock_inputs(n, 710 + n)
    na, nb, o = 4, 3, 5
    ea, eb, e = _levels(rng, n, na), _levels(rng, n, nb), _levels(rng, n, o)
    Ua, Ub = rng.standard_normal((n, n)) / np.sqrt(n), rng.standard_normal((n, n)) / np.sqrt(n)
    calls = {
        "fock_uhf": lambda g: g.build_fock_uhf(n, Da, Db, H),
        "ump2": lambda g: g.do_ump2(n, na, nb, Ca, Cb, ea, eb, None),
        "fock": lambda g: g.build_fock(n, Da, H),
        "mp2": lambda g: g.do_mp2_spatial(n, o, Ca, e, None),
        "rotate": lambda g: g.mo_rotate_uhf(n, Ua, Ub, want_eri=True),
    }
    fresh = {}
    for name, call in calls.items():
        with _fresh() as g:
            g.set_eri(n, eri)
            if name == "rotate":
                calls["mp2"](g)
            fresh[name] = call(g)
    with _fresh() as one:
        one.set_eri(n, eri)
        for step, name in enumerate(["fock_uhf", "ump2", "fock", "mp2", "rotate", "fock_uhf", "mp2", "ump2"], 1):
            assert _same(calls[name](one), fresh[name]), (step, name)
    if n == 18:
        V = I.unpack(n, eri)
        f = I.fock_factor(n)
        major = I.fock_majorant(n, H, V, Da, Db)
        for s, r in enumerate(I.fock_uhf(n, H, V, Da, Db, LD)):
            _tensor(fresh["fock_uhf"][s], r, major[s], f, f"S1 build_fock_uhf spin {s}", "Fock")
        _tensor(fresh["fock"], I.fock_rhf(n, H, V, Da, LD), I.fock_majorant(n, H, V, Da), f, "S1 build_fock", "Fock")
        ref = Reference(n, Ca, Cb, eri)
        ref.check_blocks(*fresh["ump2"][1:], "S1 do_ump2")
        _scalar(fresh["ump2"][0], *I.ump2(ref.aa, ref.ab, ref.bb, ea, eb, na, nb, LD), "S1 E(UMP2)")
        _tensor(I.unpack(n, fresh["mp2"][1]), ref.aa, ref.major[0], I.xform_factor(n), "S1 do_mp2_spatial", "transform")
        _scalar(fresh["mp2"][0], *I.mp2(ref.aa, e, o, LD), "S1 E(MP2)")
        # the rotation acts on the MO integrals the engine holds (fresh["mp2"]): reference and majorant from those
        Reference(n, Ua, Ub, fresh["mp2"][1]).check_blocks(*fresh["rotate"], "S1 mo_rotate_uhf")


def test_sequence_of_basis_sizes_on_one_engine(monkeypatch):
    """S2.  n = 30, 18, 30 under AFESP_AO2MO_TG=1: ld = 32 each time, so the same buffers serve and rows that were data are padding"""
    monkeypatch.setenv("AFESP_AO2MO_TG", "1")
    args = {}
    for n in (30, 18):
        rng, eri, C, _ = _system(n, 720 + n, 1.0)
        args[n] = (n, 4, C, _levels(rng, n, 4), eri)
    fresh = {}
    for n in args:
        with _fresh() as g:
            fresh[n] = g.do_mp2_spatial(*args[n])
    with _fresh() as one:
        for step, n in enumerate((30, 18, 30)):
            assert _same(one.do_mp2_spatial(*args[n]), fresh[n]), (step, n)


@pytest.mark.parametrize("n", [18, 30])
@pytest.mark.parametrize("first,then", [({"AFESP_AO2MO_TG": "1"}, {"AFESP_AO2MO_TG": "0"}), ({"AFESP_AO2MO_TG": "0"}, {"AFESP_AO2MO_TG": "1"}),
                                        ({"AFESP_AO2MO_TG": "1"}, {"AFESP_AO2MO_TG": "1", "AFESP_AO2MO_BLOCKED": "1"})])
def test_knobs_changed_between_a_fock_build_and_the_transform(n, first, then, monkeypatch):
    """S3.  build_fock under one set of knobs leaves (ij|KL) with its columns in one layout; the transform under another set must not take it
    for its own: bit for bit the result of a fresh engine under the transform's knobs."""
    rng, eri, C, _ = _system(n, 730 + n, 1.0)
    _, H, D, _ = _fock_inputs(n, 740 + n)
    e = _levels(rng, n, 4)
    for k, val in then.items():
        monkeypatch.setenv(k, val)
    with _fresh() as g:
        g.set_eri(n, eri)
        expect = g.do_mp2_spatial(n, 4, C, e, None)
    with _fresh() as one:
        one.set_eri(n, eri)
        for k in then:
            monkeypatch.delenv(k)
        for k, val in first.items():
            monkeypatch.setenv(k, val)
        f = one.build_fock(n, D, H)
        for k in first:
            monkeypatch.delenv(k)
        for k, val in then.items():
            monkeypatch.setenv(k, val)
        assert _same(one.do_mp2_spatial(n, 4, C, e, None), expect)
        assert _same(one.build_fock(n, D, H), f)        # (and the Fock build after it: the layout is the knobs', the sums are the same)


# ------------------------------------------------------------------------------------------------------------------ (h) 128-row tiles only
def test_ao2mo_with_128_row_tiles_only(monkeypatch):
    n, o = 24, 5
    rng, eri, C, _ = _system(n, 800 + n, 1.0)
    e = _levels(rng, n, o)
    monkeypatch.setenv("AFESP_AO2MO_TG", "1")
    with _fresh() as g:
        e_def, mo_def = g.do_mp2_spatial(n, o, C, e, eri)
        assert g.launch_counts()["tgemm_mixed"] > 0
    monkeypatch.setenv("AFESP_AO2MO_MIXED", "0")
    with _fresh() as g:
        e_128, mo_128 = g.do_mp2_spatial(n, o, C, e, eri)
        lc = g.launch_counts()
    assert lc["tgemm_mixed"] == 0 and lc["tgemm"] > 0, lc
    assert np.max(np.abs(mo_128 - mo_def)) <= 1e-11 * np.max(np.abs(mo_def))
    ref = Reference(n, C, C, eri)
    _tensor(I.unpack(n, mo_128), ref.aa, ref.major[0], I.xform_factor(n), "128-row tiles only, n 24", "transform")
    _scalar(e_128, *I.mp2(ref.aa, e, o, LD), "E(MP2), 128-row tiles only")
    assert abs(e_128 - e_def) <= I.scalar_bound(e_def)
