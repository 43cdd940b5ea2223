"""Case generator and references for the gather-GEMM matrix tests (numpy only; csrc/gett.hip, csrc/contract.hip).

One kernel template is compiled about a hundred times: 14 tile codes x 4 operand layouts (a_kcontig, b_kcontig) x 8-byte or 16-byte
staging (the latter where tm, tn >= 2), plus the stream-K twins of the two narrow tiles.  The cases below are written so that each of
them is reached on purpose -- the generator states which one a case is for, and the GPU test checks that statement against the
launcher's diagnostic line.

Integer operands make the check exact: entries from {-3..3}, alpha in {1, 2}, beta in {0, -0.5, 1} and even-integer C0 keep every
product and every partial sum an integer below 2^53, so fp64 holds them exactly in ANY summation order -- K slices, stream-K pieces and
MFMA accumulation order included -- and the result must equal an int64 einsum bit for bit.
"""
import itertools
from dataclasses import dataclass, field

import numpy as np

BK = 16   # K step of the kernel

# (tm, tn) -> (BM, BN): rows and columns of the workgroup's tile (gett_launch)
TILE_CODES = [(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4), (4, 1), (4, 2), (4, 4), (8, 8), (16, 8), (8, 16), (16, 7), (16, 6)]
UNSUPPORTED_CODES = [(3, 0), (16, 4), (4, 8), (8, 4)]
_EXTENT = {1: 32, 2: 64, 4: 128, 8: 128, 16: 256, 7: 112, 6: 96}


def tile_extent(code):
    return _EXTENT[code[0]], _EXTENT[code[1]]


def has_wide_instantiation(code):
    """16-byte staging is compiled for the tiles with tm >= 2 and tn >= 2 ((16,7), (16,6) included)."""
    return code[0] >= 2 and code[1] >= 2


def staging_widths(code):
    return (1, 2) if has_wide_instantiation(code) else (1,)


# ---------------------------------------------------------------------------------------------------------------- two-index forms
FORMS = [(la, lb, lc) for la in ("mk", "km") for lb in ("kn", "nk") for lc in ("mn", "nm")]


def kernel_view(la, lb, lc):
    """What the planner makes of a two-index form whose extents are all > 1: (swapped, a_kcontig, b_kcontig).

    The kernel's column index runs along C's fastest label (Fortran order: the first).  If that label belongs to the caller's A, the
    operands change roles: the kernel's A is the caller's B and its rows are the caller's n.  An operand is K-contiguous when k is
    its first label."""
    swapped = lc[0] in la
    ka, kb = (lb, la) if swapped else (la, lb)
    return swapped, ka[0] == "k", kb[0] == "k"


def launcher_wide(akc, bkc, Mk, Nk, K, allow_wide=True):
    """The launcher's `wide` for a dense two-index product: every offset even and the contiguous direction of each operand in
    unit-stride pairs -- K even always (a K-contiguous operand pairs along K, the other one's K stride is its even extent), and the
    row / column extent even for an operand that is contiguous along it."""
    return bool(allow_wide and K % 2 == 0 and (akc or Mk % 2 == 0) and (bkc or Nk % 2 == 0))


def launcher_split(K, force_split):
    """K slices gett_launch ends up with for force_split > 0: clamped to the number of K steps, then evened out."""
    ksteps = -(-K // BK)
    split = min(force_split, ksteps) if ksteps > 0 else 1
    steps_per = max(1, -(-ksteps // split))
    return max(1, -(-ksteps // steps_per))


@dataclass
class Case:
    code: tuple            # forced (tm, tn)
    la: str
    lb: str
    lc: str
    m: int                 # the caller's extents
    n: int
    k: int
    Mk: int                # the kernel's rows and columns (after the planner's swap)
    Nk: int
    akc: int
    bkc: int
    allow_wide: bool       # False: run under set_tuning(group_m=0x10000)
    wide: int              # the launcher's flag expected in the diagnostic line
    staging: int           # elements per load of the instantiation this case is for (1: 8 bytes, 2: 16 bytes)
    force_split: int
    split: int             # K slices expected in the diagnostic line
    alpha: float
    beta: float
    kind: str = "int"      # "int": exact, "float": gamma bound
    ab_seed: int = 0
    c_seed: int = 0

    def shapes(self):
        d = {"m": self.m, "n": self.n, "k": self.k}
        return tuple(d[c] for c in self.la), tuple(d[c] for c in self.lb), tuple(d[c] for c in self.lc)


# M = BM + 16 q + r: the rows end inside the second tile, inside the second 16-row block of it (the second accumulator of a wave
# where TM >= 2, the second wave row where TM = 1) and r rows into that block; columns likewise with another remainder.
_R = {"odd": (5, 9), "even": (6, 10)}
_K = {"odd": (7, 39, 48), "even": (6, 38, 48)}     # one partial step / two steps and a tail / whole steps
SPLITS = (1, 3, 7)                                 # 7 is more than the three K steps there are: clamped by the launcher
BETAS = (0.0, -0.5, 1.0)


def kernel_extents(code, parity):
    BM, BN = tile_extent(code)
    r, rp = _R[parity]
    return BM + 16 + r, BN + 16 + rp


def cases(code):
    """Every case of one tile code: the eight forms x three K x three splits x three betas, on odd extents, on even extents and on the
    even extents with 16-byte staging switched off; plus one float case per staging width."""
    out = []
    ci = TILE_CODES.index(code)
    for parity, allow in (("odd", True), ("even", True), ("even", False)):
        Mk, Nk = kernel_extents(code, parity)
        for fi, (la, lb, lc) in enumerate(FORMS):
            swapped, akc, bkc = kernel_view(la, lb, lc)
            m, n = (Nk, Mk) if swapped else (Mk, Nk)
            for ki, K in enumerate(_K[parity]):
                wide = launcher_wide(akc, bkc, Mk, Nk, K, allow)
                staging = 2 if wide and has_wide_instantiation(code) else 1
                ab_seed = ((ci * 2 + (parity == "even")) * 8 + fi) * 3 + ki
                for si, fs in enumerate(SPLITS):
                    for bi, beta in enumerate(BETAS):
                        out.append(Case(code, la, lb, lc, m, n, K, Mk, Nk, int(akc), int(bkc), allow, int(wide), staging, fs,
                                        launcher_split(K, fs), float(1 + (si + bi + fi) % 2), beta, "int", ab_seed,
                                        ab_seed * 16 + si * 4 + bi))
    # float operands: one per staging width, the form cycling with the tile code, two K steps and a tail in three slices
    for parity in ("odd", "even") if has_wide_instantiation(code) else ("odd",):
        Mk, Nk = kernel_extents(code, parity)
        la, lb, lc = FORMS[ci % 8]
        swapped, akc, bkc = kernel_view(la, lb, lc)
        m, n = (Nk, Mk) if swapped else (Mk, Nk)
        K = _K[parity][1]
        wide = launcher_wide(akc, bkc, Mk, Nk, K)
        out.append(Case(code, la, lb, lc, m, n, K, Mk, Nk, int(akc), int(bkc), True, int(wide), 2 if wide and has_wide_instantiation(code) else 1,
                        3, launcher_split(K, 3), 2.0, -0.5, "float", 100000 + ci * 2 + (parity == "even"), 200000 + ci))
    return out


def cases_for(code, staging):
    return [c for c in cases(code) if c.staging == staging]


def check_exactness_bound(K, alpha, beta, C0):
    """Every partial sum of alpha * sum_k a b + beta * C0 is an integer of magnitude below 2^53: exact in fp64 in any order."""
    c0 = 0.0 if beta == 0.0 else float(np.max(np.abs(beta * C0), initial=0.0))
    assert K * 9 * abs(alpha) + c0 < 2 ** 53, (K, alpha, beta, c0)


def int_operands(shape_a, shape_b, seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 4, size=shape_a).astype(np.int64)
    B = rng.integers(-3, 4, size=shape_b).astype(np.int64)
    return A, B


def int_c0(shape_c, beta, seed):
    """Even integers (beta = -0.5 keeps them integers); NaN where beta = 0 says they must not be read."""
    if beta == 0.0:
        return np.full(shape_c, np.nan, order="F")
    rng = np.random.default_rng(seed)
    return np.asfortranarray(2.0 * rng.integers(-4, 5, size=shape_c))


def int_reference(prod, alpha, beta, C0):
    """alpha * prod + beta * C0 from the int64 product; exact, returned as fp64."""
    assert alpha == int(alpha)
    ref = int(alpha) * prod
    if beta != 0.0:
        bc = beta * C0
        assert np.array_equal(bc, np.rint(bc))
        ref = ref + bc.astype(np.int64)
    return ref.astype(np.float64)


def int_product(la, A, lb, B, lc):
    return np.einsum(f"{la},{lb}->{lc}", A, B)


def float_case(case):
    """Operands uniform in (-1, 1), the reference in extended precision and the element-wise bound
    |got - ref| <= (K + 3) 2^-53 (|alpha| |A| |B| + |beta C0|): the gamma bound of a K-term dot product in any order plus one rounding each
    for the scaling by alpha, the product beta C0 and their sum.  Without an extended type the reference itself carries that error:
    twice the bound."""
    rng = np.random.default_rng(case.ab_seed)
    sa, sb, sc = case.shapes()
    A = np.asfortranarray(rng.uniform(-1.0, 1.0, size=sa))
    B = np.asfortranarray(rng.uniform(-1.0, 1.0, size=sb))
    C0 = np.asfortranarray(rng.uniform(-1.0, 1.0, size=sc))
    ext = np.finfo(np.longdouble).eps < 1e-18
    T = np.longdouble if ext else np.float64
    expr = f"{case.la},{case.lb}->{case.lc}"
    ref = T(case.alpha) * np.einsum(expr, A.astype(T), B.astype(T)) + T(case.beta) * C0.astype(T)
    mag = abs(case.alpha) * np.einsum(expr, np.abs(A).astype(T), np.abs(B).astype(T)) + np.abs(T(case.beta) * C0.astype(T))
    bound = (case.k + 3) * T(2.0) ** -53 * mag * (1 if ext else 2)
    return A, B, C0, ref, bound


# ------------------------------------------------------------------------------------------------------------------- stream-K
def stream_k_decision(Mk, Nk, K, tn, ws_bytes=256 << 20, split_below=192, split_min_steps=4):
    """gett_launch for a forced (16, tn), tn in {6, 7}, force_split = 0, 16-byte staging: (K slices of the plain path, stream-K taken,
    pieces per tile).  A line-by-line copy of the launcher's condition, so that the test's shape is derived and not tried out."""
    BM, BN = 256, 16 * tn
    tiles = -(-Mk // BM) * -(-Nk // BN)
    ksteps = -(-K // BK)
    split = 1
    if tiles < split_below and ksteps >= 2 * split_min_steps:
        split = min(-(-512 // tiles), ksteps // split_min_steps)
    elif tiles < 1024 and ksteps >= 64 and Mk * Nk * 16 <= (Mk + Nk) * K:
        split = min(-(-1024 // tiles), ksteps // 8)
    split = max(1, min(split, ksteps))
    steps_per = max(1, -(-ksteps // split))
    ksplit = max(1, -(-ksteps // steps_per))
    if not (ksplit > 1 and ksteps >= 64):
        return ksplit, False, 0
    items = tiles * ksplit
    rounds = -(-items // 256)
    nkp = -(-ksteps // 8) * 8
    j8 = -(-tiles // 32)
    U = j8 * (nkp // 8)
    parts = -(-nkp // U) + 1
    fill = items / (rounds * 256)
    sk = (fill < 0.97 and tiles / (32.0 * j8) > fill + 0.02 and j8 < 8 and U >= 32 and parts <= 8 and parts * Mk * Nk * 8 <= ws_bytes
          and tiles * nkp < 2 ** 31)
    return ksplit, bool(sk), parts if sk else 0


def smallest_stream_k_shape(tn):
    """The shape of least work (tiles x K steps) that takes stream-K, among shapes with two column tiles whose last row tile and last
    column tile are partial (rows 256 (mt - 1) + 22, columns 16 tn + 26, both even) and whose last K step is partial (K = 16 ks - 14)."""
    best = None
    Nk = 16 * tn + 26
    for mt in range(2, 129):
        for ks in range(64, 400):
            Mk, K = 256 * (mt - 1) + 22, 16 * ks - 14
            if stream_k_decision(Mk, Nk, K, tn)[1]:
                if best is None or 2 * mt * ks < best[0]:
                    best = (2 * mt * ks, Mk, Nk, K)
                break
    return best[1:]


# ---------------------------------------------------------------------------------------------------------------- planner forms
def _strides(labels, dims):
    s, out = 1, {}
    for c in labels:
        out[c] = s
        s *= dims[c]
    return out, s


def _min_stride_label(labels, dims):
    for c in labels:          # Fortran order: strides ascend along the labels
        if dims[c] > 1:
            return c
    return labels[0] if labels else ""


def plan(la0, lb0, lc, dims, repack_min=256):
    """The planner's view of A(la0) B(lb0) -> C(lc) for dense Fortran-ordered operands (csrc/contract.hip): operand roles, the label
    order of the row, column and summation groups, the layout hints and which operand (kernel role 'A' / 'B' or None) it would
    re-lay out.  Written from the planner's rules; the GPU test checks M, N, K, akc and bkc against the launch line."""
    cfast = _min_stride_label(lc, dims)
    swapped = cfast in la0
    la, lb = (lb0, la0) if swapped else (la0, lb0)
    sa, size_a = _strides(la, dims)
    sb, size_b = _strides(lb, dims)
    sc, _ = _strides(lc, dims)
    M = [c for c in la if c in lc]
    K = [c for c in la if c not in lc]
    N = [c for c in lb if c not in la]
    afast, bfast = _min_stride_label(la, dims), _min_stride_label(lb, dims)
    N.sort(key=lambda c: sc[c])
    M.sort(key=(lambda c: sa[c]) if afast in M else (lambda c: sc[c]))
    if afast in K and bfast in K:
        K.sort(key=(lambda c: sb[c]) if size_b > 4 * size_a else (lambda c: sa[c]))
    elif afast in K:
        K.sort(key=lambda c: sa[c])
    elif bfast in K:
        K.sort(key=lambda c: sb[c])
    else:
        K.sort(key=lambda c: sa[c])

    def lead(g):
        for c in g:
            if dims[c] > 1:
                return c
        return ""
    a_ok = lead(K) == afast or lead(M) == afast or size_a <= 4096
    b_ok = lead(K) == bfast or lead(N) == bfast or size_b <= 4096
    Md = int(np.prod([dims[c] for c in M], dtype=np.int64))
    Nd = int(np.prod([dims[c] for c in N], dtype=np.int64))
    Kd = int(np.prod([dims[c] for c in K], dtype=np.int64))
    longk = Kd >= 65536
    repack = None
    if not b_ok and (Md >= repack_min or size_a >= 8 * size_b or (longk and size_b <= 2 * size_a)):
        repack = "B"
    elif not a_ok and (Nd >= repack_min or size_b >= 8 * size_a or (longk and size_a <= 2 * size_b)):
        repack = "A"
    akc = bool(K) and K[0] == afast and sa[K[0]] == 1
    bkc = bool(K) and K[0] == bfast and sb[K[0]] == 1
    return dict(swapped=swapped, M=M, N=N, K=K, Md=Md, Nd=Nd, Kd=Kd, akc=akc, bkc=bkc, sa=sa, sb=sb, sc=sc, repack=repack,
                repacked_caller_operand=None if repack is None else ("A" if (repack == "A") != swapped else "B"))


def offset_table(group, strides, dims):
    """Offsets of a label group enumerated first label fastest (an empty group is the single offset 0)."""
    t = [0]
    for c in group:
        t = [x + i * strides[c] for i in range(dims[c]) for x in t]
    return t


def _pairs(t):
    return len(t) % 2 == 0 and all(t[x] % 2 == 0 and t[x + 1] == t[x] + 1 for x in range(0, len(t), 2))


def _evens(t):
    return all(x % 2 == 0 for x in t)


def scan_wide(la0, lb0, lc, dims):
    """16-byte staging is legal when, for each operand, the table of its contiguous direction advances in aligned unit-stride pairs
    and every entry of its other table is even -- found here by scanning the enumerated tables, entry by entry; then the launcher's
    own parity conditions on the extents."""
    p = plan(la0, lb0, lc, dims)
    am, ak = offset_table(p["M"], p["sa"], dims), offset_table(p["K"], p["sa"], dims)
    bn, bk = offset_table(p["N"], p["sb"], dims), offset_table(p["K"], p["sb"], dims)
    a = (_pairs(ak) and _evens(am)) if p["akc"] else (_pairs(am) and _evens(ak))
    b = (_pairs(bk) and _evens(bn)) if p["bkc"] else (_pairs(bn) and _evens(bk))
    M, N, K = len(am), len(bn), len(ak)
    return bool(a and b and (p["akc"] or M % 2 == 0) and (p["bkc"] or N % 2 == 0) and K % 2 == 0)


# group structures (labels in M, N, K): ranks up to 4 + 4 -> 4, a GEMV-shaped and an outer-product-shaped member included
_EXTENTS = (1, 2, 3, 4, 6, 7)
_RANDOM_STRUCTURES = [(2, 2, 2), (1, 2, 2), (2, 1, 2), (3, 1, 1), (1, 3, 1), (2, 2, 1), (1, 1, 3), (2, 0, 2), (0, 2, 1), (2, 2, 0), (1, 1, 0),
                      (3, 0, 1)]


def _labels(nm, nn, nk):
    return "abc"[:nm], "ijl"[:nn], "pqr"[:nk]


def planner_forms(seed=20240607):
    """About 150 products (la, lb, lc, dims), deterministic: every label order of the structures (1,1,1) and (2,1,1), two hand-written
    pairs on the merging rule, and seeded random label orders of the larger structures; extents from {1, 2, 3, 4, 6, 7}, extent-1
    labels in leading and other positions."""
    rng = np.random.default_rng(seed)
    out = []

    def draw(labels):
        return {c: int(rng.choice(_EXTENTS)) for c in labels}
    for nm, nn, nk in ((1, 1, 1), (2, 1, 1)):
        m, n, k = _labels(nm, nn, nk)
        for pa in itertools.permutations(m + k):
            for pb in itertools.permutations(k + n):
                for pc in itertools.permutations(m + n):
                    out.append(("".join(pa), "".join(pb), "".join(pc), draw(m + n + k)))
    # a leading free label of odd extent continued by the next label enumerates in pairs (3 x 4 = 12 consecutive elements); ...
    out.append(("abp", "pi", "iab", dict(a=3, b=4, p=6, i=4)))
    # ... the same two labels with the summation label between them in memory do not (0 1 2 | 18 19 20 | ...)
    out.append(("apb", "pi", "iab", dict(a=3, b=4, p=6, i=4)))
    # an extent-1 label in front of / between the pair changes nothing: it enumerates nothing
    out.append(("cabp", "pi", "icab", dict(c=1, a=3, b=4, p=6, i=4)))
    out.append(("acbp", "pi", "iacb", dict(a=3, c=1, b=4, p=6, i=4)))
    while len(out) < 150:
        nm, nn, nk = _RANDOM_STRUCTURES[len(out) % len(_RANDOM_STRUCTURES)]
        m, n, k = _labels(nm, nn, nk)
        la = "".join(rng.permutation(list(m + k)))
        lb = "".join(rng.permutation(list(k + n)))
        lc = "".join(rng.permutation(list(m + n)))
        dims = draw(m + n + k)
        if len(out) % 5 == 0:                      # an extent-1 label for certain, wherever the permutation put it
            dims[str(rng.choice(list(m + n + k)))] = 1
        out.append((la, lb, lc, dims))
    return out


# ------------------------------------------------------------------------------------------------------------------ re-layout
# Operands of more than 4096 elements whose unit-stride label leads neither their free nor the summation enumeration: the caller's
# A and B both start with a summation label, in opposite orders, so the summation group follows one of them only.
REPACK_FORMS = [
    # B is more than four times A: the summation group follows B, A(p,q,m) is gathered across its columns -> kernel A re-laid-out
    ("pqm", "qpn", "nm", dict(p=16, q=18, m=17, n=69), "A", False),
    # operands of like size: the summation group follows A -> kernel B re-laid-out
    ("pqm", "qpn", "nm", dict(p=16, q=18, m=37, n=35), "B", False),
    # C's fastest label is the caller's A's: roles swapped, the kernel's B -- the caller's A -- is re-laid-out
    ("pqm", "qpn", "mn", dict(p=16, q=18, m=37, n=35), "B", True),
]
