"""The spin-orbital Lambda equations and the density (csrc/lambda_so.hip) term by term at extents where the planner leaves its smallest
branch: every H-bar element through afesp_ccsd_so_get_tensor, one Jacobi step, G_vv / G_oo, the pseudo energy, the density, a second
initialisation on the same state and a T iteration on the scratch Lambda has used -- against the explicit restatement of np_lambda
(hbar, lambda_rhs_explicit, density_explicit) at O(1) random amplitudes.  tests/test_lambda_cpu.py shows that restatement equal to the
complex-step definition at small extents and within 1e-13 of its own np.longdouble evaluation at two of the shapes used here.

Shapes (o, v spin orbitals), each the smallest that crosses the thresholds named:
  rhf_mid   RHF-fed      n = 14, 5 + 5   o = 10, v = 18   even extents (16-byte staging), o v = 180 and v^2 = 324 rows (64- and 128-row
                                                           tiles), operands above 4096 elements, o v^2 = 3240 rows for the tall kernel
  fock_odd  Fock-rotated n = 11, 5 + 4   o =  9, v = 13   odd extents (8-byte staging only), every f_ov / f_oo / f_vv term, so_sum2_kernel's
                                                           f . l1 sum over 117 elements
  rhf_cap   RHF-fed      n = 29, 6 + 6   o = 12, v = 46   o^2 v^2 = 304704 > 262144: the 1024-block cap and a second grid-stride pass of
                                                           lam_l2_assemble_kernel / lam_energy_kernel; v^2 = 2116 >= 2048: the tile-scoring
                                                           block of gett_launch; offset tables of v^3 = 97336 >= 32768 entries (device-built)

Tolerance: 1e-11 x max(1, max |ref|) per tensor, 1e-11 x max(1, |value|) per scalar; every comparison prints its error
and its bound.  BRANCHES and ERRORS at the end of this docstring are as printed on an MI355X.

BRANCHES.  One row per product of so_lambda_init / so_lambda_iterate / so_density, per shape: kernel extents M x N x K, tile code tm,tn
(1, 2, 4: 32, 64, 128 rows or columns), K slices s, 16-byte staging w, and T where the product runs on the tall kernel once AFESP_TALL_MIN is
o^2 v (test_t1_products_on_the_tall_kernel; the default threshold 2^17 sends none of them there).  No product of any shape is re-laid-out.
`pair-form ladder` is so_ladder_bare's own launch on its packed pair buffers (v (v - 1) / 2 rows, o (o - 1) / 2 columns padded to even): it
stages 16 bytes at fock_odd too, where every product of the planner stages 8.  The scoring block of gett_launch hands out 4,2 at M = 2116
(rhf_cap: mnab,mnie>ieab; miaf,mbef>ieab; ijme,emab>ijab; ijmn,mnab>ijab); none of Lambda's products reaches a 256-row tile (tm 16).
  call     product           | rhf_mid (10, 18)             | fock_odd (9, 13)             | rhf_cap (12, 46)
  init     mnef,nf>me        | 1x180x180 1,4 s3 w1          | 1x117x117 1,4 s2 w0          | 1x552x552 1,4 s7 w1
  init     mnie,ne>mi        | 1x100x180 1,4 s3 w1          | 1x81x117 1,4 s2 w0           | 1x144x552 1,4 s7 w1
  init     inef,mnef>mi      | 10x10x3240 1,1 s41 w1        | 9x9x1521 1,1 s24 w0          | 12x12x25392 1,1 s318 w1
  init     mafe,mf>ae        | 1x324x180 1,4 s3 w1          | 1x169x117 1,4 s2 w0          | 1x2116x552 1,4 s7 w1
  init     mnaf,mnef>ae      | 18x18x1800 1,1 s23 w1        | 13x13x1053 1,1 s14 w0        | 46x46x6624 2,2 s83 w1
  init     mnie,je>mnij      | 10x1000x18 1,4 s1 w1         | 9x729x13 1,4 s1 w0           | 12x1728x46 1,4 s1 w1
  init     mnef,ijef>mnij    | 100x100x324 4,4 s5 w1        | 81x81x169 4,4 s2 w0          | 144x144x2116 4,4 s27 w1
  init     na,nmef>amef      | 3240x18x10 4,1 s1 w1         | 1521x13x9 4,1 s1 w0          | 25392x46x12 4,2 s1 w1
  init     mnef,if>mnie      | 10x1800x18 1,4 s1 w1 T       | 9x1053x13 1,4 s1 w0          | 12x6624x46 1,4 s1 w1 T
  init     mbef,jf>mbej      | 10x3240x18 1,4 s1 w1 T       | 9x1521x13 1,4 s1 w0          | 12x25392x46 1,4 s1 w1 T
  init     nb,nmej>mbej      | 18x1800x10 1,4 s1 w1         | 13x1053x9 1,4 s1 w0          | 46x6624x12 2,4 s1 w1
  init     mnef,nfjb>mbej    | 180x180x180 4,4 s3 w1        | 117x117x117 4,4 s2 w0        | 552x552x552 4,4 s7 w1
  init     mnef,nibf>mbei    | 180x180x180 4,4 s3 w1        | 117x117x117 4,4 s2 w0        | 552x552x552 4,4 s7 w1
  init     if,amef>miae      | 10x3240x18 1,4 s1 w0         | 9x1521x13 1,4 s1 w0          | 12x25392x46 1,4 s1 w0
  init     me,miab>ieab      | 18x3240x10 1,4 s1 w1         | 13x1521x9 1,4 s1 w0          | 46x25392x12 2,4 s1 w1
  init     if,abef>ieab      | 5832x10x18 4,1 s1 w1 T       | 2197x9x13 4,1 s1 w0          | 97336x12x46 4,1 s1 w1 T
  init     mnab,mnie>ieab    | 324x180x100 4,4 s1 w1        | 169x117x81 4,4 s1 w0         | 2116x552x144 4,2 s2 w1
  init     miaf,mbef>ieab    | 324x180x180 4,4 s3 w1        | 169x117x117 4,4 s2 w0        | 2116x552x552 4,2 s4 w1
  init     ma,mbei>ieab      | 18x3240x10 1,4 s1 w1         | 13x1521x9 1,4 s1 w0          | 46x25392x12 2,4 s1 w1
  init     mb,miae>ieab      | 18x3240x10 1,4 s1 w1         | 13x1521x9 1,4 s1 w0          | 46x25392x12 2,4 s1 w1
  init     me,ijbe>mbij      | 1800x10x18 4,1 s1 w1 T       | 1053x9x13 4,1 s1 w0          | 6624x12x46 4,1 s1 w1 T
  init     nb,mnij>mbij      | 18x1000x10 1,4 s1 w1         | 13x729x9 1,4 s1 w0           | 46x1728x12 2,4 s1 w1
  init     ijef,mbef>mbij    | 100x180x324 4,4 s5 w1        | 81x117x169 4,4 s2 w0         | 144x552x2116 4,4 s27 w1
  init     jnbe,mnie>mbij    | 180x100x180 4,4 s3 w1        | 117x81x117 4,4 s2 w0         | 552x144x552 4,4 s7 w1
  init     ie,mbej>mbij      | 10x1800x18 1,4 s1 w1 T       | 9x1053x13 1,4 s1 w0          | 12x6624x46 1,4 s1 w1 T
  iterate  mnef,mnaf>ae      | 18x18x1800 1,1 s23 w1        | 13x13x1053 1,1 s14 w0        | 46x46x6624 2,2 s83 w1
  iterate  mnef,inef>mi      | 10x10x3240 1,1 s41 w1        | 9x9x1521 1,1 s24 w0          | 12x12x25392 1,1 s318 w1
  iterate  ie,ea>ia          | 18x10x18 1,1 s1 w1           | 13x9x13 1,1 s1 w0            | 46x12x46 2,1 s1 w1
  iterate  im,ma>ia          | 18x10x10 1,1 s1 w1           | 13x9x9 1,1 s1 w0             | 46x12x12 2,1 s1 w1
  iterate  me,ieam>ia        | 1x180x180 1,4 s3 w1          | 1x117x117 1,4 s2 w0          | 1x552x552 1,4 s7 w1
  iterate  imef,maef>ia      | 18x10x3240 1,1 s41 w1        | 13x9x1521 1,1 s24 w0         | 46x12x25392 2,1 s318 w1
  iterate  mnae,iemn>ia      | 18x10x1800 1,1 s23 w1        | 13x9x1053 1,1 s14 w0         | 46x12x6624 2,1 s83 w1
  iterate  ef,eifa>ia        | 1x180x324 1,4 s5 w1          | 1x117x169 1,4 s2 w0          | 1x552x2116 1,4 s27 w1
  iterate  mn,mina>ia        | 1x180x100 1,4 s1 w1          | 1x117x81 1,4 s1 w0           | 1x552x144 1,4 s2 w1
  iterate  pair-form ladder  | 153x46x154 4,2 s2 w1         | 78x36x78 4,2 s1 w1           | 1035x66x1036 4,4 s13 w1
  iterate  ijef,mf>ijme      | 10x1800x18 1,4 s1 w1 T       | 9x1053x13 1,4 s1 w0          | 12x6624x46 1,4 s1 w1 T
  iterate  ijme,emab>ijab    | 324x100x180 4,4 s3 w1        | 169x81x117 4,4 s2 w0         | 2116x144x552 4,2 s7 w1
  iterate  ijef,mnef>ijmn    | 100x100x324 4,4 s5 w1        | 81x81x169 4,4 s2 w0          | 144x144x2116 4,4 s27 w1
  iterate  ijmn,mnab>ijab    | 324x100x100 4,4 s1 w1        | 169x81x81 4,4 s1 w0          | 2116x144x144 4,2 s2 w1
  iterate  ijmn,mnab>ijab    | 324x100x100 4,4 s1 w1        | 169x81x81 4,4 s1 w0          | 2116x144x144 4,2 s2 w1
  iterate  imae,jebm>ijab    | 180x180x180 4,4 s3 w1        | 117x117x117 4,4 s2 w0        | 552x552x552 4,4 s7 w1
  iterate  jm,imab>ijab      | 10x3240x10 1,4 s1 w1         | 9x1521x9 1,4 s1 w0           | 12x25392x12 1,4 s1 w1
  iterate  ie,ejab>ijab      | 3240x10x18 4,1 s1 w1 T       | 1521x9x13 4,1 s1 w0          | 25392x12x46 4,1 s1 w1 T
  iterate  imab,mj>ijab      | 10x3240x10 1,4 s1 w1         | 9x1521x9 1,4 s1 w0           | 12x25392x12 1,4 s1 w1
  iterate  ijae,eb>ijab      | 18x1800x18 1,4 s1 w1 T       | 13x1053x13 1,4 s1 w0         | 46x6624x46 2,4 s1 w1
  iterate  ijmb,ma>ijab      | 18x1800x10 1,4 s1 w1         | 13x1053x9 1,4 s1 w0          | 46x6624x12 2,4 s1 w1
  iterate  ijae,be>ijab      | 18x1800x18 1,4 s1 w1 T       | 13x1053x13 1,4 s1 w0         | 46x6624x46 2,4 s1 w1
  density  mnef,mnaf>ae      | 18x18x1800 1,1 s23 w1        | 13x13x1053 1,1 s14 w0        | 46x46x6624 2,2 s83 w1
  density  mnef,inef>mi      | 10x10x3240 1,1 s41 w1        | 9x9x1521 1,1 s24 w0          | 12x12x25392 1,1 s318 w1
  density  ma,ia>mi          | 10x10x18 1,1 s1 w1           | 9x9x13 1,1 s1 w0             | 12x12x46 1,1 s1 w1
  density  ia,ie>ae          | 18x18x10 1,1 s1 w1           | 13x13x9 1,1 s1 w0            | 46x46x12 2,2 s1 w1
  density  ia,imae>me        | 1x180x180 1,4 s3 w1          | 1x117x117 1,4 s2 w0          | 1x552x552 1,4 s7 w1
  density  mb,be>me          | 18x10x18 1,1 s1 w1           | 13x9x13 1,1 s1 w0            | 46x12x46 2,1 s1 w1
  density  mj,je>me          | 18x10x10 1,1 s1 w1           | 13x9x9 1,1 s1 w0             | 46x12x12 2,1 s1 w1
  init     me,ie>mi          | -                            | 9x9x13 1,1 s1 w0             | -
  init     ma,me>ae          | -                            | 13x13x9 1,1 s1 w0            | -

ERRORS.  Largest error over its bound, per shape: rhf_mid 2.2e-4 (G_vv: 5.3e-15 against 2.4e-11), fock_odd 2.0e-4 (G_vv: 2.6e-15 against
1.3e-11), rhf_cap 1.2e-4 (G1: 1.4e-13 against 1.1e-9); the longest sum, K = o v^2 = 25392 of H_oo / G_oo at rhf_cap, is 8.0e-15 off.  No
tensor needs the long-sum rule.  The tall kernel and the gather kernel agree to the bit on every tensor compared (one K step order).
RE-LAYOUT.  Zero launches of the traced pass at rhf_cap carry `(repacked)` (measured), although operands exceed 4096 elements and free
extents exceed AFESP_REPACK_MIN = 256 there: in these label forms the unit-stride label of each operand leads its free or its summed group
(a_ok / b_ok of contract.hip).  That rule looks at labels and strides only, so the same is supposed -- not measured -- of larger systems;
tests/test_gpu_gett_matrix.py::test_relayout_branch covers the branch with forms of its own."""
import re

import numpy as np
import pytest

import np_lambda
from test_gpu_gett_matrix import _FIELDS, LAUNCH
from test_gpu_lambda import _build_case, _close, _feed

pytestmark = pytest.mark.gpu

MID = {   # name: (source, n, nalpha, nbeta, seed)
    "rhf_mid": ("rhf", 14, 5, 5, 201),
    "fock_odd": ("fock", 11, 5, 4, 202),
    "rhf_cap": ("rhf", 29, 6, 6, 203),
}
EXTENTS = {"rhf_mid": (10, 18), "fock_odd": (9, 13), "rhf_cap": (12, 46)}
# getter name (include/afesp.h) -> key of np_lambda.hbar, in the storage both document
HBAR = {"H_ov": "Hov", "H_oo": "Hoo", "H_vv": "Hvv", "H_oooo": "Hoooo", "H_vovv": "Hvovv", "H_ooov": "Hooov", "H_ovvo": "Hovvo",
        "H_vvvo": "Hvvvo", "H_ovoo": "Hovoo", "lam_tau": "tau"}
TRACE = re.compile(r"contract (\S+)\s*,(\S+)\s*>(\S+)\s+M\s+(\d+) N\s+(\d+) K\s+(\d+) akc (\d) bkc (\d) wide (\d)[^\n]*?(\(repacked\)|\(tall\))?\n")

_REF = {}


def _ref(name):
    """the numpy side of a shape, made once and left unchanged: the system, two sets of amplitudes, the explicit form at both"""
    if name in _REF:
        return _REF[name]
    c = _build_case(name, *MID[name])
    cc, o, v = c["cc"], c["o"], c["v"]
    assert (o, v) == EXTENTS[name]
    rng = np.random.default_rng(7)
    t1, t2 = np_lambda.antisym_random(rng, o, v)
    l1, l2 = np_lambda.antisym_random(rng, o, v)
    s1, s2 = np_lambda.antisym_random(np.random.default_rng(8), o, v)       # the second initialisation's amplitudes
    I = np_lambda.hbar(cc, t1, t2)
    x1, x2 = np_lambda.lambda_rhs_explicit(cc, t1, t2, l1, l2, I)
    r = dict(c=c, t=(t1, t2), l=(l1, l2), s=(s1, s2), I=I, x=(x1, x2), I2=np_lambda.hbar(cc, s1, s2),
             Gvv=-0.5 * np.einsum("mnef,mnaf->ae", t2, l2, optimize=True), Goo=0.5 * np.einsum("mnef,inef->mi", t2, l2, optimize=True),
             density=np_lambda.density_explicit(cc, t1, t2, l1, l2), pe=np_lambda.pseudo_energy(cc, l1, l2))
    keep = cc.t1, cc.t2
    cc.t1, cc.t2 = t1, t2
    try:
        cc.iterate()                                                        # one T iteration from (t1, t2)
        r["t_next"] = cc.t1, cc.t2
    finally:
        cc.t1, cc.t2 = keep
    if c["src"] == "fock":
        assert min(np.max(np.abs(cc.f_ov)), np.max(np.abs(cc.f_oo)), np.max(np.abs(cc.f_vv))) > 1e-2
    _REF[name] = r
    return r


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.ccsd_set_fused(-1)
    e.close()


def _scalar(x, ref, what):
    err, bound = abs(x - ref), 1e-11 * max(1.0, abs(ref))
    print(what, "error", err, "bound", bound)
    assert err < bound, what


def _hbar_against(eng, I, tag):
    for name, key in HBAR.items():
        _close(eng.so_tensor(name), I[key], 1e-11, f"{tag} {name}")


def _lambda_pass(eng, r, tag, hbar=True):
    """so_lambda_init, the H-bar elements, the pseudo energy of the set l, one Jacobi step with G_vv / G_oo and both monitor sums, the
    density of the set l -> (l1_new, l2_new, density).  t and l are the shape's first set."""
    cc = r["c"]["cc"]
    (t1, t2), (l1, l2) = r["t"], r["l"]
    eng.so_set_amplitudes(t1, t2)
    eng.so_lambda_init(0)
    if hbar:
        _hbar_against(eng, r["I"], tag)
    eng.so_set_lambda(l1, l2)
    pe0, _, _ = eng.so_lambda_energy(1e-11, 1e-11)
    _scalar(pe0, r["pe"], f"{tag} pseudo energy of the set l")
    pe, rms, _ = eng.so_lambda_iterate(1e-11, 1e-11)
    n1, n2 = eng.so_lambda()
    _close((n1 - l1) * cc.D1, r["x"][0] - cc.D1 * l1, 1e-11, f"{tag} G1")
    _close((n2 - l2) * cc.D2, r["x"][1] - cc.D2 * l2, 1e-11, f"{tag} G2")
    _scalar(pe, np_lambda.pseudo_energy(cc, n1, n2), f"{tag} pseudo energy of the new l")
    _scalar(rms, float(np.sum((n2 - l2) ** 2)), f"{tag} sum of squared l2 changes")
    _close(eng.so_tensor("G_vv"), r["Gvv"], 1e-11, f"{tag} G_vv")
    _close(eng.so_tensor("G_oo"), r["Goo"], 1e-11, f"{tag} G_oo")
    eng.so_set_lambda(l1, l2)
    d = eng.so_density()
    _close(d, r["density"], 1e-11, f"{tag} density")
    assert np.array_equal(d, d.T)
    a1, a2 = eng.so_amplitudes()
    assert np.array_equal(a1, t1) and np.array_equal(a2, t2)              # bit for bit
    return n1, n2, d


def _t_step(eng, r, tag):
    """one T iteration from the shape's first amplitudes -> (t1, t2), checked against numpy"""
    eng.so_set_amplitudes(*r["t"])
    eng.so_iterate(1e-11, 1e-11)
    g1, g2 = eng.so_amplitudes()
    _close(g1, r["t_next"][0], 1e-11, f"{tag} t1 after one T iteration")
    _close(g2, r["t_next"][1], 1e-11, f"{tag} t2 after one T iteration")
    return g1, g2


@pytest.mark.parametrize("name", sorted(MID))
def test_every_term_at_mid_size_and_the_branches_it_ran_on(eng, capfd, monkeypatch, name):
    """The whole list of the module docstring in one engine, and -- from the launcher's own lines (AFESP_GETT_DEBUG) during
    so_lambda_init + so_lambda_iterate + so_density -- that the shape ran where it was chosen to run."""
    r = _ref(name)
    c = r["c"]
    _feed(eng, c)
    monkeypatch.setenv("AFESP_GETT_DEBUG", "1")
    capfd.readouterr()
    _lambda_pass(eng, r, name)
    cap = capfd.readouterr()
    monkeypatch.delenv("AFESP_GETT_DEBUG")
    print(cap.out, end="")                                                  # (the errors and bounds printed so far)
    err, ls = cap.err, [dict(zip(_FIELDS, map(int, m.groups()))) for m in LAUNCH.finditer(cap.err)]
    for l in ls:
        print("launch", {k: l[k] for k in ("M", "N", "K", "akc", "bkc", "wide", "tm", "tn", "split")})
    assert len(ls) >= 50, err
    o, v = EXTENTS[name]
    npo, npv = o * (o - 1) // 2, v * (v - 1) // 2
    ladder = [l for l in ls if l["M"] == npv and l["N"] in (npo, npo + 1) and l["K"] in (npv, npv + 1)]
    assert len(ladder) == 1, ladder                                         # so_ladder_bare's own launch, not a product of the planner
    if name == "fock_odd":
        # odd extents: every product of the planner stages 8 bytes.  The pair-form ladder runs on packed pair buffers of its own with
        # even extents (78 x 36 x 78) and stages 16 bytes legitimately: the one launch excepted, by its extents
        assert all(l["wide"] == 0 for l in ls if l is not ladder[0]) and len(ls) - 1 >= 50
        assert (ladder[0]["M"], ladder[0]["N"], ladder[0]["K"]) == (78, 36, 78)
        assert any(max(l["tm"], l["tn"]) > 1 for l in ls if l is not ladder[0])
    else:
        assert any(l["wide"] == 1 for l in ls)
        assert any(l["tm"] == 4 or l["tn"] == 4 for l in ls)
        assert any(l["split"] > 1 for l in ls)
    if name == "rhf_cap":
        # a tile that only the scoring block of gett_launch (M >= 2048, 128 x 128 by extent, 16-byte staging) hands out
        assert any(l["tm"] == 16 or (l["tm"] == 4 and l["tn"] == 2 and l["M"] >= 2048 and l["N"] > 64) for l in ls)
        assert any(max(l["M"], l["N"]) >= 32768 for l in ls)                # an offset table the device wrote
    # a second initialisation on the same state, other amplitudes: nothing of the first pass may show
    eng.so_set_amplitudes(*r["s"])
    eng.so_lambda_init(0)
    _hbar_against(eng, r["I2"], f"{name} second initialisation")
    s1, s2 = eng.so_lambda()
    assert np.array_equal(s1, r["s"][0]) and np.array_equal(s2, r["s"][1])
    # the T iteration on the scratch (so_AB, so_A, so_B) and the plan cache Lambda has used
    if name == "rhf_mid":
        runs = {}
        for mode in (0, 1):
            eng.ccsd_set_fused(mode)
            runs[mode] = _t_step(eng, r, f"{name} fused {mode}")
        eng.ccsd_set_fused(-1)
        for a, b, ref in zip(runs[0], runs[1], r["t_next"]):
            assert np.max(np.abs(a - b)) < 1e-12 * max(1.0, np.max(np.abs(ref)))
    else:
        _t_step(eng, r, name)


def test_device_built_tables_equal_the_host_enumeration_at_rhf_cap(monkeypatch):
    """AFESP_PLAN_VERIFY=1 in a fresh engine (no cached plan): every plan of the pass, those with device-built tables included, is
    compared with the host enumeration and the scanned alignment flags -- a difference is status 2."""
    from afesp_amd.capi import Engine
    r = _ref("rhf_cap")
    monkeypatch.setenv("AFESP_PLAN_VERIFY", "1")
    with Engine(0) as fresh:
        _feed(fresh, r["c"])
        _lambda_pass(fresh, r, "rhf_cap verified plans", hbar=False)
        _close(fresh.so_tensor("H_vvvo"), r["I"]["Hvvvo"], 1e-11, "rhf_cap verified plans H_vvvo")


@pytest.mark.parametrize("name", ["rhf_mid", "rhf_cap"])
def test_t1_products_on_the_tall_kernel(monkeypatch, name):
    """With AFESP_TALL_MIN at o^2 v the products of t1 with a four-index array (mbef,jf->mbej; mnef,if->mnie; ijef,mf->ijme: K = v,
    S = o, the tall operand's leading free index unit-stride) go to csrc/tall.hip: the counter rises in so_lambda_init and in
    so_lambda_iterate, every result matches numpy again, and the same run with AFESP_TALL=0."""
    from afesp_amd.capi import Engine
    r = _ref(name)
    o, v = EXTENTS[name]
    out = {}
    for tall in ("1", "0"):
        monkeypatch.setenv("AFESP_TALL_MIN", str(o * o * v))
        monkeypatch.setenv("AFESP_TALL", tall)
        with Engine(0) as fresh:
            _feed(fresh, r["c"])
            fresh.so_set_amplitudes(*r["t"])
            n0 = fresh.launch_counts()["tall"]
            fresh.so_lambda_init(0)
            n1 = fresh.launch_counts()["tall"]
            fresh.so_set_lambda(*r["l"])
            fresh.so_lambda_iterate(1e-11, 1e-11)
            n2 = fresh.launch_counts()["tall"]
            print(name, "AFESP_TALL", tall, "tall launches: init", n1 - n0, "iterate", n2 - n1)
            assert (n1 > n0 and n2 > n1) if tall == "1" else n2 == n0
            n1_, n2_, d = _lambda_pass(fresh, r, f"{name} tall {tall}")
            out[tall] = dict({k: fresh.so_tensor(k) for k in ("H_ovvo", "H_ooov", "H_vvvo", "H_ovoo")}, l1=n1_, l2=n2_, density=d)
    for k in out["1"]:
        _close(out["1"][k], out["0"][k], 1e-11, f"{name} {k} on the tall kernel against the gather kernel")


def test_intermediates_are_served_by_a_live_lambda_state_only(eng):
    """afesp_ccsd_so_get_tensor: the Lambda names need a Lambda state built for the current amplitudes (status 21 otherwise, as every
    Lambda entry point); the names of the T iteration are served as before."""
    from afesp_amd.capi import AfespError
    r = _ref("fock_odd")
    _feed(eng, r["c"])
    for name in list(HBAR) + ["G_vv", "G_oo"]:
        with pytest.raises(AfespError, match="status 21: .*no Lambda state"):
            eng.so_tensor(name)
    eng.so_set_amplitudes(*r["t"])
    eng.so_lambda_init(0)
    assert eng.so_tensor("H_vvvo").shape == (9, 13, 13, 13) and eng.so_tensor("H_ovoo").shape == (9, 13, 9, 9)
    assert not eng.so_tensor("G_vv").any()                                  # (no iteration yet: the zero-filled allocation)
    eng.so_set_amplitudes(*r["s"])
    for name in list(HBAR) + ["G_vv", "G_oo"]:
        with pytest.raises(AfespError, match="status 21: .*stale"):
            eng.so_tensor(name)
    assert np.array_equal(eng.so_tensor("t1"), r["s"][0]) and eng.so_tensor("f_ov").shape == (9, 13)
    with pytest.raises(AfespError, match="status 1: .*unknown tensor"):
        eng._chk(eng.L.afesp_ccsd_so_get_tensor(eng.h, b"H_vvvv", np.zeros(1), 1))
    eng.so_lambda_init(0)
    with pytest.raises(AfespError, match="status 1: .*buffer too small for H_ooov"):
        eng._chk(eng.L.afesp_ccsd_so_get_tensor(eng.h, b"H_ooov", np.zeros(9 * 9 * 9 * 13 - 1), 9 * 9 * 9 * 13 - 1))


# launches of one traced pass at rhf_cap whose line carries `(repacked)`, as counted on the device
REPACKED_AT_RHF_CAP = 0


def test_relayout_branch_count_at_rhf_cap(capfd, monkeypatch):
    """How many of Lambda's products take the planner's re-layout branch (contract.hip: a_ok / b_ok, repack_min) in one traced pass at
    rhf_cap, where operands exceed 4096 elements and free extents exceed AFESP_REPACK_MIN = 256: counted from the `(repacked)` mark of
    the AFESP_CONTRACT_TRACE lines and held to the count in REPACKED_AT_RHF_CAP."""
    from afesp_amd.capi import Engine
    r = _ref("rhf_cap")
    monkeypatch.setenv("AFESP_CONTRACT_TRACE", "1")
    with Engine(0) as fresh:
        _feed(fresh, r["c"])
        capfd.readouterr()
        _lambda_pass(fresh, r, "rhf_cap traced", hbar=False)
        cap = capfd.readouterr()
    print(cap.out, end="")
    err, lines = cap.err, TRACE.findall(cap.err)
    assert len(lines) >= 50, err[-2000:]
    packed = [l for l in lines if l[9] == "(repacked)"]
    sample = "contract mk    ,kn    >nm     M      40 N      50 K      60 akc 0 bkc 0 wide 0       1.0 us   0.00 TF     0.1 GB/s  (repacked)\n"
    assert TRACE.findall(sample)[0][9] == "(repacked)" and len(packed) == err.count("(repacked)")      # (the parser sees the mark)
    for l in packed:
        print("repacked", l)
    assert len(packed) == REPACKED_AT_RHF_CAP

