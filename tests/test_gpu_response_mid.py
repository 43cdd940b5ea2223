"""The operator vector xi of EOM-CCSD linear response (csrc/response_so.hip) at extents where its assemble kernel crosses its block and
LDS-tile edges: the shapes of tests/test_gpu_lambda_mid.py (MID: (o, v) = (10, 18), (9, 13), (12, 46)) and the two degenerate pair spaces,
o = 2 (a single i < j pair) and v = 2 (a single a < b pair).  Against the kernel's constants:

  * 64 occupied pairs per wave: 45, 36 and 66 pairs -- part of a wave, and at (12, 46) a second block column with 2 of its 64 lanes live;
  * 4 virtual pairs per block: 153, 78 and 1035 pairs -- 1035 and 153 leave a block with 3 and 1 of its 4 waves live;
  * rows of X~_oo staged 8 at a time: o = 10, 9, 12 take 8 + 2, 8 + 1 and 8 + 4 -- a second piece with a short tail at every MID shape;
  * rows of X~_vv staged in pieces of 32: v = 46 takes 32 + 14 (a second piece with a tail); v = 18 and 13 fit one piece.

xi only, at the tolerance of tests/test_gpu_response.py: 1e-12 x max(1, |xi|)."""
import pytest

from test_gpu_lambda import _build_case, _feed
from test_gpu_lambda_mid import EXTENTS, MID
from test_gpu_response import check_xi

pytestmark = pytest.mark.gpu

SHAPES = dict(MID)
SHAPES["one_occupied_pair"] = ("fock", 4, 1, 1, 211)                        # (o, v) = (2, 6)
SHAPES["one_virtual_pair"] = ("fock", 3, 2, 2, 212)                         # (o, v) = (4, 2)
SIZES = dict(EXTENTS, one_occupied_pair=(2, 6), one_virtual_pair=(4, 2))


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_xi_at_mid_size_and_at_single_pairs(eng, name):
    c = _build_case(name, *SHAPES[name])
    assert (c["o"], c["v"]) == SIZES[name]
    if name in MID:
        assert c["o"] > 8 and c["o"] % 8 != 0                                # more than one piece of 8 rows of X~_oo, with a tail
    if name == "rhf_cap":
        assert c["v"] > 32 and c["v"] % 32 != 0                             # more than one piece of 32 of a row of X~_vv, with a tail
    _feed(eng, c)
    check_xi(eng, c["o"], c["v"], name)
