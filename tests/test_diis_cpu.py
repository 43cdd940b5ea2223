"""The numpy restatement of update_diis_cc (tests/np_diis.py) pinned against the oracle without a GPU, and the inputs of the GPU
injection tests (tests/test_gpu_diis.py) checked for their conditioning."""
import numpy as np
import pytest

import molecules
import np_diis
import orc


@pytest.mark.parametrize("nerr", [2, 3, 8, 15])
def test_np_diis_reproduces_the_oracle_extrapolation(nerr):
    """orc.OracleCC on the (4, 9) synthetic system through nerr + 3 iterations (the ring wraps), in the call order of
    tests/test_gpu_cc.py: np_diis fed the oracle's amplitudes from before each orc_cc_diis_update gives the oracle's amplitudes after
    it, within 64 eps cond max|t| (np_diis.tolerance: the two eliminate in a different order and precision)."""
    o, v = 4, 9
    n, e, eri = molecules.synthetic_system(o, v, scale=0.05)
    cc = orc.OracleCC(o, v, eri, e, nerr)
    L = cc.L
    ref = np_diis.Diis(nerr)
    L.orc_cc_energy(cc.h, 1e-14, 1e-14)
    for it in range(nerr + 3):
        s = np_diis.flat(cc.t1, cc.t2)
        L.orc_cc_diis_save(cc.h); L.orc_cc_intermediates(cc.h); L.orc_cc_amplitudes(cc.h); L.orc_cc_energy(cc.h, 1e-14, 1e-14)
        t = np_diis.flat(cc.t1, cc.t2)
        assert L.orc_cc_diis_update(cc.h) == 0
        step = ref.push(t, s)
        assert step.n == min(it + 1, nerr) and step.slot == it % nerr
        assert step.c64 is not None
        err = np.max(np.abs(np_diis.flat(cc.t1, cc.t2) - step.t))
        assert err <= np_diis.tolerance(step), (it, err, np_diis.tolerance(step), step.cond)
        assert abs(float(np.sum(step.c)) - 1.0) < 64 * np_diis.EPS * step.cond


def test_float64_elimination_names_the_singular_inputs():
    """What `singular` means in tests/test_gpu_diis.py: the binary64 elimination by division meets a pivot that is exactly zero for two
    zero error vectors and for a duplicated error vector of squared norm 49 -- and for neither a single zero vector nor a single
    non-zero one."""
    o, v = 4, 9
    s0 = np_diis.dyadic(np.linspace(-0.1, 0.1, o * v + o * o * v * v))   # (s0 + 1) - s0 == 1 to the bit
    ref = np_diis.Diis(4)
    first = ref.push(s0, s0)
    assert first.c64 is not None and first.c64[0] == 1.0 and np.array_equal(first.t, s0)
    assert ref.push(s0, s0).c64 is None
    d = np_diis.flat(*np_diis.duplicate_vector(o, v))
    assert np.count_nonzero(d) == 49 and np.all(d[d != 0] == 1.0)
    ref = np_diis.Diis(4)
    first = ref.push(s0 + d, s0)
    assert first.c64 is not None and abs(first.c64[0] - 1.0) <= 4 * np_diis.EPS   # (1 / (1 / 49) / 49 need not be 1 to the bit)
    second = ref.push(s0 + d, s0)
    assert second.c64 is None and second.t is None
    assert np.all(ref.B[:2, :2] == 49.0)
    assert np_diis.eliminate_f64(np.full((2, 2), 49.0)) is None
    assert np_diis.eliminate_f64(np.array([[49.0]])) is not None
    # a regular vector behind a singular step (the ring has moved on): regular again once the duplicate has left a 2-slot ring
    ref = np_diis.Diis(2)
    ref.push(s0 + d, s0)
    assert ref.push(s0 + d, s0).c64 is None
    t1, t2 = np_diis.perturbations("spatial", o, v, 1, 5)[0]
    assert ref.push(s0 + np_diis.flat(t1, t2), s0).c64 is not None


@pytest.mark.parametrize("kind,o,v", [("spatial", 3, 5), ("spatial", 7, 21), ("spinorb", 4, 8), ("spinorb", 6, 12)])
def test_injected_vectors_are_well_conditioned(kind, o, v):
    """The condition the GPU injection tests put on their inputs, checked here with np_diis alone: cond < 1e6 at every push of every
    history length; and the vectors carry the symmetry they claim."""
    for nerr in np_diis.INJECT_NERR:
        ds = np_diis.perturbations(kind, o, v, 2 * nerr + 2, seed=1000 * o + 10 * v + nerr)
        s0 = np.zeros(o * v + o * o * v * v)
        ref = np_diis.Diis(nerr)
        for t1, t2 in ds:
            if kind == "spatial":
                assert np.array_equal(t2, t2.transpose(1, 0, 3, 2))
            else:
                assert np.array_equal(t2, -t2.transpose(1, 0, 2, 3)) and np.array_equal(t2, -t2.transpose(0, 1, 3, 2))
            nrm = np.sqrt(np.sum(t1 * t1) + np.sum(t2 * t2))
            assert 0.5e-2 * (1 - 1e-12) <= nrm <= 2e-2 * (1 + 1e-12)
            step = ref.push(s0 + np_diis.flat(t1, t2), s0)
            assert step.cond < 1e6, (nerr, step.n, step.cond)
            assert step.c64 is not None
