"""The DIIS extrapolation on its own, against the numpy restatement of update_diis_cc (tests/np_diis.py): the device path
(diis_push_kernel, diis_solve_kernel, lincomb_kernel) of the call-by-call iteration and of every spin-orbital solve, the two-kernel
tail (cc_tail_kernel<NYT, YSW>, cc_finalize_kernel, the host elimination, lincomb_vals_kernel) of the launch-fused and the
large-system iteration, and the half-history sums of a large system -- at every history length 2..15, through ring wraps, at singular
systems and at the limits.

Injection: after ccsd_energy and one call-by-call iteration the state's saved amplitudes are s0 and no tail is pending; each
set_amplitudes(s0 + d_k) + diis() then pushes the error vector d_k, and the reference is fed the same.  Every comparison is within
np_diis.tolerance = 64 eps cond max|t| with the condition number of that step's augmented matrix; the injected d_k are well
conditioned by construction (cond < 1e6, tests/test_diis_cpu.py)."""
import numpy as np
import pytest

import molecules
import np_diis
import orc

pytestmark = pytest.mark.gpu

TIGHT = (1e-14, 1e-14)   # never converged: iterate always iterates


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.ccsd_set_fused(-1)
    e.close()


class Spatial:
    """The closed-shell state of an engine behind the four calls the tests need, amplitudes as one flat vector [t1 ; t2]."""
    kind = "spatial"

    def __init__(self, eng, o, v, nerr, scale=0.05):
        self.eng, self.o, self.v = eng, o, v
        n, e, eri = molecules.synthetic_system(o, v, scale=scale, seed=100 * o + v)
        self.system = (e, eri)
        eng.ccsd_init(o, v, e, eri, nerr)

    def energy(self):
        return self.eng.ccsd_energy(*TIGHT)

    def iterate(self):
        return self.eng.ccsd_iterate(*TIGHT)

    def diis(self):
        self.eng.ccsd_diis()

    def amps(self):
        return np_diis.flat(*self.eng.amplitudes())

    def set(self, x):
        self.eng.set_amplitudes(*np_diis.unflat(x, self.o, self.v))


class SpinOrb:
    kind = "spinorb"

    def __init__(self, eng, n, nel, nerr, scale=0.05):
        self.eng, self.o, self.v = eng, nel, 2 * n - nel
        _, e, eri = molecules.synthetic_system(nel // 2, n - nel // 2, scale=scale, seed=7 + n)
        eng.init_cc_spinorb(n, nel, e, eri, nerr)

    def energy(self):
        return self.eng.so_energy(*TIGHT)

    def iterate(self):
        return self.eng.so_iterate(*TIGHT)

    def diis(self):
        self.eng.so_diis()

    def amps(self):
        return np_diis.flat(*self.eng.so_amplitudes())

    def set(self, x):
        self.eng.so_set_amplitudes(*np_diis.unflat(x, self.o, self.v))


def _make(eng, kind, a, b, nerr, **kw):
    return Spatial(eng, a, b, nerr, **kw) if kind == "spatial" else SpinOrb(eng, a, b, nerr, **kw)


def _start(st, s0=None):
    """ccsd_energy, then one call-by-call iteration: the saved amplitudes are s0 (handed in, else the initial ones), no tail pending."""
    st.energy()
    if s0 is None:
        s0 = st.amps()
    else:
        st.set(s0)
    st.eng.ccsd_set_fused(0)
    st.iterate()
    return s0


def _check(tag, got, step):
    err = float(np.max(np.abs(got - step.t)))
    tol = np_diis.tolerance(step)
    print(f"{tag}: n {step.n} slot {step.slot} cond {step.cond:.3e} err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (tag, step.n, step.slot, err, tol)


def _inject(st, ref, s0, ds, tag):
    for k, (t1, t2) in enumerate(ds):
        t = s0 + np_diis.flat(t1, t2)
        st.set(t)
        st.diis()
        got = st.amps()
        step = ref.push(t, s0)
        assert step.cond < 1e6, (tag, k, step.cond)   # a condition on the inputs
        _check(f"{tag} push {k}", got, step)


def _walk(st, ref, count, tag):
    """`count` real iterations, each followed by diis(): the reference pushes what the engine held before and after the iteration."""
    for it in range(count):
        s = st.amps()
        st.iterate()
        x = st.amps()
        st.diis()
        got = st.amps()
        step = ref.push(x, s)
        _check(f"{tag} iteration {it}", got, step)
    return step


# ------------------------------------------------------------------------------------------------ a. device path, every length
@pytest.mark.parametrize("nerr", np_diis.INJECT_NERR)
@pytest.mark.parametrize("kind,a,b", [("spatial",) + x for x in np_diis.SPATIAL_EXTENTS] + [("spinorb",) + x for x in np_diis.SPINORB_EXTENTS])
def test_device_path_every_history_length(eng, kind, a, b, nerr):
    """diis_push_kernel / diis_solve_kernel / lincomb_kernel with 2 nerr + 2 pushes: every slot overwritten once (twice for nerr = 2), every
    accumulator up to index 14, on a vector shorter than one block and on one that is no multiple of the block."""
    st = _make(eng, kind, a, b, nerr)
    s0 = _start(st)
    ds = np_diis.perturbations(kind, st.o, st.v, 2 * nerr + 2, seed=1000 * st.o + 10 * st.v + nerr)
    _inject(st, np_diis.Diis(nerr), s0, ds, f"{kind} ({a},{b}) nerr {nerr}")
    eng.ccsd_set_fused(-1)


# ------------------------------------------------------------------------------------ b. the two-kernel tail on a pre-filled history
TAIL_CASES = [(15, 0), (15, 1), (15, 3), (15, 4), (15, 7), (15, 8), (15, 11), (15, 14),   # ny = 1, 2, 4, 5, 8, 9, 12, 15
              (2, 1), (5, 4), (9, 8),                                                      # ... with other strides of B
              (4, 6), (12, 14), (15, 17)]                                                  # k >= nerr: the slot has wrapped


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("nerr,k", TAIL_CASES)
def test_tail_on_a_prefilled_history(eng, nerr, k, large, monkeypatch):
    """k vectors injected through the device path, then real iterations on the two-kernel tail: the tail pushes x - s into the next slot
    with ny = min(k + 1, nerr) rows (cc_tail_kernel<4>, <8>, <16>), cc_finalize_kernel hands B to the host, and afesp_ccsd_diis solves there.
    Two more iterate + diis pairs check that B and the counters pass between the two paths.  large: the large-system tail
    (cc_tail_kernel<NYT, true>) with full sums -- afesp_ccsd_set_amplitudes switches the half sums off while its vector is in the history."""
    if large:
        monkeypatch.setenv("AFESP_SMALL_MAX", "0")
        monkeypatch.setenv("AFESP_RING_TG_MIN", "1")
        monkeypatch.setenv("AFESP_LARGE_TAIL", "0")   # (the first iteration call by call)
    st = Spatial(eng, 4, 9, nerr)
    s0 = _start(st)
    ref = np_diis.Diis(nerr)
    tag = f"{'large' if large else 'fused'} tail nerr {nerr} k {k}"
    _inject(st, ref, s0, np_diis.perturbations("spatial", 4, 9, k, seed=77 * nerr + k), tag)
    if large:
        monkeypatch.setenv("AFESP_LARGE_TAIL", "1")
    eng.ccsd_set_fused(1)
    step = _walk(st, ref, 1, tag)
    assert step.n == min(k + 1, nerr) and step.slot == k % nerr
    _walk(st, ref, 2, tag)
    eng.ccsd_set_fused(-1)


# --------------------------------------------------------------------------------------------- c. half-history sums past 8 rows
# The oracle needs 17 iterations at this scale (13 at 0.05, 16 at 0.07), so ny reaches 12 and the ring wraps
HALF_SCALE = 0.08


def test_half_history_sums_with_twelve_vectors(eng, monkeypatch):
    """A large system sums its DIIS overlaps over a <= b only (cc_tail_kernel<NYT, true> with p.half, the elements a < b twice) as long
    as every history vector is the solver's own: reached by a real solve only.  nerr = 12 on the large-system path, every iteration
    energy and rms against the oracle, which sums everything."""
    monkeypatch.setenv("AFESP_SMALL_MAX", "0")
    monkeypatch.setenv("AFESP_RING_TG_MIN", "1")
    monkeypatch.setenv("AFESP_LARGE_TAIL", "1")
    o, v, nerr = 4, 9, 12
    n, e, eri = molecules.synthetic_system(o, v, scale=HALF_SCALE)
    cc = orc.OracleCC(o, v, eri, e, nerr)
    eng.ccsd_init(o, v, e, eri, nerr)
    nit, en, rm = eng.do_ccsd_spatial(60, 1e-10, 1e-10)
    onit, oen, orm = cc.solve(60, 1e-10, 1e-10)
    for it in range(min(nit, onit) + 1):
        print(f"half sums iteration {it}: dE {abs(en[it] - oen[it]):.3e} drms {abs(rm[it] - orm[it]):.3e}")
    assert onit >= 15, onit
    assert nit == onit, (nit, onit)
    assert np.max(np.abs(en[:nit + 1] - oen[:nit + 1])) < 1e-10 and np.max(np.abs(rm[:nit + 1] - orm[:nit + 1])) < 1e-10


# ------------------------------------------------------------------------------------------------------------ d. singular systems
def _expect_solve_failure(call):
    from afesp_amd.capi import AfespError
    try:
        call()
    except AfespError as ex:
        assert "status 4" in str(ex) and "Linear solve failed" in str(ex), str(ex)
        return True
    return False


@pytest.mark.parametrize("case", ["zero", "duplicate"])
@pytest.mark.parametrize("kind,a,b", [("spatial", 4, 9), ("spinorb", 9, 6)])
def test_singular_system_on_the_device_path(eng, kind, a, b, case):
    """Two zero error vectors, and a non-zero error vector twice (49 entries 1.0: B = [[49, 49], [49, 49]], where the binary64 elimination
    by division meets a pivot that is exactly zero): the solve reports the reference's error (ccsd.f90:666) at the next energy
    evaluation, as np_diis.eliminate_f64 says it must; the flag is then clear, and with a regular vector in place of the older
    duplicate (a ring of two slots) the extrapolation matches the reference again."""
    st = _make(eng, kind, a, b, 2)
    st.energy()
    s0 = _start(st, np_diis.dyadic(st.amps()))   # (s0 + 1) - s0 == 1 to the bit
    ref = np_diis.Diis(2)
    d = np_diis.flat(*np_diis.duplicate_vector(st.o, st.v)) if case == "duplicate" else np.zeros(s0.size)
    t = s0 + d
    st.set(t)
    st.diis()
    first = ref.push(t, s0)
    assert first.c64 is not None   # one vector: regular, coefficient 1 (to the bit where B = 0: the pivots are the -1 of the border)
    _check(f"{kind} {case} first push", st.amps(), first)
    assert case != "zero" or np.array_equal(st.amps(), s0)
    st.energy()
    st.set(t)
    st.diis()
    second = ref.push(t, s0)
    assert second.c64 is None and np.all(ref.B == (49.0 if case == "duplicate" else 0.0))
    raised = _expect_solve_failure(st.energy)
    if not raised:
        print(f"{kind} {case}: no failure reported, max |t| after the extrapolation {np.max(np.abs(st.amps())):.3e}")
    assert raised
    st.energy()   # the flag is cleared: no second report
    r1, r2 = np_diis.perturbations(kind, st.o, st.v, 1, seed=31)[0]
    t = s0 + np_diis.flat(r1, r2)
    st.set(t)
    st.diis()
    _check(f"{kind} {case} recovery", st.amps(), ref.push(t, s0))
    st.energy()
    eng.ccsd_set_fused(-1)


@pytest.mark.parametrize("case", ["zero", "duplicate"])
def test_singular_system_on_the_fused_tail(eng, case):
    """The same two systems on the host elimination behind the two-kernel tail, where the failure surfaces in afesp_ccsd_diis itself.  The
    tail's error vector is that of a real iteration, so the integrals are all zero here: every iteration then returns exact zeros whatever
    it starts from, its error vector is minus the amplitudes it started from, and no value depends on rounding.  Afterwards the same
    engine walks three iterations of an ordinary system."""
    o, v, nerr = 4, 9, 4
    n, e, eri = molecules.synthetic_system(o, v, scale=0.05)
    eng.ccsd_set_fused(1 if case == "zero" else 0)
    eng.ccsd_init(o, v, e, np.zeros_like(eri), nerr)
    st = Spatial.__new__(Spatial)
    st.eng, st.o, st.v = eng, o, v
    st.energy()
    s0 = st.amps()
    assert not s0.any()
    ref = np_diis.Diis(nerr)
    if case == "zero":
        st.iterate()
        st.diis()
        assert ref.push(s0, s0).c64 is not None and np.array_equal(st.amps(), s0)
        st.iterate()
        assert ref.push(s0, s0).c64 is None
    else:
        d = np_diis.flat(*np_diis.duplicate_vector(o, v))
        st.iterate()                    # call by call: the saved amplitudes are zero
        st.set(d)
        st.diis()
        first = ref.push(d, s0)
        assert first.c64 is not None
        _check("fused tail duplicate first push", st.amps(), first)
        eng.ccsd_set_fused(1)
        st.set(-d)
        st.iterate()                    # the tail pushes 0 - (-d) = d
        x = st.amps()
        assert not x.any()
        assert ref.push(x, -d).c64 is None and np.all(ref.B[:2, :2] == 49.0)
    assert _expect_solve_failure(st.diis)
    st = Spatial(eng, o, v, 3)
    st.energy()
    _walk(st, np_diis.Diis(3), 3, f"fused tail {case} recovery")
    st.energy()
    eng.ccsd_set_fused(-1)


# ----------------------------------------------------------------------------------------------------------------------- e. limits
def test_history_length_limits(eng):
    """15 vectors is the limit of both solvers (one wave holds the 17 x 17 augmented system), 16 is refused by name and leaves a usable
    engine; one vector switches DIIS off (ccsd.f90:593-595): diis() leaves the amplitudes bit for bit."""
    from afesp_amd.capi import AfespError
    o, v = 3, 5
    n, e, eri = molecules.synthetic_system(o, v, scale=0.05)
    _, eso, eriso = molecules.synthetic_system(2, 4, scale=0.05, seed=13)
    eng.ccsd_init(o, v, e, eri, 15)
    eng.init_cc_spinorb(6, 4, eso, eriso, 15)
    for init in (lambda m: eng.ccsd_init(o, v, e, eri, m), lambda m: eng.init_cc_spinorb(6, 4, eso, eriso, m)):
        with pytest.raises(AfespError, match=r"status 1: .*ccsd_diis_n_errmat"):
            init(16)
        init(8)
    ref = np_diis.Diis(8)
    st = Spatial.__new__(Spatial)
    st.eng, st.o, st.v = eng, o, v
    st.energy()
    eng.ccsd_set_fused(0)
    _walk(st, ref, 2, "after a refused init")
    eng.init_cc_spinorb(6, 4, eso, eriso, 8)
    so = SpinOrb.__new__(SpinOrb)
    so.eng, so.o, so.v = eng, 4, 8
    so.energy()
    _walk(so, np_diis.Diis(8), 2, "after a refused spin-orbital init")
    for st in (Spatial(eng, o, v, 1), SpinOrb(eng, 6, 4, 1)):
        st.energy()
        st.iterate()
        x = st.amps()
        st.diis()
        assert np.array_equal(st.amps(), x)
        st.set(x + 1.0)
        st.diis()
        assert np.array_equal(st.amps(), x + 1.0)
    eng.ccsd_set_fused(-1)


# ------------------------------------------------------------------------------ f. amplitudes set between iterate and diis
def test_diis_extrapolates_the_amplitudes_current_at_the_call(eng):
    """iterate, set_amplitudes(x), diis: update_diis_cc pushes the amplitudes it is handed (ccsd.f90:640-646), so x enters the history --
    call by call, and launch-fused too, where the tail of the iteration has pushed the iteration's own result already."""
    o, v, nerr = 4, 9, 4
    d = np_diis.flat(*np_diis.perturbations("spatial", o, v, 1, seed=4)[0])
    xset, out = None, {}
    for mode in (0, 1):
        eng.ccsd_set_fused(mode)
        st = Spatial(eng, o, v, nerr)
        st.energy()
        ref = np_diis.Diis(nerr)
        _walk(st, ref, 2, f"fused {mode}")
        s = st.amps()
        st.iterate()
        if xset is None:
            xset = st.amps() + d
        st.set(xset)
        st.diis()
        got = st.amps()
        step = ref.push(xset, s)
        _check(f"fused {mode} handed-in amplitudes", got, step)
        out[mode] = (got, step)
    # (each run against the reference on its OWN history, which differs between the two by rounding: hence the third term)
    bound = np_diis.tolerance(out[0][1]) + np_diis.tolerance(out[1][1]) + float(np.max(np.abs(out[0][1].t - out[1][1].t)))
    assert np.max(np.abs(out[0][0] - out[1][0])) <= bound
    eng.ccsd_set_fused(-1)
