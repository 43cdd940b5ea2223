#!/usr/bin/env python3
"""One orbital gradient, its pair-row kernel alone and one Z-vector solve next to one Lambda iteration and one density2 build, on the same
spin-orbital state at the H2O/cc-pVTZ shape (n = 58, 10 electrons -> o = 10, v = 106 spin orbitals; synthetic integrals as
tools/density2_time.py).  Wall times of the calls, each synchronised by its own host read, the median of 7 after one warm call; the
pair-row kernel by device events over 20 launches, with the bytes per second of its one pass over the pair matrix.
DESIGN.md 4.18 records the numbers."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-fortran-electronic-structure-program_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from afesp_amd import inputs
from afesp_amd.capi import AfespError, Engine

n, nel = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (58, 10)
reps = 7
o = nel // 2
e = np.concatenate([-2.0 + np.arange(o) / max(o - 1, 1), 1.0 + 2.0 * np.arange(n - o) / max(n - o - 1, 1)])
eri = 0.02 * (2.0 * np.random.default_rng(1).random(inputs.neri(n)) - 1.0)


def median_ms(call):
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


with Engine(0) as eng:
    eng.init_cc_spinorb(n, nel, e, eri, 8, foo_as_published=True)
    eng.so_energy()
    for it in range(4):
        eng.so_iterate(); eng.so_diis()
    eng.so_lambda_init(0)
    print("Lambda iteration     median %8.2f ms  (min %.2f, max %.2f)" % median_ms(lambda: eng.so_lambda_iterate()))
    print("density2 build       median %8.2f ms  (min %.2f, max %.2f)" % median_ms(lambda: eng.so_density2_build()))
    print("orbital gradient     median %8.2f ms  (min %.2f, max %.2f): D, f D, 14 dense products, two pair-row launches, the assemble" % median_ms(lambda: eng.so_orbital_gradient(1)))
    before = eng.launch_counts()
    eng.so_orbital_gradient(1)
    after = eng.launch_counts()
    so, sv = eng.so_o, eng.so_v
    passes = -(-(sv * -(-so // 8)) // 256)
    print("launches of one gradient: GEMM layer", {k: after[k] - before[k] for k in after}, "(afesp_launch_counts) + 2 axpby + 3 kernels (density "
          "assemble, F, gradient assemble) + 2 x %d pair-row" % passes)
    npv = sv * (sv - 1) // 2
    for which, what in ((0, "<ab||cd> Gamma_ibcd"), (1, "Gamma_abcd <ib||cd>")):
        ms = sorted(eng.so_relax_pair_row(which, 20)[1] for _ in range(reps))[reps // 2]
        nbytes = 8.0 * (npv * npv + so * sv * npv)     # the stored pair matrix once, the (i,b) slices of Q of the c<d columns once
        print("pair-row kernel %d    median %8.4f ms  %s: %.1f MB, %.2f TB/s, %.2f GFLOP -> %.2f TFLOP/s" % (
            which, ms, what, 1e-6 * nbytes, 1e-9 * nbytes / ms, 2e-9 * so * sv * sv * npv, 2e-9 * so * sv * sv * npv / ms))

    def solve():
        try:
            return eng.so_zvector_solve(1e-10, 100)
        except AfespError as err:                          # (synthetic integrals: the solve may stop at maxiter; the time per iteration stands)
            return None, eng.so_zvector_last[0], eng.so_zvector_last[1], str(err)
    r = solve()
    print("Z-vector solve       median %8.2f ms  (min %.2f, max %.2f):" % median_ms(solve), r[1], "iterations, residual", r[2],
          "(one gradient, then 2 products + 4 small launches and 2 host reads per iteration)")
