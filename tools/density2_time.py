#!/usr/bin/env python3
"""One build of the two-particle density, one energy walk and one expectation value next to one Lambda iteration, on the same
spin-orbital state at the H2O/cc-pVTZ shape (n = 58, 10 electrons -> o = 10, v = 106 spin orbitals; synthetic integrals as
tools/so_time.py).  Wall times of the calls, each synchronised by its own host read; the median of the repeats after one warm call.
DESIGN.md 4.17 records the numbers."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-fortran-electronic-structure-program_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from afesp_amd import inputs
from afesp_amd.capi import Engine

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
    print("density2 energy      median %8.2f ms  (min %.2f, max %.2f): the one-particle density, sum f D on the host, six walks" % median_ms(lambda: eng.so_density2_energy()))
    m = eng.so_o + eng.so_v
    a = np.random.default_rng(2).uniform(-1.0, 1.0, (m, m))
    print("density2 expect      median %8.2f ms  (min %.2f, max %.2f): two (o+v)^2 matrices in, six walks" % median_ms(lambda: eng.so_density2_expect(a, a.T)))
    npv = eng.so_v * (eng.so_v - 1) // 2
    print("stored: %.1f MB dense blocks + %.1f MB pair form (a dense v^4 block would be %.1f MB)" % (
        8e-6 * (eng.so_o ** 4 + eng.so_o ** 3 * eng.so_v + 2 * eng.so_o ** 2 * eng.so_v ** 2 + eng.so_o * eng.so_v ** 3), 8e-6 * npv * npv, 8e-6 * eng.so_v ** 4))
