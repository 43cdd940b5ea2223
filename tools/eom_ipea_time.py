#!/usr/bin/env python3
"""One EOM-IP-CCSD and one EOM-EA-CCSD sigma build and one Davidson step of each with 4 roots, next to one Lambda iteration and one
EOM-EE sigma build, and the left-hand side of both sectors (a left sigma build, a left Davidson step, a Dyson call of
4 left and 4 right vectors), on the same spin-orbital state at the H2O/cc-pVTZ shape (n = 58, 10 electrons -> o = 10, v = 106 spin orbitals;
synthetic integrals as tools/eom_time.py).  Wall times of the calls, each synchronised by its own host read; the median of the repeats
after one warm call.  DESIGN.md 4.14 and 4.22 record the numbers."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-fortran-electronic-structure-program_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from afesp_amd import inputs
from afesp_amd.capi import Engine

n, nel = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (58, 10)
nroots, reps = 4, 7
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
    so, sv = eng.so_o, eng.so_v
    rng = np.random.default_rng(2)
    r1 = rng.uniform(-0.3, 0.3, (so, sv))
    r2 = rng.uniform(-0.3, 0.3, (so, so, sv, sv)); r2 = r2 - r2.transpose(1, 0, 2, 3); r2 = 0.5 * (r2 - r2.transpose(0, 1, 3, 2))
    a1, a2 = np.ascontiguousarray(r1.ravel(order="F")), np.ascontiguousarray(r2.ravel(order="F"))
    s1, s2 = np.zeros_like(a1), np.zeros_like(a2)
    one = lambda: eng._chk(eng.L.afesp_ccsd_so_eom_sigma(eng.h, 1, a1, a2, s1, s2))
    print("EE sigma, host in/out median %8.2f ms  (min %.2f, max %.2f): one vector with its two copies of %.1f MB" % (*median_ms(one), a2.nbytes / 1e6))
    for sector, title in ((eng.EOM_IP, "IP"), (eng.EOM_EA, "EA")):
        sh1, sh2 = eng.so_eom_ipea_shapes(sector)
        b1, b2 = rng.uniform(-0.3, 0.3, sh1), rng.uniform(-0.3, 0.3, sh2)
        b2 = 0.5 * (b2 - (b2.transpose(1, 0, 2) if sector == eng.EOM_IP else b2.transpose(0, 2, 1)))
        c1, c2 = np.ascontiguousarray(b1.ravel(order="F")), np.ascontiguousarray(b2.ravel(order="F"))
        d1, d2 = np.zeros_like(c1), np.zeros_like(c2)
        one = lambda: eng._chk(eng.L.afesp_ccsd_so_eom_ipea_sigma(eng.h, sector, 1, c1, c2, d1, d2))
        g0 = eng.launch_counts()
        one()
        g1 = eng.launch_counts()
        print("%s sigma, host in/out median %8.3f ms  (min %.3f, max %.3f): one vector with its two copies of %.2f MB; products: %d gather, %d tall"
              % (title, *median_ms(one), c2.nbytes / 1e6, g1["gett"] - g0["gett"], g1["tall"] - g0["tall"]))
        eng.so_eom_ipea_init(sector, nroots, 8 * nroots)
        eng.so_eom_ipea_guess(sector)
        eng.so_eom_ipea_iterate(sector, 1e-8)                               # (the guess step: nroots sigma builds)
        ts = []
        for it in range(5):
            t0 = time.perf_counter(); om, res, fl, ns, cv = eng.so_eom_ipea_iterate(sector, 1e-8); ts.append((time.perf_counter() - t0) * 1e3)
            print("%s Davidson step %d: %8.3f ms, %d sigma builds so far, omega[0] %.8f, residuals %s" % (title, it + 2, ts[-1], ns, om[0], np.array2string(res, precision=2)))
        print("%s Davidson step      median %8.3f ms for %d roots" % (title, float(np.median(ts)), nroots))
        one = lambda: eng._chk(eng.L.afesp_ccsd_so_eom_ipea_lsigma(eng.h, sector, 1, c1, c2, d1, d2))
        g0 = eng.launch_counts()
        one()
        g1 = eng.launch_counts()
        print("%s left sigma, host in/out median %8.3f ms  (min %.3f, max %.3f); products: %d gather, %d tall"
              % (title, *median_ms(one), g1["gett"] - g0["gett"], g1["tall"] - g0["tall"]))
        eng.so_eom_ipea_left_init(sector, nroots, 8 * nroots)
        eng.so_eom_ipea_left_guess(sector)
        eng.so_eom_ipea_left_iterate(sector, 1e-8)
        ts = []
        for it in range(5):
            t0 = time.perf_counter(); om, res, fl, ns, cv = eng.so_eom_ipea_left_iterate(sector, 1e-8); ts.append((time.perf_counter() - t0) * 1e3)
        print("%s left Davidson step median %8.3f ms for %d roots" % (title, float(np.median(ts)), nroots))
        X = [eng.so_eom_ipea_vector(sector, k) for k in range(nroots)]
        Y = [eng.so_eom_ipea_left_vector(sector, k) for k in range(nroots)]
        pair = lambda V: (np.stack([x[0] for x in V]), np.stack([x[1] for x in V]))
        print("%s Dyson call, %d left and %d right vectors, host in/out median %8.3f ms  (min %.3f, max %.3f)"
              % (title, nroots, nroots, *median_ms(lambda: eng.so_eom_ipea_dyson(sector, pair(Y), pair(X)))))
