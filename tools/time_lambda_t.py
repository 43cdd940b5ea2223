"""Cost of Lambda-CCSD(T) (afesp_ccsd_so_lambda_t) against (T) (afesp_ccsd_so_t, whose code path this leaves as it was) on the spin-orbital
H2O/cc-pVTZ shape that bench.py --full measures as CCSD(T)_spinorb: o = 10, v = 106 spin orbitals, synthetic integrals, 120 triples.

Two numbers per call: the host's wall time of the whole synchronous call (median of --reps after --warmup calls: operand copies and plan
cached, as a second shard finds them), and the split of the device time into the GEMM launches and the orbit pass from the driver's own
HIP events (afesp_profile).  A few CCSD iterations give t amplitudes of realistic size; Lambda is left at its start (l = t) and then set
to a perturbed copy, so that both operand sets are rebuilt once and the value differs from (T) -- neither changes what is launched.

    python tools/time_lambda_t.py [--reps 20] [--warmup 3] [--gett]      -> one JSON line
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-fortran-electronic-structure-program_amd"))


def measure(eng, call, reps, warmup):
    for _ in range(warmup):
        call()
    eng.profile(True)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        val = call()
        wall.append(time.perf_counter() - t0)
    p = eng.profile(False)
    return {"value": val, "wall_ms_median": 1e3 * float(np.median(wall)), "wall_ms_min": 1e3 * float(np.min(wall)),
            "gemm_ms": p["gemm_ms"] / reps, "orbit_ms": p["orbit_ms"] / reps, "chunks": p["gemm_launches"] // reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gett", action="store_true", help="the gather-GEMM back end (AFESP_T_GEMM=gett) instead of the LDS-DMA kernel")
    args = ap.parse_args()
    if args.gett:
        os.environ["AFESP_T_GEMM"] = "gett"
    from afesp_amd import inputs
    from afesp_amd.capi import Engine
    n, nel = 58, 10
    o = nel // 2
    e = np.concatenate([-2.0 + np.arange(o) / (o - 1), 1.0 + 2.0 * np.arange(n - o) / (n - o - 1)])
    eri = 0.02 * (2.0 * np.random.default_rng(1).random(inputs.neri(n)) - 1.0)
    with Engine(0) as eng:
        eng.init_cc_spinorb(n, nel, e, eri, 8, foo_as_published=True)
        eng.so_energy()
        for _ in range(4):
            eng.so_iterate()
            eng.so_diis()
        eng.so_lambda_init(0)
        l1, l2 = eng.so_lambda()
        eng.so_set_lambda(0.9 * l1, 1.1 * l2)
        t = measure(eng, eng.do_ccsd_t_spinorb, args.reps, args.warmup)
        lt = measure(eng, eng.so_lambda_t, args.reps, args.warmup)
        os_, vs_ = eng.so_o, eng.so_v
    flop_t = (os_ * (os_ - 1) * (os_ - 2) // 6) * 3 * 2.0 * vs_**3 * (vs_ + os_)
    print(json.dumps({"shape": {"o": os_, "v": vs_, "triples": os_ * (os_ - 1) * (os_ - 2) // 6}, "gemm": "gett" if args.gett else "tgemm",
                      "t": t, "lambda_t": lt,
                      "ratio_wall": lt["wall_ms_median"] / t["wall_ms_median"],
                      "ratio_gemm": lt["gemm_ms"] / t["gemm_ms"] if t["gemm_ms"] else None,
                      "ratio_orbit": lt["orbit_ms"] / t["orbit_ms"] if t["orbit_ms"] else None,
                      "gemm_tflops": {"t": flop_t / t["gemm_ms"] / 1e9 if t["gemm_ms"] else None,
                                      "lambda_t": 2 * flop_t / lt["gemm_ms"] / 1e9 if lt["gemm_ms"] else None}}))


if __name__ == "__main__":
    main()
