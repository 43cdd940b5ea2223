"""Cost of the EOM-CCSD triples correction (afesp_ccsd_so_eom_t) per state against (T) (afesp_ccsd_so_t) and Lambda-CCSD(T)
(afesp_ccsd_so_lambda_t) in the same run, on the shape of tools/time_lambda_t.py: o = 10, v = 106 spin orbitals, synthetic integrals,
120 triples.

Per call: the host's wall time of the whole synchronous call (median of --reps after --warmup calls) and the split of the device time into
the GEMM launches and the orbit pass from the driver's own HIP events (afesp_profile).  The EOM call is made with --states states at once;
its figures are divided by that number.  Its wall time includes what no other call has: the upload of the vectors, the six contractions of
gR and the operand build, per state.  The vectors are random and of the amplitudes' size -- nothing launched depends on their values.

    python tools/time_eom_t.py [--reps 10] [--warmup 2] [--states 2] [--gett]      -> one JSON line
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-fortran-electronic-structure-program_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_lambda_t import measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--states", type=int, default=2)
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
    ns = args.states
    with Engine(0) as eng:
        eng.init_cc_spinorb(n, nel, e, eri, 8, foo_as_published=True)
        eng.so_energy()
        for _ in range(4):
            eng.so_iterate()
            eng.so_diis()
        eng.so_lambda_init(0)
        l1, l2 = eng.so_lambda()
        eng.so_set_lambda(0.9 * l1, 1.1 * l2)
        rng = np.random.default_rng(2)
        vec = lambda: (l1 * rng.uniform(0.5, 1.5, l1.shape), l2 * rng.uniform(0.5, 1.5))
        L, R = [vec() for _ in range(ns)], [vec() for _ in range(ns)]
        omega = 0.1 + 0.05 * np.arange(ns)
        t = measure(eng, eng.do_ccsd_t_spinorb, args.reps, args.warmup)
        lt = measure(eng, eng.so_lambda_t, args.reps, args.warmup)
        et = measure(eng, lambda: eng.so_eom_t(omega, L, R).tolist(), args.reps, args.warmup)
        t_after = measure(eng, eng.do_ccsd_t_spinorb, args.reps, args.warmup)
        os_, vs_ = eng.so_o, eng.so_v
    per_state = {k: et[k] / ns for k in ("wall_ms_median", "wall_ms_min", "gemm_ms", "orbit_ms")}
    per_state["chunks"] = et["chunks"] // ns
    flop_t = (os_ * (os_ - 1) * (os_ - 2) // 6) * 3 * 2.0 * vs_**3 * (vs_ + os_)
    share = lambda d: {"gemm": d["gemm_ms"] / d["wall_ms_median"], "orbit": d["orbit_ms"] / d["wall_ms_median"]}
    print(json.dumps({"shape": {"o": os_, "v": vs_, "triples": os_ * (os_ - 1) * (os_ - 2) // 6}, "gemm": "gett" if args.gett else "tgemm",
                      "states": ns, "t": t, "lambda_t": lt, "eom_t": et, "eom_t_per_state": per_state, "t_after": t_after,
                      "share_of_wall": {"t": share(t), "lambda_t": share(lt), "eom_t": share(per_state)},
                      "ratio_wall": {"eom_t/t": per_state["wall_ms_median"] / t["wall_ms_median"],
                                     "eom_t/lambda_t": per_state["wall_ms_median"] / lt["wall_ms_median"]},
                      "ratio_gemm": {"eom_t/t": per_state["gemm_ms"] / t["gemm_ms"] if t["gemm_ms"] else None},
                      "ratio_orbit": {"eom_t/t": per_state["orbit_ms"] / t["orbit_ms"] if t["orbit_ms"] else None},
                      "gemm_tflops": {"t": flop_t / t["gemm_ms"] / 1e9 if t["gemm_ms"] else None,
                                      "lambda_t": 2 * flop_t / lt["gemm_ms"] / 1e9 if lt["gemm_ms"] else None,
                                      "eom_t": 3 * flop_t / per_state["gemm_ms"] / 1e9 if per_state["gemm_ms"] else None}}))


if __name__ == "__main__":
    main()
