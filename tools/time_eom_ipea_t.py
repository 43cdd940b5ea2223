"""Cost of the EOM-IP / EOM-EA triples correction (afesp_ccsd_so_eom_ipea_t) per state against (T) (afesp_ccsd_so_t) and one left sigma
build of the sector (afesp_ccsd_so_eom_ipea_lsigma) in the same run, on the shapes of tools/time_eom_t.py (o = 10, v = 106 spin orbitals,
n = 58) and of H2O / cc-pVDZ (o = 10, v = 38, n = 24), synthetic integrals: 120 triples for IP, 45 pairs for EA.

Per call: the host's wall time of the whole synchronous call (median of --reps after --warmup calls) and the split of the device time into
the GEMM part (the operand build and the contract() products of a chunk) and the contraction kernel from the driver's own HIP events
(afesp_profile).  The correction is called with --states states at once; its figures are divided by that number.  Its wall time includes the
upload of the vectors, the two intermediates U and Y and the host read that ends each state.  The vectors are random -- nothing launched
depends on their values.

    python tools/time_eom_ipea_t.py [--reps 10] [--warmup 2] [--states 2] [--n 58]      -> one JSON line
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
    ap.add_argument("--n", type=int, default=58, help="spatial orbitals (58: the H2O/cc-pVTZ shape, 24: H2O/cc-pVDZ); 10 electrons")
    args = ap.parse_args()
    from afesp_amd import inputs
    from afesp_amd.capi import Engine
    n, nel = args.n, 10
    o = nel // 2
    e = np.concatenate([-2.0 + np.arange(o) / (o - 1), 1.0 + 2.0 * np.arange(n - o) / (n - o - 1)])
    eri = 0.02 * (2.0 * np.random.default_rng(1).random(inputs.neri(n)) - 1.0)
    ns = args.states
    out = {}
    with Engine(0) as eng:
        eng.init_cc_spinorb(n, nel, e, eri, 8, foo_as_published=True)
        eng.so_energy()
        for _ in range(4):
            eng.so_iterate()
            eng.so_diis()
        eng.so_lambda_init(0)
        os_, vs_ = eng.so_o, eng.so_v
        rng = np.random.default_rng(2)
        out["shape"] = {"o": os_, "v": vs_}
        out["states"] = ns
        out["t"] = measure(eng, eng.do_ccsd_t_spinorb, args.reps, args.warmup)
        for sector, name in ((eng.EOM_IP, "ip"), (eng.EOM_EA, "ea")):
            sh1, sh2 = eng.so_eom_ipea_shapes(sector)

            def vec():
                x1, x2 = rng.uniform(-0.3, 0.3, sh1), rng.uniform(-0.3, 0.3, sh2)
                return x1, 0.5 * (x2 - (x2.transpose(1, 0, 2) if sector == eng.EOM_IP else x2.transpose(0, 2, 1)))
            L, R = [vec() for _ in range(ns)], [vec() for _ in range(ns)]
            omega = 0.3 + 0.05 * np.arange(ns)
            ls = measure(eng, lambda: float(eng.so_eom_ipea_lsigma(sector, *L[0])[0].ravel()[0]), args.reps, args.warmup)
            et = measure(eng, lambda: eng.so_eom_ipea_t(sector, omega, L, R).tolist(), args.reps, args.warmup)
            per_state = {k: et[k] / ns for k in ("wall_ms_median", "wall_ms_min", "gemm_ms", "orbit_ms")}
            per_state["chunks"] = et["chunks"] // ns
            items = eng.so_eom_ipea_t_nitems(sector)
            # the products of both sides: IP 3 images of v^2 per triple, EA 3 of v^3 per pair, summation lengths as in eom_ipea_t_so.hip
            flop = 2.0 * items * (3 * vs_**2 * (3 * vs_ + 3 * os_) if sector == eng.EOM_IP else vs_**3 * (4 * vs_ + 2 * os_ + vs_ + 2 * os_))
            out[name] = {"items": items, "lsigma": ls, "eom_ipea_t": et, "per_state": per_state,
                         "share_of_wall": {"gemm": per_state["gemm_ms"] / per_state["wall_ms_median"],
                                           "contraction": per_state["orbit_ms"] / per_state["wall_ms_median"]},
                         "ratio_wall": {"per_state/t": per_state["wall_ms_median"] / out["t"]["wall_ms_median"],
                                        "per_state/lsigma": per_state["wall_ms_median"] / ls["wall_ms_median"]},
                         "gemm_tflops": flop / per_state["gemm_ms"] / 1e9 if per_state["gemm_ms"] else None}
        out["t_after"] = measure(eng, eng.do_ccsd_t_spinorb, args.reps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
