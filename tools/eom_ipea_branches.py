#!/usr/bin/env python3
"""Prints the per-product tables of tests/test_gpu_eom_ipea_mid.py: every product of one EOM-IP and one EOM-EA sigma build at the three
mid-size shapes with its kernel extents, tile code, K slices and staging width, from the launcher's own lines (AFESP_GETT_DEBUG,
AFESP_CONTRACT_TRACE), and which of them the tall kernel takes once AFESP_TALL_MIN is o^2 v (tools/eom_branches.py, for the two sectors).
With --left: the same tables for the left sigma builds, for tests/test_gpu_eom_ipea_left_mid.py."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-fortran-electronic-structure-program_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))

CHILD = """
import sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {tests!r})
import os
import numpy as np
import np_eom_ipea
import np_lambda
from afesp_amd.capi import Engine
from test_gpu_lambda import _build_case, _feed
from test_gpu_lambda_mid import MID
name, sector = sys.argv[1], int(sys.argv[2])
c = _build_case(name, *MID[name])
rng = np.random.default_rng(7)
t = np_lambda.antisym_random(rng, c["o"], c["v"])
r = np_eom_ipea.random_vector(np.random.default_rng(9), sector, c["o"], c["v"])
with Engine(0) as eng:
    _feed(eng, c)
    eng.so_set_amplitudes(*t)
    eng.so_lambda_init(0)
    sys.stderr.write("SIGMA BEGINS\\n"); sys.stderr.flush()
    (eng.so_eom_ipea_lsigma if {left} else eng.so_eom_ipea_sigma)(sector, *r)
"""
LAUNCH = re.compile(r"gett_launch M (\d+) N (\d+) K (\d+) batch \d+ akc \d bkc \d wide (\d) -> tm (\d+) tn (\d+) tiles \d+ x \d+ split (\d+)")
TRACE = re.compile(r"contract (\S+)\s*,(\S+)\s*>(\S+)\s+M\s+(\d+) N\s+(\d+) K\s+(\d+) akc \d bkc \d wide (\d)[^\n]*?(\(repacked\)|\(tall\))?$")


def run(name, sector, tall_min=None):
    env = dict(os.environ, AFESP_GETT_DEBUG="1", AFESP_CONTRACT_TRACE="1")
    if tall_min is not None:
        env["AFESP_TALL_MIN"] = str(tall_min)
    src = CHILD.format(pkg=os.path.join(ROOT, "a-fortran-electronic-structure-program_amd"), tests=os.path.join(ROOT, "tests"), left="--left" in sys.argv)
    err = subprocess.run([sys.executable, "-c", src, name, str(sector)], env=env, capture_output=True, text=True, timeout=600, check=True).stderr
    rows, last = [], None
    for line in err.split("SIGMA BEGINS\n", 1)[1].splitlines():
        m = LAUNCH.search(line)
        if m:
            if last is not None:   # a launch with no trace line of its own: the EA pair-form ladder's, outside the planner
                rows.append(dict(form="pair-form ladder", M=last[0], N=last[1], K=last[2], wide=last[3], mark="", launch=last))
            last = m.groups()
            continue
        m = TRACE.search(line)
        if m:
            la, lb, lc, M, N, K, wide, mark = m.groups()
            if mark == "(tall)" and last is not None:   # (a tall product prints no launch line: the one before it was the ladder's)
                rows.append(dict(form="pair-form ladder", M=last[0], N=last[1], K=last[2], wide=last[3], mark="", launch=last))
                last = None
            rows.append(dict(form=f"{la},{lb}>{lc}", M=M, N=N, K=K, wide=wide, mark=mark or "", launch=last))
            last = None
    return rows, err


if __name__ == "__main__":
    from test_gpu_lambda_mid import EXTENTS
    names = ["rhf_mid", "fock_odd", "rhf_cap"]
    for sector, title in ((1, "IP"), (2, "EA")):
        cols = {}
        for name in names:
            plain, err = run(name, sector)
            o, v = EXTENTS[name]
            tall, _ = run(name, sector, o * o * v)
            if "--raw" in sys.argv:
                print(err)
            cells = []
            marks = iter([t for t in tall if t["form"] != "pair-form ladder"])
            for p in plain:
                t = dict(mark="") if p["form"] == "pair-form ladder" else next(marks)
                assert t["mark"] == "" or t["form"] == p["form"], (p, t)
                l = p["launch"]
                cell = f"{p['M']}x{p['N']}x{p['K']} " + (f"{l[4]},{l[5]} s{l[6]} w{l[3]}" if l else "(tall)")
                cells.append((p["form"], cell + (" T" if t["mark"] == "(tall)" else "") + (" R" if p["mark"] == "(repacked)" else "")))
            assert len([t for t in tall if t["form"] == "pair-form ladder"]) == len([p for p in plain if p["form"] == "pair-form ladder"])
            cols[name] = cells
        print(f"  {title} product        | " + " | ".join(f"{n} {EXTENTS[n]}".ljust(28) for n in names))
        for k in range(max(len(c) for c in cols.values())):
            form = next(c[k][0] for c in cols.values() if k < len(c))
            print(f"  {form:<17} | " + " | ".join((cols[n][k][1] if k < len(cols[n]) else "-").ljust(28) for n in names))
