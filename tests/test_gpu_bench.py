"""`bench.py` as every change is measured with it: a plain run (set-up, warm-up, timed steps, the line) and its `--dump-outputs`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(tmp_path, tag, steps):
    out = tmp_path / tag
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "n2", "--steps", str(steps),
                          "--warmup", "2", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    return line, {f[:-4]: np.load(out / f) for f in os.listdir(out)}


def test_plain_run_line_and_dumped_outputs(tmp_path):
    """The headline fields and nothing measured beside the steps; the dump holds the last step's results (its (T) sums are the
    line's `e_t`), and a second run from the same seeded inputs computes the same numbers."""
    line, out = _plain(tmp_path, "a", 4)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 4 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    for key in ("roofline", "cpu_baseline", "ao2mo", "ccsd_iter_paths", "h2o_tz_same_run", "real_molecules_same_run"):
        assert key not in line, key
    assert sorted(out) == ["ccsd_energy_residual", "t1", "t2", "t_energies"]
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["t_energies"], np.array(line["e_t"]))
    assert out["t1"].shape == (7, 21) and out["t2"].size == 7 * 7 * 21 * 21 and np.all(np.isfinite(out["t2"]))
    _, out2 = _plain(tmp_path, "b", 4)
    for name in out:
        assert np.allclose(out[name], out2[name], rtol=1e-12, atol=1e-15), name
