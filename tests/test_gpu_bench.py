"""bench.py's plain run on the GPU: `--steps` sets the number of timed steps, the result line carries the headline
fields and nothing that takes a run of its own, and `--dump-outputs DIR` writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

pytestmark = pytest.mark.gpu

STEPS, WARMUP = 3, 1


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HS_EVENT_TIMING")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out


def test_plain_line_has_the_headline_and_no_extras(plain_run):
    d, _ = plain_run
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["unit"] == "point-residuals/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value = point-residuals x steps / the timed loop's wall time; ms_per_step = that wall time / steps
    assert d["value"] == pytest.approx(d["config"]["point_residuals"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # what takes a run of its own is measured only with --full
    assert d["roofline"] is None and d["phase_ms_per_step"] is None and d["cpu_baseline"] is None
    assert "calls_ms" not in d and "speedup_vs_cpu" not in d


def test_dump_outputs_holds_the_last_timed_step(plain_run):
    d, out = plain_run
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 1000 * 1000
    n_res, n_pts, n_fr = d["config"]["point_residuals"], d["config"]["points"], d["config"]["frames"]
    assert got["energies"].shape == (STEPS,)  # one energy per timed step: --steps really sets their number
    assert np.all(np.isfinite(got["energies"])) and np.all(got["energies"] > 0)
    assert got["frames_pose"].shape == (n_fr, 7) and got["frames_state"].shape == (n_fr, 10)
    assert got["points_idepth"].shape == (n_pts,) and np.all(np.isfinite(got["points_idepth"]))
    assert got["residuals_energy"].shape == (n_res,) and got["residuals_JpJdF"].shape == (n_res, 8)
    # integer outputs arrive as float values: the residual states are HS_RES_IN / OOB / OUT (include/hs_types.h)
    assert set(np.unique(got["residuals_state"])) <= {0.0, 1.0, 2.0}
