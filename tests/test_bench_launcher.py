"""bench.py's multi-GPU launcher on the CPU (no GPU, no library): `--gpus N` without a launcher starts N rank
processes with the torch.distributed.run environment, a WORLD_SIZE that disagrees with --gpus is an error, and a
node with fewer GPUs than --gpus fails loudly instead of printing a 1-GPU line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    env.update(kw)
    return env


def _run(args, env, timeout=180):
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_flag_starts_n_ranks(n):
    r = _run(["--gpus", str(n), "--plumbing-check", "--points", "2000"], _env())
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 prints the one line
    d = json.loads(lines[0])
    assert d["world"] == n and d["group_size"] == n and d["gpus_flag"] == n
    assert d["allreduce"] == n * (n + 1) / 2  # every rank joined the group with its own RANK
    # strong scaling: the metric's 2000-point window split p % N == rank, every point on exactly one rank
    assert sum(d["strong_shard_points"]) == 2000 and max(d["strong_shard_points"]) - min(d["strong_shard_points"]) <= 1


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "2", "--plumbing-check"], _env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_too_few_gpus_fails_loudly():
    # this container has no GPU: --gpus 2 must exit non-zero before starting any rank, not print an n_gpus: 1 line
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu"], _env())
    assert r.returncode != 0
    assert "visible GPUs" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_single_gpu_workloads_reject_gpus():
    r = _run(["--workload", "track", "--gpus", "2"], _env())
    assert r.returncode != 0 and "single-GPU" in (r.stderr + r.stdout)


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: every array lands as <name>.npy in float32 / float64 with its values kept, an array above its
    share of the budget as the same ascending sample of its rows in every run, other ranks under their own names."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)  # 4 arrays: 1000 B each
    big = np.arange(3000, dtype=np.float32).reshape(1000, 3)
    arrays = {"state": np.array([0, 1, 2, 255], np.uint8), "count": [7], "energy": np.array([1.5, 2.5]), "big": big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["big.npy", "count.npy", "energy.npy", "state.npy"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["state.npy"].tolist() == [0, 1, 2, 255] and got["count.npy"].tolist() == [7]
    assert got["energy.npy"].dtype == np.float64 and got["energy.npy"].tolist() == [1.5, 2.5]
    s = got["big.npy"]
    assert s.shape == (1000 // 12, 3) and sum(a.nbytes for a in got.values()) <= 4000
    rows = (s[:, 0] / 3).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(s, big[rows])  # whole rows of the array, in its order
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))
    bench.dump_outputs(str(tmp_path / "a"), {"energy": [3.0]}, rank=2)
    assert np.load(tmp_path / "a" / "energy_rank2.npy").tolist() == [3.0]
    assert np.load(tmp_path / "a" / "energy.npy").tolist() == [1.5, 2.5]


def test_count_gpus_reads_the_kfd_topology(tmp_path, monkeypatch):
    """The launcher counts GPUs from the KFD topology (nodes with SIMDs), narrowed by the visibility variables,
    without loading a HIP library."""
    sys.path.insert(0, ROOT)
    import bench
    for i, simds in enumerate([0, 1024, 1024, 1024]):  # node 0: the CPU
        d = tmp_path / str(i)
        d.mkdir()
        (d / "properties").write_text(f"cpu_cores_count {0 if simds else 64}\nsimd_count {simds}\narray_count 32\n")
    for v in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(v, raising=False)
    assert bench.count_gpus(str(tmp_path)) == 3
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,2")
    assert bench.count_gpus(str(tmp_path)) == 2
    assert bench.count_gpus(str(tmp_path / "absent")) == 0
