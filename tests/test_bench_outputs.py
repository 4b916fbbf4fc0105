"""CPU: bench.py --dump-outputs.

`--dump-outputs DIR` writes the tensors the last timed step returned as float32 /
float64 .npy files; above the byte budget every per-problem tensor keeps the same
fixed, seeded sample of problems."""
import json
import os
import subprocess
import sys
import types

import numpy as np

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))


def test_dry_run_dumps_the_last_steps_outputs(tmp_path):
    import bench_dry_standin as sd
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "1"
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--dry-run", "--batch", "3",
           "--steps", "2", "--warmup", "1", "--prewarm-s", "0", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert sorted(os.listdir(out)) == ["J.npy", "j_star.npy", "status.npy", "t_star.npy"]
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    ref = [sd.select_for(i) for i in range(3)]
    assert got["t_star"].tolist() == [r[0] for r in ref]
    assert np.array_equal(got["j_star"], np.array([r[1] for r in ref]))
    assert np.array_equal(got["J"], np.stack([r[2] for r in ref]))
    assert np.array_equal(got["status"], np.zeros(3))


def test_dump_outputs_samples_the_same_problems_above_the_budget(tmp_path, monkeypatch):
    import torch
    import bench
    Bn, N = 1000, 16
    g = torch.Generator().manual_seed(5)
    r = types.SimpleNamespace(J=torch.randn((Bn, N), generator=g, dtype=torch.float64),
                              j_star=torch.randn((Bn,), generator=g).float(),
                              t_star=torch.arange(Bn, dtype=torch.int64),
                              status=torch.zeros(Bn, dtype=torch.int32), efg=None)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40_000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), r)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == ["J", "j_star", "sample_index", "status", "t_star"]
    assert all(np.array_equal(a[k], b[k]) for k in a)  # the sample is fixed
    idx = a["sample_index"].astype(np.int64)
    assert 1 <= len(idx) < Bn and np.all(np.diff(idx) > 0)
    assert sum(v.nbytes for v in a.values()) <= 40_000
    assert a["J"].dtype == np.float64 and a["j_star"].dtype == np.float32
    assert a["t_star"].dtype == np.float64 and np.array_equal(a["t_star"], idx)
    assert np.array_equal(a["J"], r.J.numpy()[idx])
    assert np.array_equal(a["j_star"], r.j_star.numpy()[idx])
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 60_000_000)
    bench.dump_outputs(str(tmp_path / "c"), r)  # under the budget: everything, no index
    assert sorted(os.listdir(tmp_path / "c")) == ["J.npy", "j_star.npy", "status.npy", "t_star.npy"]
    assert np.array_equal(np.load(tmp_path / "c" / "J.npy"), r.J.numpy())
