"""bench.py's multi-rank launcher on the CPU (gloo, --dry-run: no HIP call).

The driver runs `bench.py --gpus N` both bare and under torch.distributed.run; either way the JSON line
must describe N ranks, and a launcher whose WORLD_SIZE disagrees with --gpus must be refused rather
than measured (the reference's multi-process use is scripts/train_dnerf.sh:3-12).  Also on the
CPU: the --dump-outputs writer and the options of a plain and a --full run."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def _env():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_bare_bench_spawns_n_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1"],
                       capture_output=True, text=True, timeout=240, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 2 and j["dry_run"] is True
    assert [p["rank"] for p in j["per_rank"]] == [0, 1]
    # each rank's own step result reached rank 0 (num_rendered stand-in = 1000 + rank)
    assert [p["num_rendered"] for p in j["per_rank"]] == [1000, 1001]
    assert j["ms_per_step"] == max(p["ms_per_step"] for p in j["per_rank"])


def test_driver_style_launch():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2",
                        "--dry-run", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=240, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 2 and len(j["per_rank"]) == 2


def test_world_size_mismatch_is_refused():
    env = _env()
    env.update(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--dry-run"], capture_output=True, text=True,
                       timeout=120, env=env, cwd=ROOT)
    assert r.returncode != 0
    assert "refusing" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def _fake_last(P, H, W):
    import torch
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)
    return dict(color=r(3, H, W), depth=r(1, H, W), radii=torch.arange(P, dtype=torch.int32), loss=r(()),
                grads=(r(P, 3), r(P, 3), r(P, 1), r(P, 3), r(P, 6), r(P, 16, 3), r(P, 3), r(P, 4)))


def test_dump_outputs_writes_float32_arrays_within_the_cap(tmp_path, monkeypatch):
    """--dump-outputs: every returned array as float32 <name>.npy; whole when they fit the cap, else the same
    seeded sample of each in every run, and never more than the cap in all."""
    import numpy as np
    import bench
    names = {"color", "depth", "radii", "loss", "dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dsh", "dL_dscales",
             "dL_drotations"}
    last = _fake_last(50, 6, 8)
    bench.dump_outputs(str(tmp_path / "whole"), last)
    got = {f[:-4]: np.load(tmp_path / "whole" / f) for f in os.listdir(tmp_path / "whole")}
    assert set(got) == names and all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["color"], last["color"].numpy()) and got["dL_dsh"].shape == (50, 16, 3)
    assert np.array_equal(got["radii"], np.arange(50, dtype=np.float32)) and got["loss"].shape == (1,)

    cap = 64 * 1024
    monkeypatch.setattr(bench, "DUMP_BYTES", cap)
    last = _fake_last(2000, 30, 40)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), last)
    files = sorted(os.listdir(tmp_path / "a"))
    assert {f[:-4] for f in files} == names
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= cap
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and a.size >= 1 and np.array_equal(a, b)
    sh = np.load(tmp_path / "a" / "dL_dsh.npy")
    assert sh.ndim == 1 and sh.size < 2000 * 48 and np.isin(sh, last["grads"][5].numpy().reshape(-1)).all()


def test_plain_run_has_no_extra_legs():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
