"""bench.py's multi-process line on the one-GPU box: the N > 1 code path run at world size 1 over RCCL
(--dist-path), so its collectives (all_gather of the per-rank times), the in-step rooflines, the weak-scaling
line and the strong-scaling cfg4 shard (ShardedStep into rank 0's shared pinned buffer, checked against one
GPU scoring the whole list) all run for real."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BENCH = os.path.join(ROOT, "bench.py")


def _run(*args, dist_path=True):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", *(["--dist-path"] if dist_path else []), *args],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_sharded_line_over_rccl_world1():
    """The N > 1 line at world 1: the sharded list (one shard = the whole list) through ShardedStep and its step
    fence, the RCCL gather variant, and every secondary shape, each checked against one GPU."""
    d = _run("--full", "--config", "cfg2", "--steps", "5", "--warmup", "1")
    assert d["full"] is True
    assert d["n_gpus"] == 1 and d["world_size"] == 1 and d["backend"] == "nccl" and d["scaling"] == "strong"
    assert d["matches_one_gpu"] is True and d["one_gpu_ms_per_step"] > 0 and d["value"] > 0
    assert d["config"]["pairs_per_rank"] == [d["config"]["pairs"]]
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1 and "traffic_source" in d["roofline"]
    assert d["in_step_kernels"] and d["step_roofline"]["frac"] > 0
    assert d["rccl_gather"]["matches_one_gpu"] is True and d["rccl_gather"]["backend"] == "nccl"
    assert d["weak_scaling"]["pairs_per_rank"] and d["weak_scaling"]["value"] > 0
    s = d["cfg4_strong"]
    assert s["matches_one_gpu"] is True and s["pairs"] > 30_000_000 and s["speedup_vs_one_gpu"] > 0
    sw = d["cfg5_sharded_band_sweep"]
    assert [p["band"] for p in sw["points"]] == [4, 8, 16, 32, 64, -1]
    assert all(p["matches_single_gpu"] is True for p in sw["points"])
    assert d["single_process_all_gpus"]["matches_single_gpu"] is True


@pytest.fixture(scope="module")
def cfg1_reference(oracle_mod):
    """cfg1's candidate list scored by the oracle (the same seeded reads bench.py builds)."""
    from ovlgraph.candidates import dedup_reads, enumerate_candidates
    from ovlgraph.reads import config_reads
    reads, _ = dedup_reads(config_reads("cfg1", seed=0))
    a, b = enumerate_candidates(reads, 5)
    return oracle_mod.batch_dp(reads, a, b)


@pytest.mark.parametrize("dist_path", [False, True], ids=["single", "dist"])
def test_plain_run_times_and_dumps_only(dist_path, cfg1_reference, tmp_path):
    """A run without --full: the headline fields, --steps timed steps, none of the secondary measurements, and
    --dump-outputs writes the last timed step's (score, end) -- here the whole cfg1 list, equal to the oracle's."""
    import numpy as np
    out = tmp_path / "dump"
    d = _run("--config", "cfg1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out), dist_path=dist_path)
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert (d["unit"], d["higher_is_better"], d["dtype"]) == ("overlap-pairs/s", True, "int32")
    pairs = d["config"]["pairs"]
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(pairs / (d["ms_per_step"] * 1e-3), rel=1e-9)
    moved = ("roofline", "in_step_kernels", "kernel_only_roofline", "cpu_baseline", "extra_configs", "end_to_end",
             "abi_one_shot", "cfg5_band_sweep", "one_gpu_ms_per_step", "rccl_gather", "weak_scaling", "cfg4_strong")
    assert all(d.get(k) is None for k in moved), [k for k in moved if d.get(k) is not None]
    info = d["dump_outputs"]
    assert info["pairs"] == info["pairs_written"] == pairs and info["sampled"] is False
    assert sorted(os.listdir(out)) == ["end.npy", "score.npy"]
    sc, en = np.load(out / "score.npy"), np.load(out / "end.npy")
    assert sc.dtype == en.dtype == np.float64 and sc.shape == en.shape == (pairs,)
    assert np.array_equal(sc, cfg1_reference[0]) and np.array_equal(en, cfg1_reference[1])
