"""bench.py's multi-rank bookkeeping WITHOUT a GPU: `CDA_BENCH_DRY_RUN=1` runs everything of an N-rank run that is not device work - the
launcher's rendezvous (gloo), the barriers, the MAX-over-ranks reduction, the command line's shape logic - and prints the line through the SAME builders
(bench.headline_line / bench.learner_line) from fabricated timings, so that the first real multi-GPU run cannot fail on formatting.  Nothing here is a measurement."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = {"metric": str, "value": float, "unit": str, "n_gpus": int, "steps": int, "warmup": int, "ms_per_step": float, "higher_is_better": bool,
            "scaling": str, "dtype": str, "data": str, "config": dict}


def free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def run(world, *flags):
    env = dict(os.environ, CDA_BENCH_DRY_RUN="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    if world == 1:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *flags]
    else:                                                            # the driver's own launch line
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
               os.path.join(ROOT, "bench.py"), "--gpus", str(world), *flags]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout                                # ONE JSON line, from rank 0 only
    d = json.loads(lines[0])
    for k, t in CONTRACT.items():
        assert isinstance(d[k], t), (k, d[k])
    assert d["vs_baseline"] is None and d["higher_is_better"] is True and d["scaling"] == "weak" and d["unit"] == "agent-steps/s"
    assert d["n_gpus"] == world and "dry run" in d["data"]
    return d


def test_one_rank_line_has_the_contract_and_the_roofline_object():
    d = run(1, "--steps", "20", "--warmup", "5")
    assert d["steps"] == 20 and d["warmup"] == 5 and d["timed_repeats"]["n"] == 5 and d["config"]["collective"] == "none"
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert r["concurrent_launches"] == 2 and r["markets_per_launch"] == 2048 and r["algorithmic_bytes_per_launch"] == 2048 * (1444 + 4 * 324)
    assert "4096 markets x 4" in d["config"]["workload"] and "configs[2]" in d["config"]["workload"]


@pytest.mark.parametrize("transport", ["torch", "rccl"])
def test_two_ranks_hand_back_line(transport):
    d = run(2, "--steps", "20", "--warmup", "5", "--transport", transport)
    cf = d["config"]
    assert "2 all-gathers per step" in cf["collective"] and "208-B records" in cf["collective"] and f"asked: {transport}" in cf["collective"]
    assert ("ncclAllGather" if transport == "rccl" else "torch.distributed") in cf["collective"]
    assert "global 8192 markets" in cf["workload"] and cf["groups"] == 2 and d["roofline"]["kernel"] == "k_step"
    # value = the units ALL ranks processed / the slowest rank's time (rank 1 fabricates +1 %): 2 x 4096 x 4 x 20 / (20 x 40.4 us)
    assert abs(d["value"] - 2 * 4096 * 4 / 40.4e-6) / d["value"] < 1e-9 and abs(d["ms_per_step"] - 0.0404) < 1e-9


def test_two_ranks_data_parallel_learner_line():
    d = run(2, "--learner", "dp")
    assert d["steps"] == 8 and d["warmup"] == 2 and "all-reduce of the 0.9-MB gradient" in d["config"]["collective"] and "global 8192" in d["config"]["workload"]
    assert abs(d["value"] - 2 * 4096 * 4 * 64 / 7.07e-3) / d["value"] < 1e-9 and set(d["loss_last_iteration"]) == {"pg_loss", "v_loss", "entropy"}


def test_c4_shape_and_no_gather_flag():
    d = run(2, "--config", "c4", "--steps", "300", "--warmup", "10", "--no-gather")
    assert d["config"]["markets_per_gpu"] == 2048 and d["config"]["agents"] == 8 and d["config"]["collective"] == "none" and d["config"]["groups"] == 4
    assert d["timed_repeats"]["n"] == 1 and "configs[3]" in d["config"]["workload"]


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_under_the_cap(tmp_path):
    """--dump-outputs (no GPU: the writer on host tensors): float32 stays float32, integers / flags become exact float64, a dec28 array becomes the float64 of
    its exact value; above the cap every array keeps the same seeded sample of the markets, named by market_sample.npy, and the whole stays under the cap."""
    import decimal
    import numpy as np
    import torch
    from gym_continuousdoubleauction_amd import _capi as K
    bench = _bench_module()
    N, A = 1000, 4
    vals = [decimal.Decimal("1000000.123456789"), decimal.Decimal("-12.5"), decimal.Decimal("79228162514264337593543950335"), decimal.Decimal("0.000001")]
    nav = np.zeros((N, A, 16), np.uint8)
    for i in range(N):
        for a in range(A):
            nav[i, a] = np.frombuffer(bytes(K.decimal_to_dec(vals[(i + a) % 4])), np.uint8)
    g = torch.Generator().manual_seed(0)
    arrays = {"obs": torch.randn(N, 168, generator=g), "reward": torch.randn(N, A, dtype=torch.float64, generator=g),
              "terminated": (torch.arange(N) % 3 == 0).to(torch.uint8), "info_nav": torch.from_numpy(nav),
              "info_lob_actions": torch.randint(-5, 9, (N, A, 4), dtype=torch.int32, generator=g),
              "info_best_bid": torch.where(torch.arange(N) % 7 == 0, float("nan"), torch.arange(N, dtype=torch.float64))}
    bench.dump_outputs(str(tmp_path / "all"), arrays, {"info_nav"}, {"info_best_bid"})
    got = {n: np.load(tmp_path / "all" / f"{n}.npy") for n in arrays}
    assert not (tmp_path / "all" / "market_sample.npy").exists()
    assert got["obs"].dtype == np.float32 and np.array_equal(got["obs"], arrays["obs"].numpy())
    assert got["reward"].dtype == np.float64 and np.array_equal(got["reward"], arrays["reward"].numpy())
    assert got["terminated"].dtype == np.float64 and np.array_equal(got["terminated"], arrays["terminated"].numpy())
    assert got["info_lob_actions"].dtype == np.float64 and np.array_equal(got["info_lob_actions"], arrays["info_lob_actions"].numpy())
    assert got["info_nav"].shape == (N, A) and all(got["info_nav"][i, a] == float(vals[(i + a) % 4]) for i in range(4) for a in range(A))
    # NaN encodes None in the nullable fields: written as 0.0 next to a presence mask, so that every value on disk is finite
    present = np.load(tmp_path / "all" / "info_best_bid_present.npy")
    assert present.dtype == np.float64 and np.array_equal(present, (np.arange(N) % 7 != 0).astype(np.float64))
    assert np.array_equal(got["info_best_bid"], np.where(np.arange(N) % 7 == 0, 0.0, np.arange(N)))
    for f in (tmp_path / "all").iterdir():
        assert np.isfinite(np.load(f)).all(), f.name
    with pytest.raises(ValueError, match="non-finite"):
        bench.dump_outputs(str(tmp_path / "bad"), {"reward": torch.tensor([1.0, float("inf")], dtype=torch.float64)})
    bench.DUMP_MAX_BYTES = 256 << 10
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays, {"info_nav"}, {"info_best_bid"})
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= bench.DUMP_MAX_BYTES
    rows = np.load(tmp_path / "s1" / "market_sample.npy")
    assert rows.dtype == np.float64 and 0 < len(rows) < N and np.all(np.diff(rows) > 0)
    for n in list(arrays) + ["info_best_bid_present", "market_sample"]:
        assert np.array_equal(np.load(tmp_path / "s1" / f"{n}.npy"), np.load(tmp_path / "s2" / f"{n}.npy")), n
    for n in list(arrays) + ["info_best_bid_present"]:
        assert np.array_equal(np.load(tmp_path / "s1" / f"{n}.npy"), (got[n] if n in got else present)[rows.astype(np.int64)]), n
