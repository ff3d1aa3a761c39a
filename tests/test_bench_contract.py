"""GPU: bench.py prints ONE JSON line with the contract's fields (metric/value/..., roofline, cpu_baseline)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "40", "--warmup", "8", "--markets", "512",
                                   "--cpu-seconds", "0.5"], cwd=ROOT, stderr=subprocess.DEVNULL, text=True)
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 40 and d["warmup"] == 8 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["unit"] == "agent-steps/s" and d["value"] > 1e6
    assert abs(d["value"] - 512 * 4 * 40 / (d["ms_per_step"] * 1e-3 * 40)) / d["value"] < 1e-6
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert "traffic" in r and r["kernel"] == "k_step" and r["kernel_ms"] > 0
    # two concurrent group chains by default: `achieved` is the sum over the launches in flight
    assert d["config"]["groups"] == 2 and r["concurrent_launches"] == 2 and r["markets_per_launch"] == 256
    assert abs(r["achieved"] - 2 * r["achieved_per_launch"]) / r["achieved"] < 0.2
    assert abs(r["achieved_per_launch"] - r["algorithmic_bytes_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e9) / r["achieved_per_launch"] < 0.2
    assert "issue_frac" in r and "valu_busy_frac" in r
    # the HEADLINE has row a14 (every info tensor of Info_Helper.set_info) inside the timed region and says so;
    # the info-less figure, the one-launch figure and the ordered-per-step figure sit next to it
    assert d["config"]["info_outputs"] is True and "info tensor" in d["metric"] and "free-running" in d["metric"]
    assert d["value_without_info"] >= d["value"] * 0.9 and d["ms_per_step_without_info"] > 0
    assert d["value_one_launch"] > 0 and d["value_ordered_per_step"] > 0 and d["value_ordered_per_step"] <= d["value"] * 1.1
    assert d["config"]["flagged_markets"] == 0 and d["config"]["flagged_markets_without_info"] == 0
    # (ii): traffic / issue_frac come from a committed PMC pass of EXACTLY this shape or are null - 512 markets has none
    assert r["traffic"] is None and r["issue_frac"] is None and r["traffic_source"] is None
    # (iii): below 200 timed steps the K-step leg runs five times back to back; value is the median leg
    tr = d["timed_repeats"]
    assert tr["n"] == 5 and len(tr["ms_per_step"]) == 5 and tr["min"] <= tr["median"] <= tr["max"] and tr["median"] == d["ms_per_step"]
    assert "unbounded book" in d["config"]["workload"] and "HBM spill ring" in d["config"]["workload"]
    assert "cda_random_actions" in d["config"]["actions"]
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "agent-steps/s" and c["cores"] >= 1 and c["value"] > 0 and isinstance(c["sample"], str)
    assert c["value_1thread"] > 0 and isinstance(c["cpu_model"], str) and c["cpu_model"]
    assert "GPU leg's action stream" in c["sample"] and "hardware threads" in c["cores_note"] and "physical cores" in c["cores_note"]
    # the CPU leg builds the info tensors too (like the headline), says so, and carries the info-less and the
    # one-thread-per-physical-core figures next to the SMT one
    assert "info tensor" in c["outputs"] and c["value_without_info"] > 0 and "value_physical_cores" in c and "physical_cores" in c
    # ... the granted spill ring is in the config, with a flag when "unbounded inside an episode" was not affordable
    cf = d["config"]
    assert cf["book_tile"] == 256 and cf["book_spill"] >= 1024 and cf["book_spill_wanted"] >= cf["book_spill"] and cf["spill_halved"] == (cf["book_spill"] < cf["book_spill_wanted"])
    # the consumer-facing number - a policy network between the steps, per chain, no cross-stream edge inside the horizon
    assert d["value_policy_in_loop"] > 1e6 and d["ms_per_step_policy_in_loop"] > 0 and "MFMA" in cf["policy_in_loop"] and cf["flagged_markets_policy_in_loop"] == 0


def test_bench_traffic_only_from_a_pmc_pass_of_the_same_shape():
    """the committed PMC passes (profiles/pmc/) carry the shape they were taken on in their name and body; bench.py reports
    roofline.traffic for exactly that shape - here: the driver's command, 4096 x 4, info on, two chains"""
    import glob
    passes = sorted(glob.glob(os.path.join(ROOT, "profiles", "pmc", "*.json")))
    assert passes, "no PMC pass committed under profiles/pmc/"
    for f in passes:
        p = json.load(open(f))
        assert os.path.basename(f) == f"{p['markets']}x{p['agents']}_info{int(bool(p['info']))}_g{p['groups']}.json"
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                                   "--no-extra-legs"], cwd=ROOT, stderr=subprocess.DEVNULL, text=True, timeout=600)
    d = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][0])
    have = os.path.exists(os.path.join(ROOT, "profiles", "pmc", "4096x4_info1_g2.json"))
    assert (d["roofline"]["traffic"] is not None) == have
    if have:
        assert "4096x4_info1_g2" in d["roofline"]["traffic_source"] and 0 < d["roofline"]["issue_frac"] < 1


def test_bench_named_config_c4_and_single_group():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "24", "--warmup", "8", "--config", "c4", "--groups", "1",
                                   "--no-cpu-baseline", "--no-extra-legs"], cwd=ROOT, stderr=subprocess.DEVNULL, text=True, timeout=600)
    d = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][0])
    assert d["config"]["markets_per_gpu"] == 2048 and d["config"]["agents"] == 8 and "configs[3]" in d["config"]["workload"]
    assert d["config"]["groups"] == 1 and d["roofline"]["concurrent_launches"] == 1 and d["config"]["flagged_markets"] == 0
    assert d["roofline"]["algorithmic_bytes_per_launch"] == (1444 + 324 * 8) * 2048
    assert abs(d["value"] - 2048 * 8 * 24 / (d["ms_per_step"] * 1e-3 * 24)) / d["value"] < 1e-6


def test_bench_multi_gpu_code_path_on_one_rank():
    """The N>1 path of bench.py (RCCL process group, one communicator + all-gather of the hand-back records per group chain,
    the rebuild of the learner-side arrays) with a single rank - what the driver launches under torchrun at N>1."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29600 + os.getpid() % 300), RANK="0", LOCAL_RANK="0",
               WORLD_SIZE="1")
    for extra in ([], ["--groups", "1"]):
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "30", "--warmup", "5", "--markets",
                                       "512", "--no-cpu-baseline", "--force-gather"] + extra, cwd=ROOT, env=env,
                                      stderr=subprocess.STDOUT, text=True, timeout=600)
        lines = [ln for ln in out.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out[-2000:]
        d = json.loads(lines[0])
        assert d["n_gpus"] == 1 and d["value"] > 1e6 and "all-gathers per step" in d["config"]["collective"] and "208-B records" in d["config"]["collective"] and "ncclAllGather" in d["config"]["collective"]
        assert d["config"]["groups"] == (1 if extra else 2) and "hand-back" in d["metric"]
        assert d["config"]["flagged_markets"] == 0 and d["roofline"]["kernel_ms"] > 0
        # the native transport was checked against torch.distributed on synthetic records before anything was timed
        assert "self-check" in d["config"]["collective"] and "passed" in d["config"]["collective"]
    # (a): the transport can be forced, by flag and by environment; the line records what ran and what was asked for
    for how in (["--transport", "torch"], None):
        e2 = dict(env) if how else dict(env, CDA_BENCH_TRANSPORT="torch")
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "5", "--markets", "256", "--no-cpu-baseline",
                                       "--force-gather"] + (how or []), cwd=ROOT, env=e2, stderr=subprocess.STDOUT, text=True, timeout=600)
        d = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][0])
        assert "transport: torch.distributed" in d["config"]["collective"] and "asked: torch" in d["config"]["collective"] and d["config"]["flagged_markets"] == 0


def test_bench_fused_mode_reports_the_same_contract():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "64", "--warmup", "32", "--markets", "512",
                                   "--no-cpu-baseline", "--fused", "32"], cwd=ROOT, stderr=subprocess.DEVNULL, text=True, timeout=600)
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 64 and "FUSED" in d["config"]["workload"] and d["roofline"]["traffic"] is None and d["value"] > 1e6
    assert d["config"]["flagged_markets"] == 0
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "50", "--warmup", "32", "--markets", "64", "--no-cpu-baseline",
                          "--fused", "32"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "multiples" in (bad.stderr + bad.stdout)


def test_bench_two_ranks_on_one_gpu():
    """Two processes under torch.distributed.run, both pinned to GPU 0, gloo instead of RCCL: the multi-rank logic of bench.py
    (global-index seeds per rank, one communicator and one records all-gather per group chain sized by the world, the rebuild of the
    global arrays, max-over-ranks timing) runs for real; only the transport differs from the driver's 2-GPU launch."""
    env = dict(os.environ, CDA_BENCH_DEVICE="0", CDA_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(29700 + os.getpid() % 200), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "48",
                          "--warmup", "16", "--markets", "256", "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.stdout[-1500:], out.stderr[-1500:])
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 48 and "all-gathers per step" in d["config"]["collective"] and "torch.distributed" in d["config"]["collective"] and d["config"]["flagged_markets"] == 0
    assert "global 512 markets" in d["config"]["workload"] and d["timed_repeats"]["n"] == 5
    assert abs(d["value"] - 2 * 256 * 4 * 48 / (d["ms_per_step"] * 1e-3 * 48)) / d["value"] < 1e-6


def test_rccl_refuses_two_ranks_on_one_device():
    """Why the two-rank test above runs over gloo: RCCL (like NCCL) refuses a communicator with two ranks on one GPU, so the
    multi-rank RCCL path cannot execute on a one-GPU box.  This pins the refusal (and its text, quoted in DESIGN §5): if a
    future RCCL allows it, this test fails and the gloo stand-in should be replaced by the real transport."""
    env = dict(os.environ, CDA_BENCH_DEVICE="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "CDA_BENCH_BACKEND"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(29900 + os.getpid() % 90), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "8",
                          "--warmup", "4", "--markets", "64", "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode != 0
    assert "Duplicate GPU detected" in out.stderr, out.stderr[-1500:]


def _uneven_worker(rank, world, port, outdir, n_total):
    import numpy as np
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from gym_continuousdoubleauction_amd.parallel import ShardedVecEnv
    cfg = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 64, "is_render": False}
    sh = ShardedVecEnv(cfg, n_total, device="cuda:0", groups=2, handback=True)       # the HIP env, the HIP unpack kernel; gloo carries the records
    assert sh.transport == "torch" and sh.uneven and sh.n_env == n_total // world + n_total % world
    sh.reset(seed_base=1000)
    rec = []
    for t in range(10):
        rng = np.random.default_rng(700 + t)
        full = (rng.integers(0, 9, (n_total, 4)).astype(np.int32), rng.uniform(-1, 1, (n_total, 4)).astype(np.float32), rng.uniform(0, 1, (n_total, 4)).astype(np.float32),
                rng.integers(0, 10, (n_total, 4)).astype(np.int32), rng.integers(0, 3, (n_total, 4)).astype(np.int32))
        acts = [torch.from_numpy(x[sh.first:sh.first + sh.n_local]).cuda() for x in full]
        obs, rew, term, trunc, _ = sh.step(*acts)
        torch.cuda.synchronize()
        assert obs.shape[0] == sh.n_local
        rec.append((sh.full[0].cpu().numpy().copy(), sh.full[1].cpu().numpy().copy()))
    np.savez(os.path.join(outdir, f"uneven_{rank}.npz"), obs=np.stack([r[0] for r in rec]), rew=np.stack([r[1] for r in rec]))
    dist.barrier()
    sh.close()
    dist.destroy_process_group()


def test_uneven_shards_hand_back_on_the_hip_env_two_ranks_one_gpu(tmp_path):
    """13 markets over two ranks (6 + 7): every rank steps and sends seven records per step (the smaller shard padded with a market
    nobody reads), the HIP unpack kernel skips the padding; both ranks' learner-side arrays equal the oracle's single-process run, bit for bit."""
    import numpy as np
    import torch.multiprocessing as mp
    import oracle_lib as O
    n_total = 13
    mp.spawn(_uneven_worker, args=(2, 30100 + os.getpid() % 500, str(tmp_path), n_total), nprocs=2, join=True)
    ora = O.OracleEnv({"num_of_agents": 4, "init_cash": 1000000, "max_step": 64, "is_render": False}, n_total)
    ora.reset(seeds=(1000 + np.arange(n_total)).astype(np.uint64))
    got = [np.load(tmp_path / f"uneven_{r}.npz") for r in range(2)]
    for t in range(10):
        rng = np.random.default_rng(700 + t)
        full = (rng.integers(0, 9, (n_total, 4)).astype(np.int32), rng.uniform(-1, 1, (n_total, 4)).astype(np.float32), rng.uniform(0, 1, (n_total, 4)).astype(np.float32),
                rng.integers(0, 10, (n_total, 4)).astype(np.int32), rng.integers(0, 3, (n_total, 4)).astype(np.int32))
        oo, orw, _, _, _ = ora.step(*full)
        for r in range(2):
            assert np.array_equal(got[r]["obs"][t].view(np.uint32), oo.view(np.uint32)), (r, t)
            assert np.array_equal(got[r]["rew"][t].view(np.uint64), orw.view(np.uint64)), (r, t)
    ora.close()


@pytest.mark.gpu
def test_native_transport_probe_runs_in_a_sacrificial_child():
    """bench.py, N > 1: before the native RCCL hand-back (never run with more than one real rank) is trusted, every rank sends a child process through it and the ranks
    agree on the verdict; a hang costs the child, not the run.  One GPU: the child runs the real ncclAllGather on a one-rank communicator (passes); a child that is
    not given the time is killed and the verdict is torch.distributed."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    env_keep = {k: os.environ.pop(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT") if k in os.environ}
    try:
        ok, note = bench.probe_native_transport(None, 1, 0, 0, torch.device("cuda:0"), timeout_s=300.0)
        assert ok and "passed a sacrificial-child probe" in note, note
        ok, note = bench.probe_native_transport(None, 1, 0, 0, torch.device("cuda:0"), timeout_s=0.05)
        assert not ok and "did not finish" in note and "torch.distributed carries the records" in note, note
    finally:
        os.environ.update(env_keep)


def test_bench_dump_outputs_is_the_same_from_run_to_run(tmp_path):
    """--dump-outputs: the headline leg's last-step outputs (obs, reward, flags, every info tensor) as finite float32 / float64 .npy files under 64 MB; two runs
    with the same arguments write the same arrays, and so does a run that steps the batch as one launch instead of two group chains (markets never interact)."""
    import numpy as np
    runs = {"a": [], "b": [], "one_launch": ["--groups", "1"]}
    for name, extra in runs.items():
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "30", "--warmup", "6", "--markets", "512", "--no-cpu-baseline",
                                       "--no-extra-legs", "--dump-outputs", str(tmp_path / name)] + extra, cwd=ROOT, stderr=subprocess.DEVNULL, text=True, timeout=600)
        d = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][0])
        assert d["steps"] == 30 and d["ms_per_step"] > 0 and d["config"]["flagged_markets"] == 0
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert {"obs.npy", "reward.npy", "terminated.npy", "truncated.npy", "info_nav.npy", "info_reward_terms.npy"} <= set(files)
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 64 << 20
    obs = np.load(tmp_path / "a" / "obs.npy")
    assert obs.dtype == np.float32 and obs.shape[0] == 512 and np.load(tmp_path / "a" / "reward.npy").shape == (512, 4)
    assert np.abs(obs).sum() > 0 and all(np.isfinite(np.load(tmp_path / "a" / f)).all() for f in files)
    assert {"info_best_bid_present.npy", "info_best_ask_present.npy", "info_spread_present.npy"} <= set(files)      # (None, NaN in the env's tensors, as a mask)
    for other in ("b", "one_launch"):
        assert sorted(p.name for p in (tmp_path / other).iterdir()) == files
        for f in files:
            x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / other / f)
            assert x.dtype in (np.float32, np.float64) and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (other, f)
