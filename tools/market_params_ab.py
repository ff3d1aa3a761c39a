#!/usr/bin/env python3
"""What per-market parameters cost (include/cda.h cda_market_params).

Two measurements on one GPU, in one process tree, alternating so that clock and thermal drift fall on both sides alike:
  1. the homogeneous path: the driver's command (bench.py --gpus 1 --steps K --warmup W) of a PARENT tree (--head: its checkout, built) and of this
     tree, alternating, --runs times each; the headline, policy-in-the-loop and league figures as medians with their min .. max;
  2. a heterogeneous env against the homogeneous one: 4096 markets x 4 agents stepped with every info tensor (the headline's leg: two group chains,
     device-resident random actions), once with eight per-market configs laid out round robin and once with the base config only, alternating.

    python tools/market_params_ab.py --head _ab_head --out profiles/market_params [--runs 5]

Writes <out>/bench_ab.json, <out>/hetero_ab.json and prints a summary."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("value", "value_policy_in_loop", "value_league_self_play")

CONFIGS = [{}, {"tick_size": 2}, {"tick_size": 5, "initial_price_min": 500, "initial_price_max": 800}, {"init_cash": 3000},
           {"init_cash": 50000000000, "mkt_max_size": 3000, "limit_size_multiple": 7}, {"order_penalty": 0.01, "trade_penalty": 0.3, "passive_bonus": 0.5},
           {"min_size": 3, "mkt_max_size": 20, "limit_size_multiple": 3}, {"drawdown_penalty": 0.9, "loss_multiplier": 2.5, "initial_price_min": 1, "initial_price_max": 30}]


def _bench(tree, steps, warmup, timeout):
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline"]
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, cwd=tree, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} exited {r.returncode}:\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    return {k: d.get(k) for k in KEYS}


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def bench_ab(head, runs, steps, warmup, timeout):
    res = {"head": [], "this": []}
    for i in range(runs):
        for side, tree in (("head", head), ("this", ROOT)) if i % 2 == 0 else (("this", ROOT), ("head", head)):
            res[side].append(_bench(tree, steps, warmup, timeout))
            print(side, json.dumps(res[side][-1]), flush=True)
    out = {"command": f"bench.py --gpus 1 --steps {steps} --warmup {warmup} --no-cpu-baseline", "order": "alternating, the first side swapped every round"}
    for k in KEYS:
        h = [r[k] for r in res["head"] if r[k] is not None]
        t = [r[k] for r in res["this"] if r[k] is not None]
        if h and t:
            out[k] = {"head": _spread(h), "this": _spread(t), "this_vs_head_median": statistics.median(t) / statistics.median(h) - 1.0}
    return out


def hetero_ab(runs, steps, warmup, markets=4096, agents=4):
    import torch
    sys.path.insert(0, ROOT)
    from gym_continuousdoubleauction_amd import CDAVecEnv
    base = {"num_of_agents": agents, "max_step": 4096, "is_render": False}      # (the spill ring, sized from max_step, must admit every row's size scale)
    envs = {"homogeneous": CDAVecEnv(base, n_markets=markets, with_info=True, groups=2),
            "heterogeneous": CDAVecEnv(base, n_markets=markets, with_info=True, groups=2, market_configs=[CONFIGS[m % len(CONFIGS)] for m in range(markets)])}
    acts = envs["homogeneous"].random_actions_device(0, warmup + steps, action_seed=2024)
    for e in envs.values():
        e.reset(seed=7)
        for t in range(warmup):
            e.step(*[a[t] for a in acts])
        e.join()
    torch.cuda.synchronize()
    ms = {k: [] for k in envs}
    for i in range(runs):
        order = list(envs) if i % 2 == 0 else list(envs)[::-1]
        for k in order:
            e = envs[k]
            e.reset(seed=7 + i)
            for t in range(warmup):
                e.step(*[a[t] for a in acts])
            e.join()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(warmup, warmup + steps):
                e.step(*[a[t] for a in acts])
            e.join()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    flags = {k: int((e.flags() != 0).sum()) for k, e in envs.items()}
    out = {"workload": f"{markets} markets x {agents} agents, every info tensor, 2 group chains, device-resident random actions, {steps} timed steps after {warmup}",
           "configs": CONFIGS, "flagged_markets": flags}
    for k, v in ms.items():
        out[k] = {"ms_per_step": _spread(v), "agent_steps_per_s_median": markets * agents / (statistics.median(v) * 1e-3)}
    out["heterogeneous_vs_homogeneous_time"] = statistics.median(ms["heterogeneous"]) / statistics.median(ms["homogeneous"]) - 1.0
    for e in envs.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", default=None, help="a built checkout of the parent tree (skip the bench A/B when absent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "market_params"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per bench.py run")
    ap.add_argument("--hetero-steps", type=int, default=1000)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.head:
        ab = bench_ab(os.path.abspath(args.head), args.runs, args.steps, args.warmup, args.timeout)
        with open(os.path.join(args.out, "bench_ab.json"), "w") as fh:
            json.dump(ab, fh, indent=1)
        for k in KEYS:
            if k in ab:
                print(f"{k}: head {ab[k]['head']['median'] / 1e6:.1f} M [{ab[k]['head']['min'] / 1e6:.1f} .. {ab[k]['head']['max'] / 1e6:.1f}]  "
                      f"this {ab[k]['this']['median'] / 1e6:.1f} M [{ab[k]['this']['min'] / 1e6:.1f} .. {ab[k]['this']['max'] / 1e6:.1f}]  ({ab[k]['this_vs_head_median'] * 100:+.2f} %)")
    het = hetero_ab(args.runs, args.hetero_steps, 64)
    with open(os.path.join(args.out, "hetero_ab.json"), "w") as fh:
        json.dump(het, fh, indent=1)
    print(f"heterogeneous vs homogeneous: {het['heterogeneous_vs_homogeneous_time'] * 100:+.2f} % time per step "
          f"({het['homogeneous']['ms_per_step']['median']:.4f} vs {het['heterogeneous']['ms_per_step']['median']:.4f} ms); flagged {het['flagged_markets']}")


if __name__ == "__main__":
    main()
