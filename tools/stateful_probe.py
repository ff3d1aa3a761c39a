#!/usr/bin/env python3
"""What the stateful opponents cost, and whether their memory shows in the stylised facts (CDAVecEnv.set_stateful, csrc/cda_stateful.inc
k_stateful_actions).

Cost: mlp.RolloutChains (a shared policy in slot 0, four chains, captured graphs, horizon 64, info-less steps) at 4096 markets x 4 agents and 2048 x 8:
  (a0) the PARENT tree (--head: its checkout, built), nothing attached;
  (a)  this tree, nothing attached: the chains launch what (a0) launches;
  (s)  this tree, the slots behind slot 0 played by k_script_actions (maker, taker, imbalance);
  (b)  this tree, the same placement played by k_stateful_actions (trend, value, execution).
They alternate in one call, --runs times each, the order rotated every round; every run is a fresh child process that measures both shapes: three warm-up rollouts
(the first captures), then --reps timed ones; host-clock time around the replays, ending in a device synchronise, over reps x horizon steps.

Stylised facts: one 1000-step episode of 256 markets x 8 agents, every slot rule-based, for two populations - slots cycling through maker, taker, trend, value and
through maker, taker only; the quote tape's return statistics pooled over the markets (stylised.returns_summary): excess kurtosis and the autocorrelation of |returns|.

    python tools/stateful_probe.py --head _ab_head --out profiles/stateful/cost.txt [--runs 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATELESS = ["maker", "taker", "imbalance"]
STATEFUL = ["trend", "value", "execution"]
SHAPES = [(4096, 4), (2048, 8)]
LAGS = (1, 2, 5, 10)


def child(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd import scripted as S
    T, out = args.horizon, {}
    for n, a in SHAPES:
        env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}, n_markets=n, device="cuda:0", with_info=False)
        env.reset(seed=1)
        slots = S.opponent_slots(n, a, 1, 3)
        if args.mode == "scripted":
            env.set_scripted(slots, STATELESS, seed=1)
        elif args.mode == "stateful":
            env.set_stateful(slots, STATEFUL, seed=1)
        chains = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=1), T, groups=4, seed=5, trained_slots=None if args.mode == "none" else 1)
        for _ in range(3):
            chains.run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            chains.run()
        torch.cuda.synchronize()
        out[f"{n}x{a}"] = {"us_per_step": 1e6 * (time.perf_counter() - t0) / (args.reps * T), "graphs": chains.graphs is not None, "launches_per_step": chains.launches_per_step,
                           "flagged_or_invalid_markets": int((env.flags() != 0).sum()) + int((env.check_invariants() != 0).sum())}
        env.close()
    print(json.dumps(out))


def stylised_child(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd import stylised as SF
    n, a, steps = 256, 8, 1000
    out = {}
    for name, cycle in (("maker, taker, trend, value", ["maker", "taker", "trend", "value"]), ("maker, taker", ["maker", "taker"])):
        env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": steps + 1, "is_render": False}, n_markets=n, device="cuda:0", with_info=False)
        env.reset(seed=11)
        env.enable_quotes(2048)
        m, j = np.meshgrid(np.arange(n), np.arange(a), indexing="ij")
        who = (m + j) % len(cycle)                               # slot j of market m plays cycle[(m + j) % len]
        for family, attach in ((STATELESS, env.set_scripted), (STATEFUL, env.set_stateful)):
            mine = [c for c in cycle if c in family]
            table = np.zeros((n, a), np.int32)
            for k, c in enumerate(mine):
                table[who == cycle.index(c)] = 1 + k
            if mine:
                attach(table, mine, seed=2)
        env.run_scripted(steps)
        torch.cuda.synchronize()
        base, lagged, hist, info = env.quote_returns(LAGS, 1, hist_half=16, episode="current")
        s = SF.returns_summary(SF.pool(base).cpu().numpy(), SF.pool(lagged).cpu().numpy(), SF.pool(hist).cpu().numpy(), LAGS)
        out[name] = {"returns": s["returns"], "variance": s["variance"], "excess_kurtosis": s["excess_kurtosis"], "clipped_share": s["clipped_share"],
                     "acf_abs": {k: v["acf_abs"] for k, v in s["lags"].items()}, "acf": {k: v["acf"] for k, v in s["lags"].items()},
                     "quotes_lost": int(info.cpu().numpy()[:, 1].sum()), "t_step": int(env.get_state(0).t_step),
                     "flagged_or_invalid_markets": int((env.flags() != 0).sum()) + int((env.check_invariants() != 0).sum())}
        env.close()
    print(json.dumps(out))


def run_one(tree, mode, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--mode", mode, "--horizon", str(args.horizon), "--reps", str(args.reps)]
    r = subprocess.run(["timeout", "-k", "10", str(args.timeout)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} exited {r.returncode}:\n{r.stderr[-2000:]}")       # (a faulted child ends the probe: nothing more is started)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", default=None, help="a built checkout of the parent tree (configuration (a0); skipped when absent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stateful", "cost.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40, help="timed rollouts per shape and run, after three warm-up rollouts")
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child run")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--mode", default="none", choices=["none", "scripted", "stateful", "stylised"])
    args = ap.parse_args()
    if args.child:
        return stylised_child(args) if args.mode == "stylised" else child(args)
    sides = ([("a0", os.path.abspath(args.head), "none")] if args.head else []) + [("a", ROOT, "none"), ("s", ROOT, "scripted"), ("b", ROOT, "stateful")]
    res = {s[0]: [] for s in sides}
    for i in range(args.runs):
        for name, tree, mode in sides[i % len(sides):] + sides[:i % len(sides)]:
            res[name].append(run_one(tree, mode, args))
            print(name, json.dumps(res[name][-1]), flush=True)
    facts = run_one(ROOT, "stylised", args)
    what = {"a0": "(a0) parent commit, nothing attached", "a": "(a) this commit, nothing attached", "s": f"(s) this commit, {', '.join(STATELESS)} behind slot 0 (k_script_actions)",
            "b": f"(b) this commit, {', '.join(STATEFUL)} behind slot 0 (k_stateful_actions)"}
    lines = [f"mlp.RolloutChains, one shared policy in slot 0, 4 chains, captured graphs, horizon {args.horizon}, info-less steps; {args.runs} runs each, alternating in one call,",
             f"each a fresh process: 3 warm-up rollouts + {args.reps} timed per shape; host-clock time ending in a device synchronise, per step.",
             f"    python tools/stateful_probe.py --head <built parent checkout> --runs {args.runs} --reps {args.reps}", ""]
    for n, a in SHAPES:
        key = f"{n}x{a}"
        lines.append(f"{n} markets x {a} agents")
        med = {}
        for name in res:
            r = [x[key]["us_per_step"] for x in res[name]]
            med[name] = statistics.median(r)
            lines.append(f"  {what[name]}: median {med[name]:.2f} us per step, spread {min(r):.2f} .. {max(r):.2f}; runs {', '.join(f'{v:.2f}' for v in r)}; launches per step "
                         f"{sorted({x[key]['launches_per_step'] for x in res[name]})}; graphs {all(x[key]['graphs'] for x in res[name])}; flagged or invalid markets "
                         f"{sum(x[key]['flagged_or_invalid_markets'] for x in res[name])}")
        if "a0" in res:
            lo, hi = min(x[key]["us_per_step"] for x in res["a0"]), max(x[key]["us_per_step"] for x in res["a0"])
            where = "yes" if lo <= med["a"] <= hi else ("NO, below it (faster)" if med["a"] < lo else "NO, above it (slower)")
            lines.append(f"  (a) median inside the spread of (a0): {where} ({med['a'] / med['a0'] - 1.0:+.2%} against (a0)'s median)")
        lines.append(f"  (b) against (s), the same placement: {med['b'] - med['s']:+.2f} us per step ({med['b'] / med['s'] - 1.0:+.2%}); against (a): (s) {med['s'] - med['a']:+.2f}, "
                     f"(b) {med['b'] - med['a']:+.2f} us per step (with opponents attached a chain's step is two launches plus the law's, and the books differ)")
        lines.append("")
    lines.append(f"Stylised facts of one 1000-step episode, 256 markets x 8 agents, every slot rule-based (named defaults), one-step bars, pooled over the markets; lags {list(LAGS)}")
    for name, f in facts.items():
        lines.append(f"  slots cycle through {name}: returns {f['returns']}, variance {f['variance']:.4f}, excess kurtosis {f['excess_kurtosis']:.3f} (clipped share "
                     f"{f['clipped_share']:.5f}); acf of |returns| " + ", ".join(f"{k} {v:+.4f}" for k, v in f["acf_abs"].items()) + "; acf of returns " +
                     ", ".join(f"{k} {v:+.4f}" for k, v in f["acf"].items()) + f"; quotes lost {f['quotes_lost']}; t_step {f['t_step']}; flagged or invalid markets "
                     f"{f['flagged_or_invalid_markets']}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
