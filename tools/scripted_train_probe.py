#!/usr/bin/env python3
"""What scripted opponents in the league's pool cost (league_train.train_league_fused(scripted_opponents=...)).

train_league_fused at 2048 markets x 8 agents, 2 trainable policies, horizon = episode = 64 (the shape of profiles/r06's league figure), three configurations:
  (a) the PARENT tree (--head: its checkout, built);
  (b) this tree with no scripted opponent - it launches the same kernels as (a);
  (c) this tree with three scripted opponents (maker, taker, imbalance) in the pool - one k_script_actions launch more per step.
The three alternate in one call, --runs times each, the order rotated every round; every run is a fresh child process that trains one warm-up iteration
(graph capture) and then --iters timed ones.  The rate is agent-steps over the iterations' host-clock time, each interval ending in a device synchronise
(the loop's own rollout_s + update_s).

    python tools/scripted_train_probe.py --head _ab_head --out profiles/scripted_train/cost.txt [--runs 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTED = ["maker", "taker", "imbalance"]


def child(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    env = CDAVecEnv({"num_of_agents": args.agents, "init_cash": 1000000, "max_step": args.episode, "is_render": False, "auto_reset": True}, n_markets=args.markets,
                    device="cuda:0", with_info=False)
    kw = dict(scripted_opponents=SCRIPTED) if args.scripted else {}
    _, _, hist = train_league_fused(env, iters=1 + args.iters, horizon=args.episode, num_trainable=2, log=lambda *_: None, **kw)
    torch.cuda.synchronize()
    tail = hist[1:]
    bad = int((env.flags() != 0).sum()) + int((env.check_invariants() != 0).sum())
    print(json.dumps({"rate": sum(h["agent_steps"] for h in tail) / sum(h["rollout_s"] + h["update_s"] for h in tail),
                      "rollout_us_per_step": 1e6 * sum(h["rollout_s"] for h in tail) / (len(tail) * args.episode),
                      "update_ms": 1e3 * sum(h["update_s"] for h in tail) / len(tail), "flagged_or_invalid_markets": bad}))
    env.close()


def run_one(tree, scripted, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--markets", str(args.markets), "--agents", str(args.agents), "--episode", str(args.episode),
           "--iters", str(args.iters)] + (["--scripted"] if scripted else [])
    r = subprocess.run(["timeout", "-k", "10", str(args.timeout)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} exited {r.returncode}:\n{r.stderr[-2000:]}")       # (a faulted child ends the probe: nothing more is started)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", default=None, help="a built checkout of the parent tree (configuration (a); skipped when absent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scripted_train", "cost.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4, help="timed iterations per run, after one warm-up iteration")
    ap.add_argument("--markets", type=int, default=2048)
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--episode", type=int, default=64)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child run")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--scripted", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    sides = ([("a", os.path.abspath(args.head), False)] if args.head else []) + [("b", ROOT, False), ("c", ROOT, True)]
    res = {s[0]: [] for s in sides}
    for i in range(args.runs):
        for name, tree, scripted in sides[i % len(sides):] + sides[:i % len(sides)]:
            res[name].append(run_one(tree, scripted, args))
            print(name, json.dumps(res[name][-1]), flush=True)
    what = {"a": "(a) parent commit", "b": "(b) this commit, no scripted opponent", "c": "(c) this commit, maker + taker + imbalance in the pool"}
    lines = [f"train_league_fused, {args.markets} markets x {args.agents} agents, 2 trainable policies, horizon = episode = {args.episode}; {args.runs} runs each, alternating in one call,",
             f"each a fresh process: 1 warm-up iteration + {args.iters} timed; agent-steps / host-clock seconds, every interval ending in a device synchronise.", ""]
    med = {}
    for name in res:
        r = [x["rate"] for x in res[name]]
        med[name] = statistics.median(r)
        lines.append(f"{what[name]}: median {med[name] / 1e6:.2f} M agent-steps/s, spread {min(r) / 1e6:.2f} .. {max(r) / 1e6:.2f} M; rollout "
                     f"{statistics.median(x['rollout_us_per_step'] for x in res[name]):.1f} us per step, update {statistics.median(x['update_ms'] for x in res[name]):.2f} ms; "
                     f"runs {', '.join(f'{v / 1e6:.2f}' for v in r)}; flagged or invalid markets {sum(x['flagged_or_invalid_markets'] for x in res[name])}")
    lines.append("")
    if "a" in res:
        lo, hi = min(x["rate"] for x in res["a"]), max(x["rate"] for x in res["a"])
        lines.append(f"(b) median inside the spread of (a): {'yes' if lo <= med['b'] <= hi else 'NO'} ({med['b'] / med['a'] - 1.0:+.2%} against (a)'s median)")
    rb, rc = (statistics.median(x["rollout_us_per_step"] for x in res[n]) for n in ("b", "c"))
    lines.append(f"(c) against (b): {med['c'] / med['b'] - 1.0:+.2%} end to end; rollout {rc:.1f} against {rb:.1f} us per step ({rc / rb - 1.0:+.2%}; the evaluation chain's "
                 "share for one k_script_actions launch per step was 74.0 against 71.5 us, +3.5 %)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
