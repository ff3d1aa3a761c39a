#!/usr/bin/env python3
"""What an attached order schedule costs per env step (needs the GPU).

    python tools/order_schedule_cost.py [--parent-root DIR] [--alt-root DIR] [--out profiles/order_schedule/cost.txt]

Info-less stepping (with_info=False, auto_reset, one launch chain) at 4096 x 4 and 2048 x 8 with
    none    nothing attached (the host path's one null check)
    empty   a schedule attached whose windows are all empty (the launch, sched_of / header / offsets reads, no record load)
    one     one limit order per market and step
    A       one limit order per agent slot, market and step
--alt-root: this tree with its library built with -DCDA_SCHED_LOADS_FIRST (csrc/cda_schedule.inc: the record's loads issued ahead of the window's choice), every
variant timed beside this tree's.  --parent-root: a checkout of the parent commit with its library built; its `none` step time is measured in the same session, the trees in processes of their
own that alternate (parent, alt, this, parent, alt, this).  Each process warms every variant up, then times BLOCK steps per variant, the variants in turn, REPS times over, a host
clock around work that ends in a device synchronise; the table holds the median block and the spread (min .. max) in microseconds per step.  No threshold: the
numbers are written down."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((4096, 4), (2048, 8))
BLOCK, REPS, WARM, MAX_STEP = 256, 7, 64, 256


def child(n, a):
    sys.path.insert(0, os.environ.get("ORDER_SCHEDULE_COST_ROOT") or ROOT)
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd import _capi as K
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": MAX_STEP, "is_render": False, "auto_reset": True}, n_markets=n, with_info=False)
    acts = env.random_actions_device(0, 64, action_seed=11)
    has = hasattr(env, "set_order_schedule")
    quote = lambda slot, t: (slot, K.T_LIMIT, (t + slot) % 2, 1, 40 + (t % 5) if (t + slot) % 2 == 0 else 60 - (t % 5))      # noqa: E731 - a small resting quote
    schedules = {"none": None}
    if has:
        schedules.update(empty=[[[] for _ in range(MAX_STEP)]], one=[[[quote(a - 1, t)] for t in range(MAX_STEP)]],
                         A=[[[quote(s, t) for s in range(a)] for t in range(MAX_STEP)]])

    def run(steps, k0):
        for k in range(steps):
            j = (k0 + k) % 64
            env.step(acts[0][j], acts[1][j], acts[2][j], acts[3][j], acts[4][j])

    times = {v: [] for v in schedules}
    for rep in range(REPS + 1):                            # (the first round is the warm-up: every variant's kernels loaded, every shape seen)
        for v, rows in schedules.items():
            if has:
                env.clear_order_schedule() if rows is None else env.set_order_schedule(rows, market_schedule=[0] * n)
            env.reset(seed=77)
            run(WARM, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(BLOCK, WARM)
            torch.cuda.synchronize()
            if rep:
                times[v].append((time.perf_counter() - t0) / BLOCK * 1e6)
            assert int((env.flags() != 0).sum()) == 0 and int((env.check_invariants() != 0).sum()) == 0, v
    counts = env.order_schedule_counts().sum(0).tolist() if has and env.order_schedule else None
    print(json.dumps({"times_us": times, "last_counts": counts}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent-root", default=None)
    p.add_argument("--alt-root", default=None)
    p.add_argument("--out", default=None)
    p.add_argument("--child", nargs=2, type=int, default=None)
    args = p.parse_args()
    if args.child:
        return child(*args.child)
    lines = [f"order schedule cost: us per env step, info-less, auto_reset, max_step {MAX_STEP}; median of {REPS} blocks of {BLOCK} steps (min .. max); two processes per tree, alternating"]
    for n, a in SHAPES:
        libs = [(name, root) for name, root in (("parent", args.parent_root), ("alt", args.alt_root)) if root] + [("this", None)]
        got = {}
        for _round in range(2):
            for name, lib in libs:
                envv = dict(os.environ, ORDER_SCHEDULE_COST_ROOT=os.path.abspath(lib) if lib else "")
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(a)], env=envv, capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    sys.stderr.write(out.stdout + out.stderr)
                    raise SystemExit(f"the {name} run at {n} x {a} failed ({out.returncode})")
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                for v, ts in rec["times_us"].items():
                    got.setdefault((name, v), []).extend(ts)
                if rec["last_counts"]:
                    got[(name, "counts")] = rec["last_counts"]
        lines.append(f"{n} markets x {a} agents")
        base = statistics.median(got[("this", "none")])
        for (name, v), ts in got.items():
            if v == "counts":
                continue
            med = statistics.median(ts)
            lines.append(f"  {name:6s} {v:6s} {med:9.2f}  ({min(ts):.2f} .. {max(ts):.2f})   {med - base:+8.2f} us vs this/none")
        if ("this", "counts") in got:
            lines.append(f"  messages of the last A block: done, rejected, invalid, fills = {got[('this', 'counts')]}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
