#!/usr/bin/env python3
"""What the order tape costs per env step, and what its readers cost per call (needs the GPU).

    python tools/order_tape_cost.py [--parent-root DIR] [--out profiles/order_tape/cost.txt]

Info-less stepping (with_info=False, auto_reset, one launch chain) at 4096 x 4 and 2048 x 8 with
    off          no service on (the host path's null checks)
    depth        the depth tape alone, levels 10: k_depth_record ahead of every step (the neighbour)
    orders       the order tape alone: k_order_record ahead of every step
and, behind an episode of 1000 steps with the trade tape, the depth tape and the order tape on, one call each of order_tape_series, order_flow, order_fills,
depth_series and tape_exec of that episode, a device synchronise behind each, and the host route for the same two tables: order_tape_series and the trade tape
of HOST_MARKETS markets copied to the host and the two numpy specifications over them (per market).  --parent-root: a checkout of the parent commit with its
library built; its off and depth step times are measured in the same session, the trees in processes of their own that alternate (parent, this, this, parent).
Each process warms every variant up, then times BLOCK steps per variant, the variants in turn, REPS times over, a host clock around work that ends in a device
synchronise; the table holds the median block and the spread (min .. max) in microseconds.  No threshold: the numbers are written down."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((4096, 4), (2048, 8))
BLOCK, REPS, WARM, MAX_STEP, LEVELS = 256, 7, 64, 256, 10
EPISODE, HOST_MARKETS, TAPE_CAP = 1000, 8, 8192
STEP_VARIANTS = ("off", "depth", "orders")


def child(n, a):
    sys.path.insert(0, os.environ.get("ORDER_TAPE_COST_ROOT") or ROOT)
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv

    def make(max_step):
        return CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}, n_markets=n, with_info=False)
    env = make(MAX_STEP)
    acts = env.random_actions_device(0, 64, action_seed=11)
    has = hasattr(env, "enable_order_tape")
    variants = [v for v in STEP_VARIANTS if has or v != "orders"]

    def setting(e, v):
        if e.depth_enabled != (v == "depth"):
            e.enable_depth(2 * MAX_STEP, LEVELS) if v == "depth" else e.disable_depth()
        if has and e.order_tape_enabled != (v == "orders"):
            e.enable_order_tape(2 * MAX_STEP) if v == "orders" else e.disable_order_tape()

    def run(e, steps, k0):
        for k in range(steps):
            j = (k0 + k) % 64
            e.step(acts[0][j], acts[1][j], acts[2][j], acts[3][j], acts[4][j])

    times = {v: [] for v in variants}
    for rep in range(REPS + 1):                            # (the first round is the warm-up: every variant's kernels loaded, every shape seen)
        for v in variants:
            setting(env, v)
            env.reset(seed=77)
            run(env, WARM, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(env, BLOCK, WARM)
            torch.cuda.synchronize()
            if rep:
                times[v].append((time.perf_counter() - t0) / BLOCK * 1e6)
            assert int((env.flags() != 0).sum()) == 0 and int((env.check_invariants() != 0).sum()) == 0, v
    env.close()
    records = 0
    if has:                                                # the readers: one finished episode of EPISODE steps in every ring
        from gym_continuousdoubleauction_amd import order_tape as OT
        env = make(EPISODE)
        env.enable_tape(TAPE_CAP); env.enable_depth(1024, LEVELS); env.enable_order_tape(1024)
        env.reset(seed=77)
        run(env, EPISODE + 1, 0)
        torch.cuda.synchronize()

        def host_route():
            rec, cnt, _ = (x.cpu().numpy() for x in env.order_tape_series(EPISODE, episode="previous", n_markets=HOST_MARKETS))
            rows, tcnt = (x.cpu().numpy() for x in env.tape_last(TAPE_CAP, n_markets=HOST_MARKETS, episode="previous"))
            for m in range(HOST_MARKETS):
                held = rec[m, :cnt[m]]
                OT.flow_from_records(held)
                OT.fills_from_records(rows[m, :tcnt[m]], held, a)
        calls = {"order_tape_series": lambda: env.order_tape_series(EPISODE, episode="previous"),
                 "order_flow": lambda: env.order_flow(episode="previous"),
                 "order_fills": lambda: env.order_fills(episode="previous"),
                 "depth_series": lambda: env.depth_series(EPISODE, episode="previous"),
                 "tape_exec": lambda: env.tape_exec((1, 5, 20), episode="previous"),
                 f"host route, {HOST_MARKETS} markets": host_route}
        for name, fn in calls.items():
            times[name] = []
            for rep in range((REPS if "host" not in name else 1) + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[name].append((time.perf_counter() - t0) * 1e6)
        flow, info = env.order_flow(episode="previous")
        records = int(info[:, 0].sum())
        assert records == n * EPISODE and int(info[:, 1].sum()) == 0 and int(flow[:, :, [0, 2]].sum()) == n * a * EPISODE      # (steps present + steps absent)
        env.close()
    print(json.dumps({"times_us": times, "records": records}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent-root", default=None)
    p.add_argument("--out", default=None)
    p.add_argument("--child", nargs=2, type=int, default=None)
    args = p.parse_args()
    if args.child:
        return child(*args.child)
    lines = [f"order tape cost: us per env step (info-less, auto_reset, max_step {MAX_STEP}; depth at levels {LEVELS}) and us per reader call over one finished episode of "
             f"{EPISODE} steps; median of {REPS} blocks of {BLOCK} steps / of {REPS} calls (min .. max); two processes per tree, alternating (parent, this, this, parent)"]
    for n, a in SHAPES:
        libs = ([("parent", args.parent_root)] if args.parent_root else []) + [("this", None)]
        got, records = {}, 0
        for _round in range(2):
            for name, lib in (libs if _round == 0 else libs[::-1]):      # (parent, this) then (this, parent): neither tree always runs first
                envv = dict(os.environ, ORDER_TAPE_COST_ROOT=os.path.abspath(lib) if lib else "")
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(a)], env=envv, capture_output=True, text=True, timeout=400)
                if out.returncode != 0:
                    sys.stderr.write(out.stdout + out.stderr)
                    raise SystemExit(f"the {name} run at {n} x {a} failed ({out.returncode})")
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                for v, ts in rec["times_us"].items():
                    got.setdefault((name, v), []).extend(ts)
                records = max(records, rec["records"])
        lines.append(f"{n} markets x {a} agents ({records} order records in the episode)")
        base = {name: statistics.median(got[(name, "off")]) for name, _ in libs}
        for (name, v), ts in got.items():
            med = statistics.median(ts)
            lines.append(f"  {name:6s} {v:24s} {med:11.2f}  ({min(ts):.2f} .. {max(ts):.2f})" +
                         (f"   {med - base[name]:+8.2f} us vs {name}/off" if v in STEP_VARIANTS else "   per call"))
        if args.parent_root:
            po, to = got[("parent", "off")], got[("this", "off")]
            lines.append(f"  off, this against the parent's own spread: parent {min(po):.2f} .. {max(po):.2f}, this {min(to):.2f} .. {max(to):.2f}, medians {statistics.median(to) - statistics.median(po):+.2f} us")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
