#!/usr/bin/env python3
"""What the depth tape costs per env step, and what its reductions cost per call (needs the GPU).

    python tools/depth_cost.py [--parent-root DIR] [--out profiles/depth/cost.txt]

Info-less stepping (with_info=False, auto_reset, one launch chain) at 4096 x 4 and 2048 x 8 with
    off          no service on (the host path's null checks)
    quotes       the quote tape alone: k_quote_record ahead of every step (the first yardstick)
    depth        the depth tape alone, levels 10: k_depth_record ahead of every step
    levels+sync  no service on, one book_levels(10) call and a device synchronise behind every step: the route the depth tape replaces (the second yardstick)
    levels       no service on, one book_levels(10) launch ahead of every step, no synchronise: what one cda_book_levels launch adds
and, behind an episode of 1000 steps with the quote tape, the trade tape and the depth tape on, one call each of depth_profile, depth_imbalance, depth_ofi,
quote_stats and tape_flow_returns of that episode, a device synchronise behind each, and the host route: depth_series of HOST_MARKETS markets copied to the host
and the three numpy specifications over them (per market).  --parent-root: a checkout of the parent commit with its library built; its off, quotes, levels+sync
and levels step times are measured in the same session, the trees in processes of their own that alternate (parent, this, this, parent).  Each process warms
every variant up, then times BLOCK steps per variant, the variants in turn, REPS times over, a host clock around work that ends in a device synchronise; the
table holds the median block and the spread (min .. max) in microseconds.  No threshold: the numbers are written down."""
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
EPISODE, HOST_MARKETS = 1000, 8
LAGS, OFI_LAGS, DEPTHS = (1, 2, 5, 10), (0, 1, 5), (1, 5, 10)
STEP_VARIANTS = ("off", "quotes", "depth", "levels+sync", "levels")


def child(n, a):
    sys.path.insert(0, os.environ.get("DEPTH_COST_ROOT") or ROOT)
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv

    def make(max_step):
        return CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}, n_markets=n, with_info=False)
    env = make(MAX_STEP)
    acts = env.random_actions_device(0, 64, action_seed=11)
    has = hasattr(env, "enable_depth")
    variants = [v for v in STEP_VARIANTS if has or v != "depth"]

    def setting(e, v):
        if e.quotes_enabled != (v == "quotes"):
            e.enable_quotes(2 * MAX_STEP) if v == "quotes" else e.disable_quotes()
        if has and e.depth_enabled != (v == "depth"):
            e.enable_depth(2 * MAX_STEP, LEVELS) if v == "depth" else e.disable_depth()

    def run(e, steps, k0, v=""):
        for k in range(steps):
            j = (k0 + k) % 64
            if v.startswith("levels"):
                e.book_levels(LEVELS)
                if v == "levels+sync":
                    torch.cuda.synchronize()
            e.step(acts[0][j], acts[1][j], acts[2][j], acts[3][j], acts[4][j])

    times = {v: [] for v in variants}
    for rep in range(REPS + 1):                            # (the first round is the warm-up: every variant's kernels loaded, every shape seen)
        for v in variants:
            setting(env, v)
            env.reset(seed=77)
            run(env, WARM, 0, v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(env, BLOCK, WARM, v)
            torch.cuda.synchronize()
            if rep:
                times[v].append((time.perf_counter() - t0) / BLOCK * 1e6)
            assert int((env.flags() != 0).sum()) == 0 and int((env.check_invariants() != 0).sum()) == 0, v
    env.close()
    records = 0
    if has:                                                # the reductions: one finished episode of EPISODE steps in every ring
        import numpy as np
        from gym_continuousdoubleauction_amd import depth as D
        env = make(EPISODE)
        env.enable_tape(4096); env.enable_quotes(EPISODE + 8); env.enable_depth(EPISODE + 8, LEVELS)
        env.reset(seed=77)
        run(env, EPISODE + 1, 0)
        torch.cuda.synchronize()

        def host_route():
            rec, cnt, info = (x.cpu().numpy() for x in env.depth_series(EPISODE, episode="previous", n_markets=HOST_MARKETS))
            for m in range(HOST_MARKETS):
                rows = rec[m, :cnt[m]]
                D.profile_from_records(rows, LEVELS, 32)
                D.imbalance_from_records(rows, LEVELS, LAGS, LEVELS, 8)
                D.ofi_from_records(rows, LEVELS, OFI_LAGS, 1, DEPTHS)
        calls = {"depth_profile": lambda: env.depth_profile(32, episode="previous"),
                 "depth_imbalance": lambda: env.depth_imbalance(LAGS, LEVELS, 8, episode="previous"),
                 "depth_ofi": lambda: env.depth_ofi(OFI_LAGS, 1, DEPTHS, episode="previous"),
                 "depth_series": lambda: env.depth_series(EPISODE, episode="previous"),
                 "quote_stats": lambda: env.quote_stats(episode="previous"),
                 "tape_flow_returns": lambda: env.tape_flow_returns(OFI_LAGS, 1, episode="previous"),
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
        records = int(env.depth_profile(32, episode="previous")[3][:, 0].sum())
        assert records == n * EPISODE and int(np.asarray(env.depth_series(1, episode="previous")[2].cpu())[:, 1].sum()) == 0
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
    lines = [f"depth tape cost: us per env step (info-less, auto_reset, max_step {MAX_STEP}, levels {LEVELS}) and us per reduction call over one finished episode of {EPISODE} steps "
             f"(lags {LAGS}, OFI lags {OFI_LAGS}, depths {DEPTHS}); median of {REPS} blocks of {BLOCK} steps / of {REPS} calls (min .. max); two processes per tree, "
             f"alternating (parent, this, this, parent)"]
    for n, a in SHAPES:
        libs = ([("parent", args.parent_root)] if args.parent_root else []) + [("this", None)]
        got, records = {}, 0
        for _round in range(2):
            for name, lib in (libs if _round == 0 else libs[::-1]):      # (parent, this) then (this, parent): neither tree always runs first
                envv = dict(os.environ, DEPTH_COST_ROOT=os.path.abspath(lib) if lib else "")
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(a)], env=envv, capture_output=True, text=True, timeout=400)
                if out.returncode != 0:
                    sys.stderr.write(out.stdout + out.stderr)
                    raise SystemExit(f"the {name} run at {n} x {a} failed ({out.returncode})")
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                for v, ts in rec["times_us"].items():
                    got.setdefault((name, v), []).extend(ts)
                records = max(records, rec["records"])
        lines.append(f"{n} markets x {a} agents ({records} depth records in the episode)")
        base = {name: statistics.median(got[(name, "off")]) for name, _ in libs}
        for (name, v), ts in got.items():
            med = statistics.median(ts)
            lines.append(f"  {name:6s} {v:24s} {med:11.2f}  ({min(ts):.2f} .. {max(ts):.2f})" +
                         (f"   {med - base[name]:+8.2f} us vs {name}/off" if v in STEP_VARIANTS else "   per call"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
