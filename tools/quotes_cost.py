#!/usr/bin/env python3
"""What the quote tape costs per env step, and what its reductions cost per call (needs the GPU).

    python tools/quotes_cost.py [--parent-root DIR] [--out profiles/quotes/cost.txt]

Info-less stepping (with_info=False, auto_reset, one launch chain) at 4096 x 4 and 2048 x 8 with
    off          neither service on (the host path's one null check)
    tape         the trade tape alone (the yardstick the parent has too)
    quotes       the quote tape alone: k_quote_record ahead of every step
    quotes+tape  both
and, behind an episode of MAX_STEP steps with both services on, one call each of quote_stats, tape_spreads, tape_exec (same horizons) and drain_tape of the same
episode, a device synchronise behind each.  --parent-root: a checkout of the parent commit with its library built; its `off` and `tape` step times and its
tape_exec / drain_tape are measured in the same session, the trees in processes of their own that alternate (parent, this, this, parent).  Each process warms
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
BLOCK, REPS, WARM, MAX_STEP = 256, 7, 64, 256
HORIZONS = (1, 5, 20)


def child(n, a):
    sys.path.insert(0, os.environ.get("QUOTES_COST_ROOT") or ROOT)
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": MAX_STEP, "is_render": False, "auto_reset": True}, n_markets=n, with_info=False)
    acts = env.random_actions_device(0, 64, action_seed=11)
    has = hasattr(env, "enable_quotes")
    variants = ["off", "tape"] + (["quotes", "quotes+tape"] if has else [])

    def setting(v):
        if env.tape_enabled != ("tape" in v):
            env.enable_tape(4096) if "tape" in v else env.disable_tape()
        if has and env.quotes_enabled != ("quotes" in v):
            env.enable_quotes(2 * MAX_STEP) if "quotes" in v else env.disable_quotes()

    def run(steps, k0):
        for k in range(steps):
            j = (k0 + k) % 64
            env.step(acts[0][j], acts[1][j], acts[2][j], acts[3][j], acts[4][j])

    times = {v: [] for v in variants}
    for rep in range(REPS + 1):                            # (the first round is the warm-up: every variant's kernels loaded, every shape seen)
        for v in variants:
            setting(v)
            env.reset(seed=77)
            run(WARM, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(BLOCK, WARM)
            torch.cuda.synchronize()
            if rep:
                times[v].append((time.perf_counter() - t0) / BLOCK * 1e6)
            assert int((env.flags() != 0).sum()) == 0 and int((env.check_invariants() != 0).sum()) == 0, v
    # the reductions: one finished episode of MAX_STEP steps on the tape (and in the quotes)
    setting("quotes+tape" if has else "tape")
    env.reset(seed=77)
    run(MAX_STEP, 0)
    torch.cuda.synchronize()
    calls = {"tape_exec": lambda: env.tape_exec(HORIZONS, episode="previous"),
             "drain_tape": lambda: env.drain_tape(cursor=torch.zeros(n, dtype=torch.int64, device=env.device))}
    if has:
        calls.update(quote_stats=lambda: env.quote_stats(episode="previous"), tape_spreads=lambda: env.tape_spreads(HORIZONS, episode="previous"),
                     quote_series=lambda: env.quote_series(MAX_STEP, episode="previous"))
    for name, fn in calls.items():
        times[name] = []
        for rep in range(REPS + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append((time.perf_counter() - t0) * 1e6)
    fills = int(env.tape_exec(HORIZONS, episode="previous")[2][:, 0].sum())
    print(json.dumps({"times_us": times, "fills": fills}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent-root", default=None)
    p.add_argument("--out", default=None)
    p.add_argument("--child", nargs=2, type=int, default=None)
    args = p.parse_args()
    if args.child:
        return child(*args.child)
    lines = [f"quote tape cost: us per env step (info-less, auto_reset, max_step {MAX_STEP}) and us per reduction call over one finished episode, horizons {HORIZONS}; "
             f"median of {REPS} blocks of {BLOCK} steps / of {REPS} calls (min .. max); two processes per tree, alternating (parent, this, this, parent)"]
    for n, a in SHAPES:
        libs = ([("parent", args.parent_root)] if args.parent_root else []) + [("this", None)]
        got, fills = {}, None
        for _round in range(2):
            for name, lib in (libs if _round == 0 else libs[::-1]):      # (parent, this) then (this, parent): neither tree always runs first
                envv = dict(os.environ, QUOTES_COST_ROOT=os.path.abspath(lib) if lib else "")
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(a)], env=envv, capture_output=True, text=True, timeout=240)
                if out.returncode != 0:
                    sys.stderr.write(out.stdout + out.stderr)
                    raise SystemExit(f"the {name} run at {n} x {a} failed ({out.returncode})")
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                for v, ts in rec["times_us"].items():
                    got.setdefault((name, v), []).extend(ts)
                fills = rec["fills"]
        lines.append(f"{n} markets x {a} agents ({fills} fills in the episode)")
        base = statistics.median(got[("this", "off")])
        for (name, v), ts in got.items():
            med = statistics.median(ts)
            step = v in ("off", "tape", "quotes", "quotes+tape")
            lines.append(f"  {name:6s} {v:12s} {med:9.2f}  ({min(ts):.2f} .. {max(ts):.2f})" + (f"   {med - base:+8.2f} us vs this/off" if step else "   per call"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
