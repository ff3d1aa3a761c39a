#!/usr/bin/env python3
"""What the trade tape costs: step time with the tape off and on (same build, same seeds, same resident random actions), fills per market-step, and the drain's
bandwidth.  Usage (on the GPU): python tools/tape_probe.py [--steps 1024] [--reps 5] [--out FILE]
Shapes: 4096 x 4 and 2048 x 8, info tensors on.  Off and on are measured INTERLEAVED, `reps` times each; medians and the spread are printed."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed_steps(env, acts, steps):
    env.reset(seed=123)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        env.step(*(a[t] for a in acts))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"tape_probe: {args.steps} steps per run, {args.reps} interleaved runs each, info tensors on, ring capacity {args.capacity}; {torch.cuda.get_device_name(0)}"]
    for n, a in ((4096, 4), (2048, 8)):
        cfg = {"num_of_agents": a, "init_cash": 1000000, "max_step": args.steps, "is_render": False}
        off, on = CDAVecEnv(cfg, n, with_info=True), CDAVecEnv(cfg, n, with_info=True)
        on.enable_tape(args.capacity)
        acts = off.random_actions_device(0, args.steps, action_seed=9)
        for e in (off, on):                                  # warm-up
            timed_steps(e, acts, 64)
        t_off, t_on = [], []
        for _ in range(args.reps):
            t_off.append(timed_steps(off, acts, args.steps))
            t_on.append(timed_steps(on, acts, args.steps))
        on.enable_tape(args.capacity)                        # fresh counters: one measured episode's fills
        timed_steps(on, acts, args.steps)
        fills = int(on.tape_counts()["n_total"].sum())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, offsets, dropped = on.drain_tape()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        mo, mn = statistics.median(t_off), statistics.median(t_on)
        lines += [f"{n} x {a}:",
                  f"  step, tape off: median {mo * 1e6:8.2f} us  (min {min(t_off) * 1e6:.2f}, max {max(t_off) * 1e6:.2f})   {n * a / mo / 1e6:7.1f} M agent-steps/s",
                  f"  step, tape on : median {mn * 1e6:8.2f} us  (min {min(t_on) * 1e6:.2f}, max {max(t_on) * 1e6:.2f})   {n * a / mn / 1e6:7.1f} M agent-steps/s",
                  f"  on / off: {mn / mo:.4f}  ({(mn / mo - 1) * 100:+.2f} %)",
                  f"  fills: {fills} in {args.steps} steps = {fills / (n * args.steps):.3f} per market-step = {32 * fills / (n * args.steps):.1f} B of records per market-step",
                  f"  drain: {rows.shape[0]} records ({rows.shape[0] * 32 / 1e6:.2f} MB, dropped {int(dropped.sum())}) in {dt * 1e3:.3f} ms = {rows.shape[0] * 32 / dt / 1e9:.2f} GB/s (two launches + one 8-byte read + the allocation)"]
        off.close(); on.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
