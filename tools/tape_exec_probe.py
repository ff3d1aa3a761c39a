#!/usr/bin/env python3
"""What the tape's execution report costs: tape_exec at three horizons over a whole tape against drain_tape of the same tape - of this tree and, interleaved, of
another build of the project (the parent commit, checked out and built somewhere: --parent-tree DIR) - and against the host route a user had before it existed:
drain, copy to the host, tape.exec_from_records market by market.

    python tools/tape_exec_probe.py [--steps 1024] [--reps 5] [--capacity 4096] [--horizons 1,5,20] [--parent-tree DIR] [--out FILE]

Shapes: 4096 x 4 and 2048 x 8, info tensors on, one episode of `steps` steps of resident random actions.  Every repetition is a fresh process per tree (a process
binds one build of the library), alternating between the trees; inside it the tape is built once, every call is warmed once and then timed once (wall clock
around the call and a device synchronisation, allocations of the outputs included - as tools/tape_bars_probe.py times the bars)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def child(args):
    """one process, one tree: build the tape, time each reader once -> one JSON line"""
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a = args.shape
    hz = [int(k) for k in args.horizons.split(",")]
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": args.steps, "is_render": False}, n, with_info=True)
    env.enable_tape(args.capacity)
    acts = env.random_actions_device(0, args.steps, action_seed=9)
    env.reset(seed=123)
    for t in range(args.steps):
        env.step(*(x[t] for x in acts))
    torch.cuda.synchronize()
    zero = lambda: torch.zeros(n, dtype=torch.int64, device=env.device)      # noqa: E731

    def timed(fn, warm=True):
        if warm:
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    res = {"shape": [n, a], "root": args.root, "device": torch.cuda.get_device_name(0)}
    dt, (rows, off, dropped) = timed(lambda: env.drain_tape(cursor=zero()))
    res.update(drain_ms=dt * 1e3, records=int(rows.shape[0]), dropped=int(dropped.sum()))
    if hasattr(env, "tape_exec"):
        from gym_continuousdoubleauction_amd.tape import exec_from_records
        dt, (stats, marks, info) = timed(lambda: env.tape_exec(hz))
        res.update(exec_ms=dt * 1e3, out_bytes=int(stats.numel() * 8 + marks.numel() * 8), used=int(info[:, 0].sum()))
        dt, _ = timed(lambda: env.tape_flows())
        res.update(flows_ms=dt * 1e3)

        def host():
            r, o, _ = env.drain_tape(cursor=zero())
            r, o = r.cpu().numpy(), o.cpu().numpy()
            out = [exec_from_records(r[o[m]:o[m + 1]], a, hz) for m in range(n)]
            return np.stack([x[0] for x in out]), np.stack([x[1] for x in out])
        dt, (want_s, want_m) = timed(host, warm=False)                # (seconds of numpy: timed once, cold)
        scored, opened = int(marks[:, :, 0, 1, 2].sum()), int(marks[:, :, 0, 1, 3].sum())
        res.update(host_ms=dt * 1e3, equal_host=bool(np.array_equal(stats.cpu().numpy(), want_s) and np.array_equal(marks.cpu().numpy(), want_m)),
                   scored_share=scored / max(1, scored + opened))
    env.close()
    print("RESULT " + json.dumps(res))


def run_child(root, shape, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--shape", str(shape[0]), str(shape[1]), "--steps", str(args.steps),
           "--capacity", str(args.capacity), "--horizons", args.horizons]
    env = dict(os.environ)
    env.pop("CDA_HIP_LIB", None)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, env=env)
    if out.returncode != 0:
        raise SystemExit(f"child failed ({out.returncode}) for {root}:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")      # nothing more is started behind a failure
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def fmt(xs):
    return f"median {statistics.median(xs):9.3f} ms  (min {min(xs):.3f}, max {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--horizons", default="1,5,20")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--shape", type=int, nargs=2, default=None)
    ap.add_argument("--child-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []
    for shape in ((4096, 4), (2048, 8)):
        mine, theirs = [], []
        for _ in range(args.reps):
            mine.append(run_child(args.root, shape, args))
            if args.parent_tree:
                theirs.append(run_child(os.path.abspath(args.parent_tree), shape, args))
        m = mine[0]
        if not lines:
            lines.append(f"tape_exec_probe: one episode of {args.steps} steps, info tensors on, ring capacity {args.capacity}, horizons {args.horizons}; {args.reps} runs each, one "
                         f"process per run, the trees alternating; {m['device']}")
        lines += [f"{shape[0]} x {shape[1]}: {m['records']} records ({m['records'] * 32 / 1e6:.1f} MB of records, dropped {m['dropped']}); tables equal exec_from_records over the "
                  f"drained records: {all(x['equal_host'] for x in mine)}; non-self fills scored at the first horizon: {m['scored_share']:.3f}",
                  f"  drain_tape, this tree     : {fmt([x['drain_ms'] for x in mine])}"]
        base = statistics.median([x["drain_ms"] for x in mine])
        if theirs:
            assert all(x["records"] == m["records"] for x in theirs)
            base = statistics.median([x["drain_ms"] for x in theirs])
            lines.append(f"  drain_tape, parent commit : {fmt([x['drain_ms'] for x in theirs])}")
        for key, what in (("exec_ms", f"tape_exec ({m['out_bytes'] / 1e6:.1f} MB out)    "), ("flows_ms", "tape_flows, for scale        "),
                          ("host_ms", "drain + copy + numpy report ")):
            xs = [x[key] for x in mine]
            lines.append(f"  {what}: {fmt(xs)}   = {statistics.median(xs) / base:.2f} x the {'parent' if theirs else 'tree'}'s drain")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
