#!/usr/bin/env python3
"""What the tape's device reductions cost: tape_bars and tape_flows over a whole tape against drain_tape of the same tape - of this tree and, interleaved, of
another build of the project (the parent commit, checked out and built somewhere: --parent-tree DIR) - and against what a user did before they existed: drain,
copy to the host, reduce with numpy.

    python tools/tape_bars_probe.py [--steps 1024] [--reps 5] [--capacity 4096] [--bar-steps 16] [--parent-tree DIR] [--out FILE]

Shapes: 4096 x 4 and 2048 x 8, info tensors on, one episode of `steps` steps of resident random actions.  Every repetition is a fresh process per tree (a process
binds one build of the library), alternating between the trees; inside it the tape is built once, every call is warmed once and then timed once (wall clock
around the call and a device synchronisation, allocations of the outputs included - as tools/tape_probe.py times the drain)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def host_bars(rows, off, bar_steps, n_bars):
    """numpy over the drained records of all markets at once: the records are sorted by (market, step), so a bar is a run -> reduceat over the run starts"""
    import numpy as np
    r = rows.astype(np.int64)
    market = np.repeat(np.arange(len(off) - 1), np.diff(off))
    key = market * n_bars + (r[:, 7] >> 2) // bar_steps
    start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    end = np.r_[start[1:], len(key)] - 1
    out = np.zeros(((len(off) - 1) * n_bars, 9), np.int64)
    k = key[start]
    p, q = r[:, 1], r[:, 2]
    out[k, 0], out[k, 3] = p[start], p[end]
    out[k, 1], out[k, 2] = np.maximum.reduceat(p, start), np.minimum.reduceat(p, start)
    out[k, 4] = end - start + 1
    out[k, 5] = np.add.reduceat((r[:, 3] == r[:, 6]).astype(np.int64), start)
    out[k, 6] = np.add.reduceat(q, start)
    out[k, 7] = np.add.reduceat(np.where((r[:, 7] & 2) == 0, q, 0), start)
    out[k, 8] = np.add.reduceat(p * q, start)
    return out.reshape(len(off) - 1, n_bars, 9)


def child(args):
    """one process, one tree: build the tape, time each reader once -> one JSON line"""
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a = args.shape
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": args.steps, "is_render": False}, n, with_info=True)
    env.enable_tape(args.capacity)
    acts = env.random_actions_device(0, args.steps, action_seed=9)
    env.reset(seed=123)
    for t in range(args.steps):
        env.step(*(x[t] for x in acts))
    torch.cuda.synchronize()
    zero = lambda: torch.zeros(n, dtype=torch.int64, device=env.device)      # noqa: E731

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    res = {"shape": [n, a], "root": args.root, "device": torch.cuda.get_device_name(0)}
    dt, (rows, off, dropped) = timed(lambda: env.drain_tape(cursor=zero()))
    res.update(drain_ms=dt * 1e3, records=int(rows.shape[0]), dropped=int(dropped.sum()))
    if hasattr(env, "tape_bars"):
        n_bars = -(-args.steps // args.bar_steps)
        dt, (bars, info) = timed(lambda: env.tape_bars(args.bar_steps, n_bars))
        res.update(bars_ms=dt * 1e3, bars_bytes=int(bars.numel() * 4), used=int(info[:, 0].sum()))
        dt, (flows, _) = timed(lambda: env.tape_flows())
        res.update(flows_ms=dt * 1e3, flows_bytes=int(flows.numel() * 8))

        def host():
            r, o, _ = env.drain_tape(cursor=zero())
            return host_bars(r.cpu().numpy(), o.cpu().numpy(), args.bar_steps, n_bars)
        dt, want = timed(host)
        res.update(host_ms=dt * 1e3)
        w = bars.cpu().numpy()
        got = np.concatenate([w[..., :6].astype(np.int64), np.ascontiguousarray(w[..., 6:]).view(np.int64)], axis=-1)
        res.update(bars_equal_host=bool(np.array_equal(got, want)), flows_fills=int(flows[..., 2].sum()))
    env.close()
    print("RESULT " + json.dumps(res))


def run_child(root, shape, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--shape", str(shape[0]), str(shape[1]), "--steps", str(args.steps),
           "--capacity", str(args.capacity), "--bar-steps", str(args.bar_steps)]
    env = dict(os.environ)
    env.pop("CDA_HIP_LIB", None)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, env=env)
    if out.returncode != 0:
        raise SystemExit(f"child failed ({out.returncode}) for {root}:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")      # nothing more is started behind a failure
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def fmt(xs):
    return f"median {statistics.median(xs):7.3f} ms  (min {min(xs):.3f}, max {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--bar-steps", type=int, default=16)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--shape", type=int, nargs=2, default=None)
    ap.add_argument("--child-timeout", type=int, default=240)
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
            lines.append(f"tape_bars_probe: one episode of {args.steps} steps, info tensors on, ring capacity {args.capacity}, bars of {args.bar_steps} steps; {args.reps} runs each, one process per "
                         f"run, the trees alternating; {m['device']}")
        mb = m["records"] * 32 / 1e6
        lines += [f"{shape[0]} x {shape[1]}: {m['records']} records ({mb:.1f} MB of records, dropped {m['dropped']}); bars equal numpy over the drained records: {all(x['bars_equal_host'] for x in mine)}",
                  f"  drain_tape, this tree     : {fmt([x['drain_ms'] for x in mine])}"]
        base = statistics.median([x["drain_ms"] for x in mine])
        if theirs:
            assert all(x["records"] == m["records"] for x in theirs)
            base = statistics.median([x["drain_ms"] for x in theirs])
            lines.append(f"  drain_tape, parent commit : {fmt([x['drain_ms'] for x in theirs])}")
        for key, what in (("bars_ms", f"tape_bars ({m['bars_bytes'] / 1e6:.1f} MB out) "), ("flows_ms", f"tape_flows ({m['flows_bytes'] / 1e6:.1f} MB out)"),
                          ("host_ms", "drain + copy + numpy bars ")):
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
