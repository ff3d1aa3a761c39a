#!/usr/bin/env python3
"""What the book report's device reductions cost: book_counts / book_levels / book_impact / book_agents / book_orders on a played batch against two things the
project already had - the pack launch of env.snapshot() (cda_snapshot_pack: it reads the same tile and ring bytes and writes far more) and the host loop of
get_book() over all markets, which is what the readers replace.

    python tools/book_report_probe.py [--steps 1024] [--reps 5] [--levels 10] [--out FILE]

Shapes: 4096 x 4 and 2048 x 8 after `steps` steps of resident random actions.  Every repetition is a fresh process; inside it the batch is played once, every call
is warmed once and then timed once: the launches with device events around the C entry point alone (the output allocated beforehand), the Python methods and the
get_book loop with the wall clock around the call and a device synchronisation, allocations included."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 10, 100, 1000)


def child(args):
    """one process: play the batch, time every reader once -> one JSON line"""
    sys.path.insert(0, args.root)
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd._lib import check, lib
    n, a = args.shape
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 4 * args.steps, "is_render": False}, n, with_info=True)
    acts = env.random_actions_device(0, args.steps, action_seed=9)
    env.reset(seed=123)
    for t in range(args.steps):
        env.step(*(x[t] for x in acts))
    torch.cuda.synchronize()
    L, h, stream = lib(), env._h, torch.cuda.current_stream(env.device).cuda_stream

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def launch(fn):
        """device time of one C entry point (its launches), by events on the stream it is given"""
        check(fn(), "warm-up")
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(fn(), "timed call")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    res = {"shape": [n, a], "device": torch.cuda.get_device_name(0)}
    counts = env.book_counts()
    res.update(orders=int(counts[:, :, 0].sum()), deepest_side=int(counts[:, :, 0].max()), levels_max=int(counts[:, :, 1].max()))
    # the yardstick: the snapshot's pack launch on the same env
    off = torch.empty(n + 1, dtype=torch.int64, device=env.device)
    check(L.cda_snapshot_offsets(h, 0, n, off.data_ptr(), stream), "cda_snapshot_offsets")
    total = int(off[n].item())
    blob = torch.empty(total, dtype=torch.uint8, device=env.device)
    res.update(snapshot_pack_ms=launch(lambda: L.cda_snapshot_pack(h, 0, n, off.data_ptr(), blob.data_ptr(), total, stream)), snapshot_bytes=total)
    out32 = torch.empty((n, 2, 2), dtype=torch.int32, device=env.device)
    res["counts_ms"] = launch(lambda: L.cda_book_counts(h, 0, n, out32.data_ptr(), stream))
    lv = torch.empty((n, 2, args.levels, 3), dtype=torch.int64, device=env.device)
    res["levels_ms"] = launch(lambda: L.cda_book_levels(h, 0, n, args.levels, lv.data_ptr(), stream))
    q = (C.c_int64 * len(SIZES))(*SIZES)
    imp = torch.empty((n, 2, len(SIZES), 3), dtype=torch.int64, device=env.device)
    res["impact_ms"] = launch(lambda: L.cda_book_impact(h, 0, n, q, len(SIZES), imp.data_ptr(), stream))
    ag = torch.empty((n, 2, a, 6), dtype=torch.int64, device=env.device)
    res["agents_ms"] = launch(lambda: L.cda_book_agents(h, 0, n, ag.data_ptr(), stream))
    boff = torch.empty(2 * n + 1, dtype=torch.int64, device=env.device)
    res["offsets_ms"] = launch(lambda: L.cda_book_offsets(h, 0, n, boff.data_ptr(), stream))
    rows = torch.empty((max(res["orders"], 1), 5), dtype=torch.int32, device=env.device)
    res["pack_ms"] = launch(lambda: L.cda_book_pack(h, 0, n, boff.data_ptr(), res["orders"], rows.data_ptr(), res["orders"], stream))
    # the Python methods, as a user calls them
    for name, fn in (("py_counts_ms", env.book_counts), ("py_levels_ms", lambda: env.book_levels(args.levels)), ("py_impact_ms", lambda: env.book_impact(SIZES)),
                     ("py_agents_ms", env.book_agents), ("py_orders_ms", env.book_orders), ("py_snapshot_ms", env.snapshot)):
        res[name] = wall(fn)[0]
    # what the readers replace: get_book for every market and side
    t0 = time.perf_counter()
    held = sum(len(env.get_book(i, s)) for i in range(n) for s in (0, 1))
    res.update(get_book_loop_ms=(time.perf_counter() - t0) * 1e3, get_book_orders=held)
    env.close()
    print("RESULT " + json.dumps(res))


def run_child(shape, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", args.root, "--shape", str(shape[0]), str(shape[1]), "--steps", str(args.steps), "--levels", str(args.levels)]
    env = dict(os.environ)
    env.pop("CDA_HIP_LIB", None)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, env=env)
    if out.returncode != 0:
        raise SystemExit(f"child failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")      # nothing more is started behind a failure
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def fmt(xs):
    return f"median {statistics.median(xs):8.3f} ms  (min {min(xs):.3f}, max {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--levels", type=int, default=10)
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
        runs = [run_child(shape, args) for _ in range(args.reps)]
        m = runs[0]
        if not lines:
            lines.append(f"book_report_probe: {args.steps} steps of random actions, info tensors on; ladder of {args.levels} levels, sizes {list(SIZES)}; {args.reps} runs, one process "
                         f"per run, every call warmed once; {m['device']}")
        assert all(x["orders"] == m["orders"] == x["get_book_orders"] for x in runs)
        base = statistics.median([x["snapshot_pack_ms"] for x in runs])
        lines += [f"{shape[0]} x {shape[1]}: {m['orders']} resting orders, deepest side {m['deepest_side']} orders / {m['levels_max']} levels; snapshot blob {m['snapshot_bytes'] / 1e6:.1f} MB",
                  f"  cda_snapshot_pack (yardstick) : {fmt([x['snapshot_pack_ms'] for x in runs])}"]
        for key, what in (("counts_ms", "cda_book_counts "), ("levels_ms", "cda_book_levels "), ("impact_ms", "cda_book_impact "), ("agents_ms", "cda_book_agents "),
                          ("offsets_ms", "cda_book_offsets"), ("pack_ms", "cda_book_pack   ")):
            xs = [x[key] for x in runs]
            lines.append(f"  {what}              : {fmt(xs)}   = {statistics.median(xs) / base:.2f} x the snapshot pack")
        for key, what in (("py_counts_ms", "book_counts()"), ("py_levels_ms", "book_levels()"), ("py_impact_ms", "book_impact()"), ("py_agents_ms", "book_agents()"),
                          ("py_orders_ms", "book_orders()"), ("py_snapshot_ms", "snapshot()   "), ("get_book_loop_ms", "get_book() x all markets x 2 sides")):
            lines.append(f"  {what:<30}: {fmt([x[key] for x in runs])}   (wall clock, call to synchronised)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
