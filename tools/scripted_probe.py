#!/usr/bin/env python3
"""What the scripted opponents cost: the launch of cda_scripted_actions (k_script_actions: both sides' walks and the laws in one wave per market) on a played
batch with every slot scripted, against the two book readers whose walks it does in one - cda_book_levels(10) + cda_book_agents on the same env, timed in this
tree and, with --parent-tree DIR, in another build of the project (the parent commit, checked out and built somewhere), the trees alternating - and a league
evaluation chain's step with slots 2 .. 7 scripted against the same chain with those slots on the uniform random stream.

    python tools/scripted_probe.py [--steps 1024] [--reps 5] [--horizon 32] [--parent-tree DIR] [--out FILE]

Launch shapes: 4096 x 4 and 2048 x 8 after `steps` steps of resident random actions; the chain: 4096 x 8.  Every repetition is a fresh process; inside it the
batch is played once, every call is warmed once and then timed once, with device events around the C entry point alone (the outputs allocated beforehand) or
around one RolloutChains.run() of `horizon` steps (the graphs captured and replayed once before)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CHAIN_SHAPE = (4096, 8)


def play(args, n, a, **cfg):
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv
    env = CDAVecEnv(dict({"num_of_agents": a, "init_cash": 1000000, "max_step": 4 * args.steps + 4 * args.horizon, "is_render": False}, **cfg), n, with_info=False)
    acts = env.random_actions_device(0, args.steps, action_seed=9)
    env.reset(seed=123)
    for t in range(args.steps):
        env.step(*(x[t] for x in acts))
    torch.cuda.synchronize()
    return env


def timed(fn):
    """device time of fn's launches on the current stream: warmed once, then one timed call between two events"""
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def mixed_profiles():
    """all four laws: the named defaults, a taker that trades every second step and a ten-level imbalance trader (the deepest ladder a profile may ask for)"""
    import dataclasses
    from gym_continuousdoubleauction_amd.scripted import NAMED
    return [NAMED["pass"], dataclasses.replace(NAMED["taker"], p_trade_q32=1 << 31), NAMED["maker"], dataclasses.replace(NAMED["maker"], max_orders=1, skew_position=0),
            NAMED["imbalance"], dataclasses.replace(NAMED["imbalance"], depth_levels=10, imb_num=3, imb_den=2)]


def mixed_slots(n, a, k):
    import numpy as np
    m, j = np.meshgrid(np.arange(n), np.arange(a), indexing="ij")
    return (1 + (m * 5 + j * 7 + m // 3) % k).astype(np.int32)


def child_launch(args):
    """one process: play the batch, time the two readers and (this tree only: --what launch) the scripted launch -> one JSON line"""
    import torch
    from gym_continuousdoubleauction_amd._lib import check, lib
    n, a = args.shape
    env = play(args, n, a)
    L, h, stream = lib(), env._h, torch.cuda.current_stream(env.device).cuda_stream
    counts = env.book_counts()
    res = {"shape": [n, a], "device": torch.cuda.get_device_name(0), "orders": int(counts[:, :, 0].sum()), "deepest_side": int(counts[:, :, 0].max())}
    lv = torch.empty((n, 2, 10, 3), dtype=torch.int64, device=env.device)
    ag = torch.empty((n, 2, a, 6), dtype=torch.int64, device=env.device)
    res["levels_ms"] = timed(lambda: check(L.cda_book_levels(h, 0, n, 10, lv.data_ptr(), stream), "cda_book_levels"))
    res["agents_ms"] = timed(lambda: check(L.cda_book_agents(h, 0, n, ag.data_ptr(), stream), "cda_book_agents"))
    if args.what == "launch":
        profiles = mixed_profiles()
        env.set_scripted(mixed_slots(n, a, len(profiles)), profiles, seed=7)
        out = env._action_buffers()
        out.update(a_cont=torch.zeros((n, a, 2), device=env.device), logp=torch.zeros((n, a), device=env.device), record=torch.zeros((n, a, 8), device=env.device))
        ptrs = [out[k].data_ptr() for k in ("category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp", "record")]
        res["scripted_ms"] = timed(lambda: check(L.cda_scripted_actions(h, 0, n, None, 0, *ptrs, stream), "cda_scripted_actions"))
        res["ordering"] = int((out["category"] != 0).sum())           # slots whose law sends an order on these books
    env.close()
    print("RESULT " + json.dumps(res))


def child_chain(args):
    """one process: a league evaluation chain (greedy; slot 0 and 1 two networks, slots 2 .. 7 the random module - or, --what chain_scripted, scripted)"""
    import numpy as np
    import torch
    from gym_continuousdoubleauction_amd import mlp
    n, a = args.shape
    env = play(args, n, a, auto_reset=True)
    bank = mlp.PolicyBank("cuda:0", n, a, n_trainable=1, max_frozen=1, random_seed=13)
    first, other = mlp.FusedPolicy("cuda:0", seed=1), mlp.FusedPolicy("cuda:0", seed=2)
    bank.theta[0].copy_(first.theta); bank.wb[0].copy_(first.wb)
    bank.n_frozen += 1
    bank.theta[1].copy_(other.theta); bank.wb[1].copy_(other.wb)
    bank._refresh()
    slot_net = np.full((n, a), mlp.LEAGUE_RANDOM, np.int32)
    slot_net[:, 0], slot_net[:, 1] = 0, 1
    bank.set_slots(torch.from_numpy(slot_net))
    if args.what == "chain_scripted":
        profiles = mixed_profiles()
        slots = mixed_slots(n, a, len(profiles))
        slots[:, :2] = 0
        env.set_scripted(slots, profiles, seed=7)
    chains = mlp.RolloutChains(env, bank, args.horizon, groups=4, seed=5, greedy=True)
    chains.run()                                                         # (captures the graphs and runs them once; timed() replays once more before it times)
    ms = timed(chains.run)
    flags = int((env.flags() != 0).sum())
    env.close()
    print("RESULT " + json.dumps({"shape": [n, a], "device": torch.cuda.get_device_name(0), "step_ms": ms / args.horizon, "graphs": chains.graphs is not None, "flagged": flags}))


def run_child(root, what, shape, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", what, "--root", root, "--shape", str(shape[0]), str(shape[1]), "--steps", str(args.steps),
           "--horizon", str(args.horizon)]
    env = dict(os.environ)
    env.pop("CDA_HIP_LIB", None)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, env=env)
    if out.returncode != 0:
        raise SystemExit(f"child failed ({out.returncode}) for {what} in {root}:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")      # nothing more is started behind a failure
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def fmt(xs):
    return f"median {statistics.median(xs):8.4f} ms  (min {min(xs):.4f}, max {max(xs):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--what", default="launch", choices=("launch", "readers", "chain_random", "chain_scripted"))
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--shape", type=int, nargs=2, default=None)
    ap.add_argument("--child-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, args.root)
        return child_chain(args) if args.what.startswith("chain") else child_launch(args)
    lines = []
    for shape in ((4096, 4), (2048, 8)):
        mine, theirs = [], []
        for _ in range(args.reps):
            mine.append(run_child(args.root, "launch", shape, args))
            if args.parent_tree:
                theirs.append(run_child(os.path.abspath(args.parent_tree), "readers", shape, args))
        m = mine[0]
        if not lines:
            lines.append(f"scripted_probe: {args.steps} steps of random actions, then every slot scripted (six profiles, all four laws); {args.reps} runs each, one process per "
                         f"run, every call warmed once, device time by events{', the trees alternating' if theirs else ''}; {m['device']}")
        assert all(x["orders"] == m["orders"] for x in mine + theirs)
        ref = theirs or mine
        both = [x["levels_ms"] + x["agents_ms"] for x in ref]
        base = statistics.median(both)
        whose = "parent commit" if theirs else "this tree"
        xs = [x["scripted_ms"] for x in mine]
        lines += [f"{shape[0]} x {shape[1]}: {m['orders']} resting orders, deepest side {m['deepest_side']}; {m['ordering']} of {shape[0] * shape[1]} slots send an order",
                  f"  cda_book_levels(10), {whose:<13}: {fmt([x['levels_ms'] for x in ref])}",
                  f"  cda_book_agents, {whose:<13}    : {fmt([x['agents_ms'] for x in ref])}",
                  f"  their sum (the yardstick)          : {fmt(both)}"]
        if theirs:
            lines.append(f"  the same sum, this tree            : {fmt([x['levels_ms'] + x['agents_ms'] for x in mine])}")
        lines.append(f"  cda_scripted_actions               : {fmt(xs)}   = {statistics.median(xs) / base:.2f} x the sum")
    if not args.no_chain:
        rnd, scr = [], []
        for _ in range(args.reps):
            rnd.append(run_child(args.root, "chain_random", CHAIN_SHAPE, args))
            scr.append(run_child(args.root, "chain_scripted", CHAIN_SHAPE, args))
        assert all(x["graphs"] and x["flagged"] == 0 for x in rnd + scr)
        a, b = statistics.median([x["step_ms"] for x in rnd]), statistics.median([x["step_ms"] for x in scr])
        lines += [f"league evaluation chain, {CHAIN_SHAPE[0]} x {CHAIN_SHAPE[1]}, 4 chains of captured graphs, one run() of {args.horizon} steps, per step (slots 0, 1 two networks):",
                  f"  slots 2 .. 7 the random module     : {fmt([x['step_ms'] for x in rnd])}",
                  f"  slots 2 .. 7 scripted              : {fmt([x['step_ms'] for x in scr])}   = {b / a:.2f} x, + {(b - a) * 1e3:.1f} us a step"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
