#!/usr/bin/env python3
"""What the P&L report costs (profiles/pnl/cost.txt): CDAVecEnv.tape_pnl - the sixteen words alone, and with the three series - over one finished 1000-step
episode, at 4096 markets x 4 agents and 2048 x 8, against

  (1) the family's other tape readers on the same build, records and process: tape_exec, tape_spreads (three horizons) and tape_flow_returns (eight lags);
  (2) the host route a user has without it: tape_last and quote_series of 64 markets to the host and the numpy specification there, scaled to all markets.

Device events around batches of calls, after a warm-up; the sides alternate; median and spread of the repeated timed batches.  --step-cost times the env step
alone with both tapes on and the report never called (the line that is compared with the same run on the parent commit's build).

    python tools/pnl_cost.py [--repeats 9] [--batch 10] [--step-cost]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imitate_cost import timed  # noqa: E402

MAX_STEP, HOST_MARKETS = 1000, 64
FLOW_LAGS = (0, 1, 2, 3, 5, 10, 20, 50)


def line(name, xs, note=""):
    print(f"  {name:<44s} median {statistics.median(xs):9.2f} us   spread {min(xs):9.2f} .. {max(xs):9.2f}{note}")


def actions(rng, n, a):
    return (rng.integers(0, 9, (n, a)).astype(np.int32), rng.uniform(-1, 1, (n, a)).astype(np.float32), rng.uniform(0, 1, (n, a)).astype(np.float32),
            rng.integers(0, 10, (n, a)).astype(np.int32), rng.integers(0, 3, (n, a)).astype(np.int32))


def episode(n, a, steps=MAX_STEP + 8):
    """an env whose PREVIOUS episode is a whole 1000-step one of uniform random actions, both tapes on"""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": MAX_STEP, "is_render": False, "auto_reset": True}, n_markets=n, device="cuda:0", with_info=False)
    env.enable_tape(8192)
    env.enable_quotes(2048)
    env.reset(seed=np.arange(7000, 7000 + n, dtype=np.uint64))
    rng = np.random.default_rng(3)
    for _ in range(steps):
        env.step(*actions(rng, n, a))
    return env


def host_route(env):
    """seconds for HOST_MARKETS markets: the records to the host, then the specification in numpy, market by market"""
    from gym_continuousdoubleauction_amd import pnl as PN
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    qrec, qcnt, _ = (x.cpu().numpy() for x in env.quote_series(episode="previous", n_markets=HOST_MARKETS))
    trec, tcnt = (x.cpu().numpy() for x in env.tape_last(env.tape_capacity, n_markets=HOST_MARKETS, episode="previous"))
    t1 = time.perf_counter()
    for m in range(HOST_MARKETS):
        PN.pnl_from_records(trec[m, :tcnt[m]], qrec[m, :qcnt[m]], env.num_agents, 1)
    return {"copy": t1 - t0, "pnl": time.perf_counter() - t1}


def step_cost(repeats, batch):
    """us per env step at 4096 x 4 with both tapes on, the report never called: device events around batches of steps on prepared host actions"""
    n, a = 4096, 4
    env = episode(n, a, steps=64)
    rng = np.random.default_rng(5)
    acts = [actions(rng, n, a) for _ in range(batch)]
    state = {"i": 0}

    def step():
        env.step(*acts[state["i"] % batch])
        state["i"] += 1
    xs = timed({"step": step}, repeats, batch)["step"]
    line(f"env step, {n} x {a}, both tapes on", xs)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--step-cost", action="store_true")
    args = ap.parse_args()
    if args.step_cost:
        step_cost(args.repeats, 50)
        return
    print(f"{torch.cuda.get_device_name(0)}; us per call over one finished episode of {MAX_STEP} steps (episode='previous'), bar_steps 1; device events around batches of "
          f"{args.batch} calls, 10 warm-up calls, {args.repeats} timed batches each, the sides alternating")
    for n, a in ((4096, 4), (2048, 8)):
        env = episode(n, a)
        info = env.tape_pnl(1, "previous")[1].cpu().numpy()
        print(f"{n} markets x {a} agents: {int(info[:, 0].sum())} fills and {n * MAX_STEP} quotes in the episode, {int(info[:, 1].sum())} fills and {int(info[:, 2].sum())} quotes lost")
        side = timed({"tape_exec (1, 5, 20)": lambda: env.tape_exec((1, 5, 20), episode="previous"),
                      "tape_spreads (1, 5, 20)": lambda: env.tape_spreads((1, 5, 20), episode="previous"),
                      "tape_flow_returns, eight lags": lambda: env.tape_flow_returns(FLOW_LAGS, 1, episode="previous"),
                      "tape_pnl": lambda: env.tape_pnl(1, "previous"),
                      "tape_pnl with the three series": lambda: env.tape_pnl(1, "previous", series=True),
                      "tape_pnl bar_steps 5": lambda: env.tape_pnl(5, "previous")}, args.repeats, args.batch)
        base = statistics.median(side["tape_flow_returns, eight lags"])
        for k, xs in side.items():
            line(k, xs, f"   {statistics.median(xs) / base:5.2f} x tape_flow_returns" if k.startswith("tape_pnl") else "")
        host_route(env)
        h = host_route(env)
        scale = n / HOST_MARKETS
        print(f"  host route, {HOST_MARKETS} markets timed and scaled x {scale:.0f}: copy {h['copy'] * scale * 1e3:8.1f} ms   pnl_from_records {h['pnl'] * scale * 1e3:8.1f} ms")
        env.close()


if __name__ == "__main__":
    main()
