#!/usr/bin/env python3
"""What the stylised-facts reductions cost (profiles/stylised/cost.txt): CDAVecEnv.quote_returns, tape_signs and tape_flow_returns with eight lags over one
finished 1000-step episode, at 4096 markets x 4 agents and 2048 x 8, each against

  (1) its one-pass neighbour on the same records, in the same process: quote_stats for quote_returns, tape_spreads (three horizons) for the two tape readers;
  (2) the host route a user has without them: quote_series / tape_last of 64 markets to the host and the numpy specification there, scaled to all markets.

Device events around batches of calls, after a warm-up; the sides of a comparison alternate; median and spread of the repeated timed batches.

    python tools/stylised_cost.py [--repeats 9] [--batch 10]
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
LAGS = (1, 2, 3, 5, 10, 20, 50, 100)                             # eight lags; 100 is beyond tape_signs' two-pass window of 64 fills
NEAR_LAGS = (1, 2, 3, 5, 10, 20, 50, 64)
FLOW_LAGS = (0, 1, 2, 3, 5, 10, 20, 50)


def line(name, xs, note=""):
    print(f"  {name:<44s} median {statistics.median(xs):9.2f} us   spread {min(xs):9.2f} .. {max(xs):9.2f}{note}")


def episode(n, a):
    """an env whose PREVIOUS episode is a whole 1000-step one of uniform random actions, both tapes on"""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": MAX_STEP, "is_render": False, "auto_reset": True}, n_markets=n, device="cuda:0", with_info=False)
    env.enable_tape(8192)
    env.enable_quotes(2048)
    env.reset(seed=np.arange(7000, 7000 + n, dtype=np.uint64))
    rng = np.random.default_rng(3)
    for _ in range(MAX_STEP + 8):
        env.step(rng.integers(0, 9, (n, a)).astype(np.int32), rng.uniform(-1, 1, (n, a)).astype(np.float32), rng.uniform(0, 1, (n, a)).astype(np.float32),
                 rng.integers(0, 10, (n, a)).astype(np.int32), rng.integers(0, 3, (n, a)).astype(np.int32))
    return env


def host_route(env):
    """seconds for HOST_MARKETS markets: the records to the host, then the specification in numpy, market by market"""
    from gym_continuousdoubleauction_amd import stylised as SF
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    qrec, qcnt, _ = (x.cpu().numpy() for x in env.quote_series(episode="previous", n_markets=HOST_MARKETS))
    trec, tcnt = (x.cpu().numpy() for x in env.tape_last(env.tape_capacity, n_markets=HOST_MARKETS, episode="previous"))
    t1 = time.perf_counter()
    for m in range(HOST_MARKETS):
        SF.returns_from_quotes(qrec[m, :qcnt[m]], LAGS, 1, 16)
    t2 = time.perf_counter()
    for m in range(HOST_MARKETS):
        SF.signs_from_records(trec[m, :tcnt[m]], LAGS)
    t3 = time.perf_counter()
    for m in range(HOST_MARKETS):
        SF.flow_returns_from_records(trec[m, :tcnt[m]], qrec[m, :qcnt[m]], FLOW_LAGS, 1)
    t4 = time.perf_counter()
    return {"copy": t1 - t0, "returns": t2 - t1, "signs": t3 - t2, "flow_returns": t4 - t3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    args = ap.parse_args()
    print(f"{torch.cuda.get_device_name(0)}; us per call over one finished episode of {MAX_STEP} steps (episode='previous'), eight lags; device events around batches of "
          f"{args.batch} calls, 10 warm-up calls, {args.repeats} timed batches each, the sides alternating")
    for n, a in ((4096, 4), (2048, 8)):
        env = episode(n, a)
        info = env.tape_flow_returns(FLOW_LAGS, 1, episode="previous")[2].cpu().numpy()
        print(f"{n} markets x {a} agents: {int(info[:, 0].sum())} fills and {n * MAX_STEP} quotes in the episode, {int(info[:, 1].sum())} fills and {int(info[:, 2].sum())} quotes lost")
        quote_side = timed({"quote_stats": lambda: env.quote_stats(episode="previous"),
                            "quote_returns": lambda: env.quote_returns(LAGS, 1, 16, episode="previous"),
                            "quote_returns bar_steps 5": lambda: env.quote_returns(LAGS, 5, 16, episode="previous"),
                            "quote_returns one lag": lambda: env.quote_returns((1,), 1, 16, episode="previous")}, args.repeats, args.batch)
        tape_side = timed({"tape_spreads (1, 5, 20)": lambda: env.tape_spreads((1, 5, 20), episode="previous"),
                           "tape_signs": lambda: env.tape_signs(LAGS, episode="previous"),
                           "tape_signs lags <= 64": lambda: env.tape_signs(NEAR_LAGS, episode="previous"),
                           "tape_signs one lag": lambda: env.tape_signs((1,), episode="previous"),
                           "tape_flow_returns": lambda: env.tape_flow_returns(FLOW_LAGS, 1, episode="previous"),
                           "tape_flow_returns one lag": lambda: env.tape_flow_returns((0,), 1, episode="previous")}, args.repeats, args.batch)
        base = statistics.median(quote_side["quote_stats"])
        for k, xs in quote_side.items():
            line(k, xs, "" if k == "quote_stats" else f"   {statistics.median(xs) / base:5.2f} x quote_stats")
        base = statistics.median(tape_side["tape_spreads (1, 5, 20)"])
        for k, xs in tape_side.items():
            line(k, xs, "" if k.startswith("tape_spreads") else f"   {statistics.median(xs) / base:5.2f} x tape_spreads")
        host_route(env)
        h = host_route(env)
        scale = n / HOST_MARKETS
        print(f"  host route, {HOST_MARKETS} markets timed and scaled x {scale:.0f}: copy {h['copy'] * scale * 1e3:8.1f} ms   returns {h['returns'] * scale * 1e3:8.1f} ms   "
              f"signs {h['signs'] * scale * 1e3:8.1f} ms   flow_returns {h['flow_returns'] * scale * 1e3:8.1f} ms")
        env.close()


if __name__ == "__main__":
    main()
