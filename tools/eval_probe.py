"""Greedy (evaluation) rollout rate against the sampled two-launch rollout, both on the fused network kernels: agent-steps/s of RolloutChains(greedy=True)
and of RolloutChains with CDA_POLICY_STEP=0 (the sampled network kernel + env step, no one-launch k_policy_step) at 4096 x 4 and 2048 x 8.

    python tools/eval_probe.py [--horizon 64] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rate(N, A, horizon, reps, greedy):
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    env = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}, n_markets=N, with_info=False)
    env.reset(seed=1)
    roll = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=0), horizon, seed=0, greedy=greedy)
    for _ in range(2):                                     # capture + one warm replay
        roll.run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        roll.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.close()
    return N * A * horizon * reps / dt


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--horizon", type=int, default=64)
    p.add_argument("--reps", type=int, default=10)
    args = p.parse_args()
    os.environ["CDA_POLICY_STEP"] = "0"                    # the sampled chain's two launches (greedy chains never take the one-launch step)
    out = []
    for N, A in ((4096, 4), (2048, 8)):
        g = rate(N, A, args.horizon, args.reps, True)
        s = rate(N, A, args.horizon, args.reps, False)
        out.append({"markets": N, "agents": A, "horizon": args.horizon, "greedy_agent_steps_per_s": g, "sampled_two_launch_agent_steps_per_s": s, "greedy_over_sampled": g / s})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
