"""One launch per rollout step against two, per network: the shared-policy rollout leg (mlp.RolloutChains, horizon 64, graphs, 4 chains) of every hidden activation
with both trunks at 4096 x 4 and 2048 x 8, CDA_POLICY_STEP=1 (the one launch where advised: k_policy_step for tanh with its own value network, k_net_step for
every other network) against =0 (network kernel, then step kernel) - the SAME build, the same process, the two settings' rollouts ALTERNATING (each on its own env
and its own captured graphs), median and range of `reps` timed windows (8 rollouts) each after warm-up, device events.  Then the advised threshold: 16 384 x 4 with =2 (the one
launch wherever supported) against =0 for relu and the shared-trunk tanh network.  Prints one JSON line per (shape, network)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _chains(N, A, act, vfs, flag, horizon):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    os.environ["CDA_POLICY_STEP"] = flag                    # (read by the chains as they are enqueued: the captured graphs keep the path)
    env = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}, n_markets=N, with_info=False)
    env.reset(seed=0)
    roll = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=1, activation=act, vf_share_layers=vfs), horizon, groups=4, seed=3)
    for _ in range(3):                                      # capture + warm-up
        roll.run()
    torch.cuda.synchronize()
    return env, roll


def _time(roll, inner=8):
    """ms per rollout over a window of `inner` back-to-back rollouts"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        roll.run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def compare(N, A, act, vfs, one_flag, reps, horizon=64):
    pairs = [_chains(N, A, act, vfs, flag, horizon) for flag in (one_flag, "0")]
    paths = [r.launches_per_step for _, r in pairs]
    ts = ([], [])
    for _ in range(reps):
        for k, (_, r) in enumerate(pairs):
            ts[k].append(_time(r))
    for env, _ in pairs:
        env.close()
    row = {"markets": N, "agents": A, "activation": act, "vf_share_layers": vfs, "CDA_POLICY_STEP": one_flag, "launches_per_step": paths}
    for k, name in enumerate(("one_launch", "two_launches")):
        s = sorted(ts[k])
        row[name + "_ms_per_step"] = {"median": round(s[len(s) // 2] / horizon, 5), "min": round(s[0] / horizon, 5), "max": round(s[-1] / horizon, 5)}
    row["one_over_two"] = round(row["one_launch_ms_per_step"]["median"] / row["two_launches_ms_per_step"]["median"], 4)
    print(json.dumps(row), flush=True)


def shapes(reps=7):
    """which of the two the 2048 x 8 result follows, the market count or the agent count: the two shapes between, and a quarter of the resident round"""
    for N, A in ((2048, 4), (4096, 8), (1024, 4), (1024, 8)):
        for act, vfs in (("tanh", False), ("relu", False), ("tanh", True)):
            compare(N, A, act, vfs, "1", reps)


def main(reps=7):
    from gym_continuousdoubleauction_amd import mlp
    for N, A in ((4096, 4), (2048, 8)):
        for vfs in (False, True):
            for act in mlp.ACTIVATIONS:
                compare(N, A, act, vfs, "1", reps)
    for act, vfs in (("relu", False), ("tanh", True)):
        compare(16384, 4, act, vfs, "2", reps)


if __name__ == "__main__":
    (shapes if "--shapes" in sys.argv else main)(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 7)
