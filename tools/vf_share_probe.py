"""Shared trunk (vf_share_layers) against separate networks, tanh: one FusedUpdate minibatch step of 65 536 rows (k_mlp_fb + k_mlp_wgrad + reduce + Adam, lr 0)
and the shared-policy rollout leg (RolloutChains, 4096 markets x 4 agents, horizon 64, graphs) - median wall time of N repetitions after warm-up, torch.cuda
events.  Prints one JSON line per network.  --update-only: the update steps alone (what a rocprofv3 --kernel-trace --stats run of this script attributes per kernel).

    python tools/vf_share_probe.py 20
    rocprofv3 --kernel-trace --stats -d OUT -o vfs -- python tools/vf_share_probe.py 20 --update-only
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main(reps=20, update_only=False):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    dev = "cuda:0"
    for vfs in (False, True):
        p = mlp.FusedPolicy(dev, seed=1, vf_share_layers=vfs)
        R, A = 65536, 4
        g = torch.Generator().manual_seed(2)
        x = (torch.randn(R, mlp.OBS, generator=g) * 0.5).to(dev)
        rec = torch.zeros(R, A, 8)
        rec[..., 0] = torch.randint(0, 9, (R, A), generator=g).int().view(torch.float32)
        rec[..., 1] = torch.randint(0, 10, (R, A), generator=g).int().view(torch.float32)
        rec[..., 2] = torch.randint(0, 3, (R, A), generator=g).int().view(torch.float32)
        rec[..., 3:5] = torch.randn(R, A, 2, generator=g)
        rec[..., 5] = -7.0
        rec[..., 6:8] = torch.randn(R, A, 2, generator=g)
        recd = rec.to(dev)
        upd = mlp.FusedUpdate(p, R, R, A)
        ts = []
        for i in range(reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            upd.minibatch_step(0, R, None, None, None, None, 0.2, 0.5, 0.01, 0.0, (0.9, 0.999), 1e-8, 0.5, records=(recd.data_ptr(), None, 0), obs_rows=x)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1))
        res = {"vf_share_layers": vfs, "wgrad_jobs": int(p.L.fn("cda_mlp_wgrad_jobs")()), "wgrad_chunks": upd.chunks, "update_step_65536_rows_ms": round(_median(ts), 4)}
        if not update_only:
            env = CDAVecEnv({"num_of_agents": 4, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}, n_markets=4096, with_info=False)
            env.reset(seed=0)
            roll = mlp.RolloutChains(env, p, 64, groups=4, seed=3)
            rs = []
            for i in range(max(4, reps // 4) + 2):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                roll.run()
                e1.record()
                torch.cuda.synchronize()
                if i >= 2:
                    rs.append(e0.elapsed_time(e1))
            env.close()
            res.update(rollout_4096x4_h64_ms=round(_median(rs), 3), rollout_ms_per_step=round(_median(rs) / 64, 4))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 20, "--update-only" in sys.argv)
