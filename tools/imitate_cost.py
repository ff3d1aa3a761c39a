#!/usr/bin/env python3
"""What behaviour cloning's kernels cost (profiles/imitate/cost.txt):

  (1) cda_bc_records for a 4096 x 4 x 64-step rollout;
  (2) cda_bc_loss_records against cda_ppo_loss_records at 65 536 rows x 4 (the rows gathered through a permutation, as the update does);
  (3) a whole BC minibatch step (imitate.BCUpdate) against the PPO step of mlp.FusedUpdate(fused=False) at the same shape.

Device events around batches of launches, after a warm-up; the two sides of a comparison alternate; median and spread of the repeated timed batches.

    python tools/imitate_cost.py [--repeats 15] [--batch 20]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def timed(fns, repeats, batch, warm=10):
    """fns: {name: callable}; alternating batches; returns {name: [us per call, ...]}"""
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / batch)
    return out


def line(name, xs, note=""):
    print(f"  {name:<58s} median {statistics.median(xs):9.2f} us   spread {min(xs):9.2f} .. {max(xs):9.2f}{note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    args = ap.parse_args()
    from gym_continuousdoubleauction_amd import imitate as IM, mlp
    from gym_continuousdoubleauction_amd._lib import check, lib
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1)
    print(f"{torch.cuda.get_device_name(0)}; device events around batches of {args.batch} launches, 10 warm-up launches, {args.repeats} timed batches each, the sides of a comparison alternating")

    # (1) the records of a 4096 x 4 x 64 rollout
    T, N, A = 64, 4096, 4
    ri = lambda n: torch.randint(0, n, (T, N, A), generator=g).int().to(DEV)     # noqa: E731
    cat, price, off = ri(9), ri(10), ri(3)
    mean, sigma = (torch.rand(T, N, A, generator=g) * 2 - 1).to(DEV), torch.rand(T, N, A, generator=g).to(DEV)
    a_cont = torch.randn(T, N, A, 2, generator=g).to(DEV)
    src = np.ones((N, A), np.int32)
    src[:, 0] = 0
    rec = torch.zeros(T, N, A, 8, device=DEV)
    src_d, w_d, stats = torch.from_numpy(src).to(DEV), torch.ones(N, A, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV)

    def records():
        check(L.cda_bc_records(cat.data_ptr(), price.data_ptr(), off.data_ptr(), mean.data_ptr(), sigma.data_ptr(), a_cont.data_ptr(), src_d.data_ptr(), w_d.data_ptr(),
                               T, N, A, rec.data_ptr(), stats.data_ptr(), st), "cda_bc_records")
    r = timed({"rec": records}, args.repeats, args.batch)
    moved = T * N * A * (5 * 4 + 24)
    print(f"\n(1) cda_bc_records, {N} markets x {A} agents x {T} steps = {T * N * A} samples ({moved / 1e6:.1f} MB read + written, a_cont not read: no policy-sample slot)")
    line("cda_bc_records", r["rec"], f"   {moved / statistics.median(r['rec']) / 1e6:.2f} TB/s")

    # (2) the two loss kernels at 65 536 rows x 4
    R = 65536
    out = torch.zeros(R, 32, device=DEV)
    out[:, :25] = torch.randn(R, 25, generator=g).to(DEV)
    ls = torch.tensor([-0.5, -0.5], device=DEV)
    lrec = rec.view(-1, A, 8)[:R].clone()
    lrec[..., 6:8] = torch.randn(R, A, 2, generator=g).to(DEV)
    prec = lrec.clone()
    prec[..., 5] = -7.0 + 0.1 * torch.randn(R, A, generator=g).to(DEV)
    perm = torch.randperm(R, generator=g).to(DEV)
    d_out, sums, out6 = torch.zeros(R, 32, device=DEV), torch.zeros(512, dtype=torch.float64, device=DEV), torch.zeros(8, device=DEV)
    logp, bstats = torch.zeros(R, A, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV)

    def ppo_loss():
        check(L.cda_ppo_loss_records(out.data_ptr(), ls.data_ptr(), prec.data_ptr(), None, 0, perm.data_ptr(), R, A, 32, 0.2, 0.5, 0.01, d_out.data_ptr(), sums.data_ptr(),
                                     out6.data_ptr(), 0, 0, 0, st), "cda_ppo_loss_records")

    def bc_loss(lp, bs):
        return lambda: check(L.cda_bc_loss_records(out.data_ptr(), ls.data_ptr(), lrec.data_ptr(), perm.data_ptr(), R, A, 32, 0.5, 0.01, 4.0 / 3.0, d_out.data_ptr(), sums.data_ptr(),
                                                   out6.data_ptr(), 0, 0, 0, lp, bs, st), "cda_bc_loss_records")
    r = timed({"ppo": ppo_loss, "bc": bc_loss(None, None), "bc_stats": bc_loss(None, bstats.data_ptr()), "bc_all": bc_loss(logp.data_ptr(), bstats.data_ptr())},
              args.repeats, args.batch)
    traffic = R * (8 + 25 * 4 + A * 32 + 32 * 4)
    print(f"\n(2) the loss kernels, {R} rows x {A} samples, rows gathered through a permutation, no clear / finish launch ({traffic / 1e6:.1f} MB: index, outputs, records, d_out)")
    line("cda_ppo_loss_records", r["ppo"])
    line("cda_bc_loss_records (no logp_out, no bc_stats)", r["bc"])
    line("cda_bc_loss_records (bc_stats: what BCUpdate launches)", r["bc_stats"])
    line("cda_bc_loss_records (bc_stats + logp_out: evaluate)", r["bc_all"])

    # (3) the whole minibatch step, separate kernels
    x = (torch.randn(R, 168, generator=g) * 0.5).to(DEV)
    steps = {}
    for name in ("ppo", "bc"):
        p = mlp.FusedPolicy(DEV, seed=3)
        upd = mlp.FusedUpdate(p, R, R, A, fused=False) if name == "ppo" else IM.BCUpdate(p, R, R, A)
        upd.perm.copy_(perm)
        check(p.L.fn("cda_mlp_prep_rows")(x.data_ptr(), upd.perm.data_ptr(), R, upd.x_rm.data_ptr(), upd.x_pk.data_ptr(), st), "cda_mlp_prep_rows")
        if name == "bc":
            upd.loss_scale = 4.0 / 3.0
        records_ = (prec if name == "ppo" else lrec, None, 0)
        steps[name] = (lambda u, rr: lambda: u.minibatch_step(0, R, None, None, None, None, 0.2, 0.5, 0.01, 1e-5, (0.9, 0.999), 1e-8, 0.5, records=rr))(upd, records_)
    r = timed(steps, args.repeats, max(1, args.batch // 4))
    print(f"\n(3) one minibatch step of the separate kernels (forward, loss, backward, weight gradients, Adam), {R} rows x {A} samples, host-launched, batches of {max(1, args.batch // 4)}")
    line("mlp.FusedUpdate(fused=False), cda_ppo_loss_records", r["ppo"])
    line("imitate.BCUpdate, cda_bc_loss_records", r["bc"])


if __name__ == "__main__":
    main()
