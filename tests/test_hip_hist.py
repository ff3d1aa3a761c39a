"""GPU: the network kernels at other history depths.  The reference trains with n_hist = 4 (168-float observations: the unsuffixed entry points);
the library also holds the same kernels compiled for n_hist 1, 2, 3, 6, 7 and 8 (include/cda_mlp.h CDA_MLP_HIST_VARIANTS: <name>_h<H>; mlp.layout(n_hist)) - 42 .. 336
inputs: other k-step counts of layer 1, 8-byte instead of 16-byte row requests for odd depths, another split of the dW1 panel over the weight-gradient jobs (two x-tile
groups at n_hist 8), one workgroup of the update kernel per CU at n_hist 8.  Same checks as tests/test_hip_mlp.py / test_hip_league.py, per depth.
This file walks the depth axis at tanh and a separate trunk; the cross product with the other activations and the shared trunk (56 objects) is walked, object by
object, in tests/test_hip_mlp_variants.py."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEPTHS = [1, 2, 3, 6, 7, 8]
ACTION_KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset")


def _policy(h, seed=3, scale=1.5):
    from gym_continuousdoubleauction_amd import mlp
    th = mlp.init_theta(42 * h, generator=torch.Generator().manual_seed(seed))
    th[:mlp.layout(h).OFF_LS] *= scale
    return mlp.FusedPolicy(DEV, theta=th)


def _obs(n, h, seed=5):
    x = torch.randn(n, 42 * h, generator=torch.Generator().manual_seed(seed)) * 1.5
    x[:, ::7] = 0.0
    return x


@pytest.mark.parametrize("h", DEPTHS)
def test_layout_constants_and_forward(h):
    from gym_continuousdoubleauction_amd import mlp
    L = mlp.layout(h)
    assert L.OBS == 42 * h and L.KX % 16 == 0 and L.KX >= L.OBS and L.KX - L.OBS < 16 and 32 * L.XT >= L.KX
    p = _policy(h)
    assert p.L is L and p.theta.numel() == L.PARAMS and p.wb.numel() == L.WB_ELEMS
    for n in (32, 200, 1031):
        x = _obs(n, h)
        out = p.forward(x.to(DEV)).cpu().double()
        ref = mlp.reference_outputs(p.theta, x)
        assert (out[:, :25] - ref[:, :25]).abs().max() <= 3e-3 * max(1.0, float(ref.abs().max())), (n, float((out[:, :25] - ref[:, :25]).abs().max()))
        assert (out[:, 25:] == 0).all()
    # the policy step: its value = the forward's, its actions in range, its log-probability that of its own actions
    N, A = 300, 4
    x = _obs(N, h, seed=31).to(DEV)
    counter = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    o = p.policy_step(x, A, seed=77, counter=counter, draw=3)
    torch.cuda.synchronize()
    out = p.forward(x).cpu()
    assert torch.equal(o["value"].cpu(), out[:, 24])
    cat, price, off, cont = o["category"].cpu().long(), o["price"].cpu().long(), o["price_offset"].cpu().long(), o["a_cont"].cpu()
    assert 0 <= cat.min() and cat.max() <= 8 and 0 <= price.min() and price.max() <= 9 and 0 <= off.min() and off.max() <= 2
    lg = out[:, :24].unsqueeze(1).expand(N, A, 24)
    ls = p.log_std.cpu()
    lp = (torch.log_softmax(lg[..., :9], -1).gather(-1, cat.unsqueeze(-1)).squeeze(-1) + torch.log_softmax(lg[..., 9:19], -1).gather(-1, price.unsqueeze(-1)).squeeze(-1)
          + torch.log_softmax(lg[..., 19:22], -1).gather(-1, off.unsqueeze(-1)).squeeze(-1))
    z = (cont - lg[..., 22:24]) * torch.exp(-ls)
    lp = lp + (-0.5 * z * z - ls - 0.5 * math.log(2 * math.pi)).sum(-1)
    assert (lp - o["logp"].cpu()).abs().max() <= 2e-4


def _grad_vector(m, L):
    gm = torch.zeros(L.PARAMS, dtype=torch.float64)
    H = 256
    gm[L.OFF_W1:L.OFF_B1] = m.l1.weight.grad.double().reshape(-1); gm[L.OFF_B1:L.OFF_W2] = m.l1.bias.grad.double()
    w2g = m.l2.weight.grad.double()
    gm[L.OFF_W2:L.OFF_B2] = torch.stack([w2g[:H, :H], w2g[H:, H:]]).reshape(-1); gm[L.OFF_B2:L.OFF_WO] = m.l2.bias.grad.double()
    wog = m.out.weight.grad.double(); blk = torch.zeros(32, H, dtype=torch.float64); blk[:24] = wog[:24, :H]; blk[24] = wog[24, H:]
    gm[L.OFF_WO:L.OFF_BO] = blk.reshape(-1)
    bog = m.out.bias.grad.double().clone(); bog[25:] = 0
    gm[L.OFF_BO:L.OFF_LS] = bog; gm[L.OFF_LS:] = m.log_std.grad.double()
    return gm


@pytest.mark.parametrize("h", DEPTHS)
def test_update_gradient_equals_float32_autograd(h):
    """the fused update (gather, forward, loss, back-propagation, weight gradients with this depth's job split, reduce) against loss.backward() through ppo.ActorCritic"""
    from gym_continuousdoubleauction_amd import mlp
    L = mlp.layout(h)
    R, A = 512, 4
    g = torch.Generator().manual_seed(6)
    p = mlp.FusedPolicy(DEV, theta=mlp.init_theta(L.OBS, generator=torch.Generator().manual_seed(13)))
    x = _obs(R, h, seed=17) * 0.5
    rec = torch.zeros(R, A, 8)
    rec[..., 0] = torch.randint(0, 9, (R, A), generator=g).int().view(torch.float32)
    rec[..., 1] = torch.randint(0, 10, (R, A), generator=g).int().view(torch.float32)
    rec[..., 2] = torch.randint(0, 3, (R, A), generator=g).int().view(torch.float32)
    rec[..., 3:5] = torch.randn(R, A, 2, generator=g)
    rec[..., 5] = torch.randn(R, A, generator=g) * 0.1 - 7.0
    rec[..., 6:8] = torch.randn(R, A, 2, generator=g)
    upd = mlp.FusedUpdate(p, R, R, A, chunks=4)
    upd.perm.copy_(torch.randperm(R, generator=g))
    recd, xd = rec.to(DEV), x.to(DEV)
    upd.minibatch_step(0, R, None, None, None, None, 0.2, 0.5, 0.01, 0.0, (0.9, 0.999), 1e-8, 0.5, records=(recd, None, 0), obs_rows=xd)
    torch.cuda.synchronize()
    grad = upd.grad.cpu().double()
    m = mlp.actor_critic_from_theta(p.theta).float()
    acts = (rec[..., 0].contiguous().view(torch.int32).long().reshape(-1), rec[..., 1].contiguous().view(torch.int32).long().reshape(-1),
            rec[..., 2].contiguous().view(torch.int32).long().reshape(-1), rec[..., 3:5].reshape(-1, 2))
    logp, ent, v = m.evaluate(x, acts, agents_per_row=A)
    ratio = (logp - rec[..., 5].reshape(-1)).exp()
    adv = rec[..., 6].reshape(-1)
    loss = -torch.min(ratio * adv, ratio.clamp(0.8, 1.2) * adv).mean() + 0.5 * (v - rec[..., 7].reshape(-1)).pow(2).mean() - 0.01 * ent.mean()
    loss.backward()
    gm = _grad_vector(m, L)
    # the weight-gradient kernel's job split and the reduction's dense -> parameter map at THIS depth, isolated: dW1 / dW2 recomputed in float64 from the kernel's own
    # packed operands (x as written by the update kernel, dz1, dz2, h1) must equal the gradient's blocks to float32 accumulation
    k1 = mlp.unpack_rows(upd.dz1p[:R * 512], R, 512, paired=True).double()
    k2 = mlp.unpack_rows(upd.dz2p[:R * 512], R, 512, paired=True).double()
    h1 = mlp.unpack_rows(upd.h1p[:R * 512], R, 512, paired=True).double()
    xb = mlp.unpack_rows(upd.x_pk_mb[:R * 32 * L.XT], R, 32 * L.XT)
    assert (xb[:, L.OBS:] == 0).all() and torch.equal(xb[:, :L.OBS], x[upd.perm.cpu()].to(torch.bfloat16).float())
    w1 = (k1.t() @ xb[:, :L.OBS].double()).reshape(-1)
    w2 = torch.stack([k2[:, :256].t() @ h1[:, :256], k2[:, 256:].t() @ h1[:, 256:]]).reshape(-1)
    for got, want, name in ((grad[L.OFF_W1:L.OFF_B1], w1, "W1"), (grad[L.OFF_W2:L.OFF_B2], w2, "W2"), (grad[L.OFF_B1:L.OFF_W2], k1.sum(0), "b1")):
        assert (got - want).abs().max() <= 1e-4 * want.abs().max() + 1e-12, (name, float((got - want).abs().max()), float(want.abs().max()))
    cos = float((grad * gm).sum() / (grad.norm() * gm.norm()))
    assert cos > 0.999, cos
    for lo, hi, name in ((L.OFF_W1, L.OFF_B1, "W1"), (L.OFF_B1, L.OFF_W2, "b1"), (L.OFF_W2, L.OFF_B2, "W2"), (L.OFF_B2, L.OFF_WO, "b2"), (L.OFF_WO, L.OFF_BO, "Wo"),
                         (L.OFF_BO, L.OFF_LS, "bo"), (L.OFF_LS, L.PARAMS, "log_std")):
        a, b = grad[lo:hi], gm[lo:hi]
        # bfloat16 operands against float32 autograd: the weight blocks are sums over 512 rows of products of two ROUNDED operands (2^-9 each) - measured up to
        # 4.1 % of the block's norm at these depths (n_hist 4: under 3 %, tests/test_hip_mlp.py); the exact statement of the same blocks is the check above
        assert (a - b).norm() <= 6e-2 * b.norm() + 1e-9, (name, float((a - b).norm() / b.norm()))
    assert abs(float(upd.out6[3]) - float(loss.detach())) <= 2e-2 * abs(float(loss.detach())) + 1e-3


@pytest.mark.parametrize("h", DEPTHS)
def test_rollout_replays_through_the_oracle_and_the_two_update_paths_agree(h):
    """An env with n_hist = h under a policy of that depth: the rollout's recorded actions replayed through the CPU oracle give the recorded observations and rewards
    bit for bit; the one-launch update step equals the separate kernels (outputs bit for bit, gradients to float32 rounding)."""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd._lib import check
    import oracle_lib as O
    N, A, T = 96, 4, 10
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True, "n_hist": h}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    assert env.obs_dim == 42 * h
    p = _policy(h, seed=29, scale=1.0)
    env.reset(seed=500)
    roll = mlp.RolloutChains(env, p, T, groups=2, seed=99)
    buf = roll.run()
    records = roll.gae(gamma=0.99, lam=0.95, reward_scale=1e-3)
    torch.cuda.synchronize()
    b = {k: v.cpu() for k, v in buf.items()}
    ora = O.OracleEnv({k: v for k, v in cfg.items() if k != "auto_reset"}, N)
    o0 = ora.reset(seeds=(500 + np.arange(N)).astype(np.uint64))
    assert np.array_equal(b["obs"][0].numpy().view(np.uint32), o0.view(np.uint32))
    for t in range(T):
        oo, orw, ot, otr, _ = ora.step(*[b[k][t].numpy() for k in ACTION_KEYS])
        assert np.array_equal(b["reward"][t].numpy().view(np.uint64), orw.view(np.uint64)), t
        assert np.array_equal(b["obs"][t + 1].numpy().view(np.uint32), oo.view(np.uint32)), t
    ora.close()
    cnt = roll.counter.clone()
    o = p.policy_step(buf["obs"][T // 2], A, seed=99, counter=cnt, draw=T // 2)
    torch.cuda.synchronize()
    for k in (*ACTION_KEYS, "a_cont", "logp"):
        assert torch.equal(o[k].cpu(), b[k][T // 2]), k
    assert torch.equal(p.forward(buf["obs"][T])[:, 24].cpu(), b["value"][T])
    R = T * N
    obs = buf["obs"][:T].view(R, -1)
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(3))
    res = []
    for fused in (False, True):
        upd = mlp.FusedUpdate(p, R, R, A, chunks=3, fused=fused)
        upd.perm.copy_(perm)
        if not fused:
            check(p.L.fn("cda_mlp_prep_rows")(obs.data_ptr(), upd.perm.data_ptr(), R, upd.x_rm.data_ptr(), upd.x_pk.data_ptr(), torch.cuda.current_stream().cuda_stream), "prep")
        upd.minibatch_step(0, R, None, None, None, None, 0.2, 0.5, 0.01, 0.0, (0.9, 0.999), 1e-8, 0.5, records=records, obs_rows=obs if fused else None, debug_outputs=True)
        torch.cuda.synchronize()
        xpk = (upd.x_pk_mb if fused else upd.x_pk)[:R * 32 * p.L.XT].clone()
        res.append(dict(out=upd.out[:R].clone(), grad=upd.grad.clone(), out6=upd.out6.clone(), xpk=xpk, h1=upd.h1p[:R * 512].clone(), h2=upd.h2p[:R * 512].clone()))
    a, c = res
    assert torch.equal(a["xpk"].view(torch.int16), c["xpk"].view(torch.int16))
    assert torch.equal(a["h1"].view(torch.int16), c["h1"].view(torch.int16)) and torch.equal(a["h2"].view(torch.int16), c["h2"].view(torch.int16))
    assert torch.equal(a["out"][:, :25], c["out"][:, :25])
    assert torch.allclose(a["out6"][:6], c["out6"][:6], rtol=1e-4, atol=1e-7)
    assert (a["grad"] - c["grad"]).abs().max() <= 1e-3 * a["grad"].abs().max()
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    env.close()


@pytest.mark.parametrize("h,league", [(1, False), (8, False), (2, True), (8, True), (3, False), (6, True)])
def test_training_loops_run_at_other_depths(h, league):
    from gym_continuousdoubleauction_amd import CDAVecEnv, ppo
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    A = 8 if league else 4
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 16, "is_render": False, "auto_reset": True, "n_hist": h}
    env = CDAVecEnv(cfg, n_markets=128, with_info=False)
    if league:
        bank, lg, hist = train_league_fused(env, iters=3, horizon=16, num_trainable=2, log=lambda s: None, std_dev_multiplier=-10.0, objective=ppo.RLLIB_DEFAULTS)
        assert bank.L.hist == h and all(math.isfinite(v) for hh in hist for p in range(2) for v in hh[f"policy_{p}"].values()) and len(lg.history) >= 1
        assert all(torch.isfinite(pp.theta).all() for pp in bank.policies)
    else:
        pol, hist = ppo.train_fused(env, iters=3, horizon=16, log=lambda s: None, minibatch=128 * 16 * A // 2, objective=ppo.RLLIB_DEFAULTS)
        assert pol.L.hist == h and all(math.isfinite(hh[k]) for hh in hist for k in ("pg_loss", "v_loss", "entropy", "kl")) and hist[-1]["kl"] > 0
        assert float(pol.adam_step.item()) == 3 * 4 * 2 and torch.isfinite(pol.theta).all()
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    env.close()


def test_other_depths_are_refused_with_a_reason():
    from gym_continuousdoubleauction_amd import mlp
    for h in (5, 9, 16):
        with pytest.raises(ValueError, match="compiled for n_hist"):
            mlp.layout(h)
    with pytest.raises(ValueError, match="n_hist"):
        mlp.FusedPolicy(DEV, theta=mlp.init_theta(84), n_hist=4)
