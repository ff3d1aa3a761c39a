"""GPU: the shared-trunk network (RLlib's `vf_share_layers = True`; entry points <name>[_h<H>][_<act>]_vfs, built with CDA_MLP_VFS) against the float64 statement of
the same network (mlp.reference_outputs / reference_gradients with vf_share_layers), float32 autograd through ppo.ActorCritic(vf_share_layers=True), the separate
kernels, and every layer above them: optimiser steps, rollouts through the oracle, the league loop, policy files, evaluation, resume and learning.

A shared trunk keeps the parameter vector of the separate networks with the value half (W1 / b1 rows 256..511, W2 block 1, b2 256..511) at exact zeros; output
row 24 reads the trunk."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 256
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


import mlp_variants as V      # noqa: E402  (the helpers every per-variant test of the network shares)

_obs, _train_forward, _images, _full_backward, _perturb_value_half, _trunk_tiles = V.obs, V.train_forward, V.images, V.full_backward, V.perturb_value_half, V.trunk_tiles


def _theta(n_hist=4, seed=3, scale=1.0, sd=False, hidden=(256, 256)):
    return V.theta(n_hist, True, seed, scale, sd, hidden)


def _policy(act="tanh", n_hist=4, seed=3, scale=1.0, sd=False, hidden=(256, 256)):
    from gym_continuousdoubleauction_amd import mlp
    return mlp.FusedPolicy(DEV, theta=_theta(n_hist, seed, scale, sd, hidden), activation=act, vf_share_layers=True)


@pytest.mark.parametrize("n_hist", [1, 4, 8])
@pytest.mark.parametrize("act", ["tanh", "elu"])
def test_forward_and_stored_activations_equal_the_rounded_reference(act, n_hist):
    """the training forward (h1 / h2 images, outputs), the plain forward and the sampling launch's value against the bf16-rounded float64 reference with
    vf_share_layers; column 24 is the trunk's, and non-zero value-half entries in theta change no output bit"""
    from gym_continuousdoubleauction_amd import mlp
    n = 192
    p = _policy(act, n_hist, seed=3 + n_hist, scale=2.0, sd=n_hist == 4)
    x = _obs(n, n_hist)
    want, xb, h1, h2 = mlp.reference_outputs(p.theta, x, keep=True, activation=act, vf_share_layers=True)
    ws = _train_forward(p, x)
    k1, k2 = _images(ws, n)
    scale = max(1.0, float(h2.abs().max()))
    assert float((k1[:, :H] - h1[:, :H]).abs().max()) <= 2 ** -7 * max(1.0, float(h1.abs().max()))
    assert float((k2[:, :H] - h2[:, :H]).abs().max()) <= 2 ** -6 * scale
    got = ws["out"][:n].cpu().double()
    assert float((got[:, :27] - want[:, :27]).abs().max()) <= 2e-2 * scale, float((got - want).abs().max())
    sep = mlp.reference_outputs(p.theta, x, activation=act)
    assert float((sep[:, 24] - want[:, 24]).abs().max()) > 1e-2                        # (the value column really is the trunk's)
    xd = x.to(DEV)
    out1 = p.forward(xd).clone()
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    s1 = {k: v.clone() for k, v in p.policy_step(xd, 4, seed=7, counter=cnt, draw=0).items()}
    torch.cuda.synchronize()
    assert float((out1.cpu().double()[:, :27] - want[:, :27]).abs().max()) <= 2e-2 * scale
    assert torch.equal(s1["value"], out1[:, 24])
    out_tr = ws["out"][:n, :27].clone()
    _perturb_value_half(p)
    ws2 = _train_forward(p, x)
    out2 = p.forward(xd)
    s2 = p.policy_step(xd, 4, seed=7, counter=cnt, draw=0)
    torch.cuda.synchronize()
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32)) and torch.equal(ws2["out"][:n, :27], out_tr)
    assert torch.equal(_trunk_tiles(ws["h2p"], n).view(torch.int16), _trunk_tiles(ws2["h2p"], n).view(torch.int16))
    for k in s1:
        assert torch.equal(s1[k].view(torch.uint8), s2[k].view(torch.uint8)), k


@pytest.mark.parametrize("n_hist", [1, 4, 8])
@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_backward_and_weight_gradients_equal_the_rounded_reference(act, n_hist):
    from gym_continuousdoubleauction_amd import mlp
    n, chunks = 160, 3
    p = _policy(act, n_hist, scale=2.0)
    L = p.L
    x = _obs(n, n_hist, seed=11)
    d_out = torch.zeros(n, 32)
    d_out[:, :25] = torch.randn(n, 25, generator=torch.Generator().manual_seed(4)) * 1e-3
    ws = _full_backward(p, x, d_out, chunks)
    h1, h2 = _images(ws, n)
    xb = mlp.unpack_rows(ws["x_pk"], n, 32 * L.XT)[:, :L.OBS].double()
    gref, dz1, dz2 = mlp.reference_gradients(p.theta, xb, h1, h2, d_out, activation=act, vf_share_layers=True)
    k2, k1 = mlp.unpack_rows(ws["dz2p"][:n * 512], n, 512, paired=True).double(), mlp.unpack_rows(ws["dz1p"][:n * 512], n, 512, paired=True).double()
    assert (k2[:, :H] - dz2[:, :H]).abs().max() <= 2 ** -7 * dz2.abs().max() and (k1[:, :H] - dz1[:, :H]).abs().max() <= 2 ** -6 * dz1.abs().max()
    grad = ws["grad"].cpu().double()
    assert bool(torch.isfinite(grad).all())
    for a, b in mlp.value_half(L):
        assert bool((grad[a:b] == 0).all())
    for lo, hi, name in ((L.OFF_W1, L.OFF_B1, "W1"), (L.OFF_B1, L.OFF_W2, "b1"), (L.OFF_W2, L.OFF_B2, "W2"), (L.OFF_B2, L.OFF_WO, "b2"),
                         (L.OFF_WO, L.OFF_BO, "Wo"), (L.OFF_BO, L.OFF_LS, "bo")):
        err = (grad[lo:hi] - gref[lo:hi]).abs().max()
        assert err <= 2e-2 * gref[lo:hi].abs().max(), (name, float(err))
    wo = grad[L.OFF_WO:L.OFF_BO].view(32, H)
    assert float(wo[24].abs().max()) > 0 and bool((wo[27:] == 0).all())


@pytest.mark.parametrize("act", ["tanh", "elu"])
def test_whole_gradient_equals_float32_autograd_through_the_pytorch_network(act):
    """the PPO gradient of one minibatch step on the kernels against float32 autograd through ActorCritic(vf_share_layers=True) - the value loss reaching the
    trunk.  Bounds as test_hip_mlp's / test_hip_activation's: cosine > 0.999, 3 % per block (profiles/vf_share/README.md has the measured figures)"""
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd._lib import check
    p = _policy(act, seed=13)
    R, A = 512, 4
    x = _obs(R, seed=17) * 0.5
    g = torch.Generator().manual_seed(6)
    B = R * A
    a_cat, a_price, a_off = torch.randint(0, 9, (B,), generator=g), torch.randint(0, 10, (B,), generator=g), torch.randint(0, 3, (B,), generator=g)
    a_cont = torch.randn(B, 2, generator=g)
    adv, ret, lp_old = torch.randn(B, generator=g), torch.randn(B, generator=g), torch.randn(B, generator=g) * 0.1 - 7.0
    upd = mlp.FusedUpdate(p, R, R, A, chunks=4)
    upd.perm.copy_(torch.arange(R))
    xd = x.to(DEV)
    check(p.L.fn("cda_mlp_prep_rows")(xd.data_ptr(), None, R, upd.x_rm.data_ptr(), upd.x_pk.data_ptr(), torch.cuda.current_stream().cuda_stream), "prep")
    acts = (a_cat.int().to(DEV), a_price.int().to(DEV), a_off.int().to(DEV), a_cont.to(DEV))
    upd.minibatch_step(0, R, acts, lp_old.to(DEV), adv.to(DEV), ret.to(DEV), 0.2, 0.5, 0.01, 0.0, (0.9, 0.999), 1e-8, 0.5)
    torch.cuda.synchronize()
    grad = upd.grad.cpu().double()
    m = p.to_actor_critic().float()
    assert m.vf_share_layers and m.activation == act
    logp, ent, v = m.evaluate(x, (a_cat, a_price, a_off, a_cont), agents_per_row=A)
    ratio = (logp - lp_old).exp()
    loss = -torch.min(ratio * adv, ratio.clamp(0.8, 1.2) * adv).mean() + 0.5 * (v - ret).pow(2).mean() - 0.01 * ent.mean()
    loss.backward()
    gm = torch.zeros(mlp.PARAMS, dtype=torch.float64)
    gm[mlp.OFF_W1:mlp.OFF_B1] = m.l1.weight.grad.double().reshape(-1); gm[mlp.OFF_B1:mlp.OFF_W2] = m.l1.bias.grad.double()
    w2g = m.l2.weight.grad.double()
    gm[mlp.OFF_W2:mlp.OFF_B2] = torch.stack([w2g[:H, :H], w2g[H:, H:]]).reshape(-1); gm[mlp.OFF_B2:mlp.OFF_WO] = m.l2.bias.grad.double()
    wog = m.out.weight.grad.double(); blk = torch.zeros(32, H, dtype=torch.float64); blk[:25] = wog[:25, :H]          # (row 24: the value head on the trunk)
    gm[mlp.OFF_WO:mlp.OFF_BO] = blk.reshape(-1)
    bog = m.out.bias.grad.double().clone(); bog[25:] = 0
    gm[mlp.OFF_BO:mlp.OFF_LS] = bog; gm[mlp.OFF_LS:] = m.log_std.grad.double()
    cos = float((grad * gm).sum() / (grad.norm() * gm.norm()))
    blocks = ((mlp.OFF_W1, mlp.OFF_B1, "W1"), (mlp.OFF_B1, mlp.OFF_W2, "b1"), (mlp.OFF_W2, mlp.OFF_B2, "W2"), (mlp.OFF_B2, mlp.OFF_WO, "b2"),
              (mlp.OFF_WO, mlp.OFF_BO, "Wo"), (mlp.OFF_BO, mlp.OFF_LS, "bo"), (mlp.OFF_LS, mlp.PARAMS, "log_std"))
    rel = {name: float((grad[lo:hi] - gm[lo:hi]).norm() / gm[lo:hi].norm()) for lo, hi, name in blocks}
    print(f"\nVFS-GRAD-VS-FLOAT32 {act}: cos {cos:.6f} " + " ".join(f"{k} {v:.4f}" for k, v in rel.items()))
    assert cos > 0.999, cos
    for name, r in rel.items():
        assert r <= 3e-2, (name, rel)
    for a, b in mlp.value_half(p.L):
        assert bool((grad[a:b] == 0).all()) and bool((gm[a:b] == 0).all())


@pytest.mark.parametrize("n_hist", [1, 4, 8])
def test_fused_forward_loss_backward_equals_the_separate_kernels(n_hist):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd._lib import check
    N, T, A = 96, 40, 4
    env = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 16, "is_render": False, "auto_reset": True, "n_hist": n_hist}, n_markets=N, with_info=False)
    p = _policy("tanh", n_hist, seed=37)                      # (the state-dependent log-std head trains on the fused kernel only: no separate-kernel twin)
    env.reset(seed=11)
    roll = mlp.RolloutChains(env, p, T, groups=2, seed=6)
    buf = roll.run()
    records = roll.gae(gamma=0.99, lam=0.95, reward_scale=1e-3)
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
        res.append(dict(out=upd.out[:R].clone(), d_out=upd.d_out[:R].clone(), grad=upd.grad.clone(), out6=upd.out6.clone(),
                        h1=_trunk_tiles(upd.h1p, R).clone(), h2=_trunk_tiles(upd.h2p, R).clone(),
                        dz2=_trunk_tiles(upd.dz2p, R).float().clone(), dz1=_trunk_tiles(upd.dz1p, R).float().clone()))
    a, b = res
    assert torch.equal(a["h1"].view(torch.int16), b["h1"].view(torch.int16)) and torch.equal(a["h2"].view(torch.int16), b["h2"].view(torch.int16))
    assert torch.equal(a["out"][:, :27], b["out"][:, :27])
    assert float(a["d_out"][:, 24].abs().max()) > 0
    assert torch.allclose(a["d_out"], b["d_out"], rtol=2e-4, atol=2e-5 * float(a["d_out"].abs().max()))
    for k in ("dz2", "dz1"):
        assert (a[k] - b[k]).abs().max() <= 2e-2 * a[k].abs().max()
    assert torch.allclose(a["out6"], b["out6"], rtol=1e-4, atol=1e-7) and float(a["out6"][1]) > 0
    assert (a["grad"] - b["grad"]).abs().max() <= 1e-3 * a["grad"].abs().max()
    for g in (a["grad"], b["grad"]):
        for lo, hi in mlp.value_half(p.L):
            assert bool((g[lo:hi] == 0).all())
    env.close()


def test_value_half_and_dead_units_stay_bit_zero_under_adam():
    from gym_continuousdoubleauction_amd import mlp
    g = torch.Generator().manual_seed(21)
    th0 = _theta(seed=4, hidden=(64, 128))
    p = mlp.FusedPolicy(DEV, theta=th0, activation="relu", vf_share_layers=True)
    R, A = 512, 4
    x = torch.randn(R, mlp.OBS, generator=g) * 0.5
    rec = torch.zeros(R, A, 8)
    rec[..., 0] = torch.randint(0, 9, (R, A), generator=g).int().view(torch.float32)
    rec[..., 1] = torch.randint(0, 10, (R, A), generator=g).int().view(torch.float32)
    rec[..., 2] = torch.randint(0, 3, (R, A), generator=g).int().view(torch.float32)
    rec[..., 3:5] = torch.randn(R, A, 2, generator=g)
    rec[..., 5] = torch.randn(R, A, generator=g) * 0.1 - 7.0
    rec[..., 6] = torch.randn(R, A, generator=g)
    rec[..., 7] = torch.randn(R, A, generator=g)
    upd = mlp.FusedUpdate(p, R, R, A)
    recd, xd = rec.to(DEV), x.to(DEV)
    for step in range(12):
        upd.perm.copy_(torch.randperm(R, generator=g))
        upd.minibatch_step(0, R, None, None, None, None, 0.3, 1.0, 0.01, 1e-3, (0.9, 0.999), 1e-8, 0.5, records=(recd.data_ptr(), None, 0), obs_rows=xd)
    torch.cuda.synchronize()
    th1 = p.theta.cpu()
    dead = th0 == 0
    dead[mlp.OFF_LS:] = False
    assert int(dead.sum()) > 150000 and bool((th1[dead] == 0).all()) and mlp.hidden_widths(th1) == (64, 128) and mlp.value_half_is_zero(th1)
    for a, b in mlp.value_half(p.L):
        assert bool((p.adam_m.cpu()[a:b] == 0).all()) and bool((p.adam_v.cpu()[a:b] == 0).all())
    live = ~dead
    live[mlp.OFF_LS:] = False
    assert float((th1[live] - th0[live]).abs().max()) > 1e-4
    wo0, wo1 = th0[mlp.OFF_WO:mlp.OFF_BO].view(32, H), th1[mlp.OFF_WO:mlp.OFF_BO].view(32, H)
    assert float((wo1[24, :128] - wo0[24, :128]).abs().max()) > 1e-4                   # the value head trains on the trunk
    want = mlp.reference_outputs(th1, x, activation="relu", vf_share_layers=True)
    got = p.forward(xd).cpu().double()
    assert float((got - want)[:, :25].abs().max()) <= 3e-3 * max(1.0, float(want.abs().max()))


def test_shared_trunk_rollout_replays_through_the_oracle_and_equals_per_step_launches(monkeypatch):
    """a shared-trunk policy rolls out with two launches per step (k_policy_step has a separate value network): the recorded actions replay through the oracle,
    the samples and values are what single policy_step launches give, and the rollout is bit for bit the same with CDA_POLICY_STEP=0"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    import oracle_lib as O
    N, A, T = 192, 4, 12
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("CDA_POLICY_STEP", flag)
        env = CDAVecEnv(cfg, n_markets=N, with_info=False)
        p = _policy("tanh", seed=29)
        env.reset(seed=500)
        roll = mlp.RolloutChains(env, p, T, groups=4, seed=99)
        buf = roll.run()
        torch.cuda.synchronize()
        runs.append({k: v.cpu().clone() for k, v in buf.items()})
        if flag == "1":
            cnt = roll.counter.clone()
            for t in range(T):
                o = p.policy_step(buf["obs"][t], A, seed=99, counter=cnt, draw=t)
                torch.cuda.synchronize()
                for k in ("category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp", "value"):
                    assert torch.equal(o[k].cpu(), runs[0][k][t]), (k, t)
            assert torch.equal(p.forward(buf["obs"][T])[:, 24].cpu(), runs[0]["value"][T])          # the bootstrap value: the trunk's column 24
        env.close()
    a, b = runs
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    ora = O.OracleEnv({k: v for k, v in cfg.items() if k != "auto_reset"}, N)
    o0 = ora.reset(seeds=(500 + np.arange(N)).astype(np.uint64))
    assert np.array_equal(a["obs"][0].numpy().view(np.uint32), o0.view(np.uint32))
    for t in range(T):
        oo, orw, *_ = ora.step(a["category"][t].numpy(), a["size_mean"][t].numpy(), a["size_sigma"][t].numpy(), a["price"][t].numpy(), a["price_offset"][t].numpy())
        assert np.array_equal(a["reward"][t].numpy().view(np.uint64), orw.view(np.uint64)), t
        assert np.array_equal(a["obs"][t + 1].numpy().view(np.uint32), oo.view(np.uint32)), t
    ora.close()


def test_shared_trunk_league_trains_promotes_and_its_policies_evaluate_bit_for_bit(tmp_path):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    from gym_continuousdoubleauction_amd.league_train import save_league, train_league_fused
    cfg = {"num_of_agents": 8, "init_cash": 1000000, "max_step": 32, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=256, with_info=False)
    bank, league, hist = train_league_fused(env, iters=6, horizon=16, num_trainable=2, min_iterations_between_champions=2, std_dev_multiplier=-10.0,
                                            max_champions=2, log=lambda s: None, vf_share_layers=True)
    assert bank.vf_share_layers and all(pol.vf_share_layers for pol in bank.policies) and bank.L.suffix == "_vfs"
    assert len(hist) == 6 and all(math.isfinite(v) for h in hist for p in range(2) for v in h[f"policy_{p}"].values())
    assert [h["promoted"] for h in hist] == [None, "champion_1", None, "champion_2", None, "champion_3"]
    assert not torch.equal(bank.policies[0].theta, bank.policies[1].theta)
    for row in range(bank.n_trainable + bank.n_frozen):
        assert mlp.value_half_is_zero(bank.theta[row].cpu())                          # trainable rows and the champions copied from them
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    env.close()
    save_league(str(tmp_path / "lg"), bank, league)
    path = str(tmp_path / "lg" / "policy_0.pt")
    assert mlp.read_policy(path, with_vf_share_layers=True)[1] is True
    loaded = mlp.load_policy(path, DEV)
    assert loaded.vf_share_layers and torch.equal(loaded.theta.cpu().view(torch.int32), bank.theta[0].cpu().view(torch.int32))
    inmem = mlp.FusedPolicy(DEV, theta=bank.theta[0].cpu(), vf_share_layers=True)
    ev = CDAVecEnv(dict(cfg, num_of_agents=4), n_markets=128, with_info=False)
    ka, kb = {}, {}
    a = evaluate(ev, inmem, episodes=2, seed=1, keep=ka)
    b = evaluate(ev, path, episodes=2, seed=1, keep=kb)
    assert a["summary"] == b["summary"]
    for k in ka["actions"]:
        assert torch.equal(ka["actions"][k].view(torch.uint8), kb["actions"][k].view(torch.uint8)), k
    c = evaluate(ev, path, opponents=["random", str(tmp_path / "lg" / "policy_1.pt")], episodes=1, seed=2)
    assert c["nav_conservation_violations"] == 0
    sep_path = str(tmp_path / "sep.pt")
    mlp.save_policy(sep_path, mlp.FusedPolicy(DEV, seed=5))
    with pytest.raises(ValueError, match="vf_share_layers"):
        evaluate(ev, path, opponents=[sep_path], episodes=1)
    with pytest.raises(ValueError, match="vf_share_layers"):
        evaluate(ev, sep_path, opponents=[path], episodes=1)
    ev.close()


def test_shared_trunk_resume_is_exact_and_a_separate_run_refuses_its_checkpoint(tmp_path):
    import shutil
    from gym_continuousdoubleauction_amd import CDAVecEnv, ppo
    cfg = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 48, "is_render": False, "auto_reset": True}
    kw = dict(horizon=32, minibatch=256 * 32 * 4 // 2, chains=2, log=lambda *_: None, vf_share_layers=True)
    keep_a = {}
    a_dir, b_dir, c_dir = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    pol_a, _ = ppo.train_fused(CDAVecEnv(cfg, n_markets=256, with_info=False), iters=3, keep=keep_a, checkpoint_dir=a_dir, chkpt_freq=2, **kw)
    assert pol_a.vf_share_layers
    names = ("obs", "category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp", "value", "reward", "record")
    bufs_a = {k: keep_a["buffers"][k].clone() for k in names}
    thetas = []
    for d in (b_dir, c_dir):
        shutil.copytree(os.path.join(a_dir, "iter_2"), os.path.join(d, "iter_2"))
        keep = {}
        pol, hist = ppo.train_fused(CDAVecEnv(cfg, n_markets=256, with_info=False), iters=3, keep=keep, checkpoint_dir=d, restore=True, **kw)
        assert [h["iter"] for h in hist] == [2]
        for k in names:
            assert torch.equal(bufs_a[k].view(torch.uint8), keep["buffers"][k].view(torch.uint8)), k
        thetas.append(pol.theta.clone())
    spread = (thetas[0] - thetas[1]).abs().max().item()
    diff = (thetas[0] - pol_a.theta).abs().max().item()
    if spread == 0.0:
        assert torch.equal(thetas[0].view(torch.int32), pol_a.theta.view(torch.int32))
    else:
        assert diff <= spread
    with pytest.raises(ValueError, match="vf_share_layers"):
        ppo.train_fused(CDAVecEnv(cfg, n_markets=256, with_info=False), iters=3, checkpoint_dir=a_dir, restore=True, **dict(kw, vf_share_layers=False))


def test_shared_trunk_fused_loop_improves_the_episode_return_and_tracks_the_float32_torch_loop():
    """test_hip_learning's run (40 iterations of 1024 markets x 4 agents x 32-step episodes at lr 3e-4) with a shared trunk in both loops (the float32 torch loop:
    ppo.train with ActorCritic(vf_share_layers=True)), held to that test's bars except the starting point, which depends on each loop's initial draw.  Measured on
    MI355X (tools/learning_curve.py --vf-share-layers; profiles/vf_share/README.md): fused -1790 -> -1.86, float32 torch -2480 -> -2.69 - starts 0.72 x apart,
    ends 0.03 % of the float32 loop's start apart."""
    from learning_curve import curves
    c = curves(markets=1024, agents=4, episode=32, iters=40, lr=3e-4, seed=0, vf_share_layers=True)
    f, l = c["fused"], c["legacy"]
    assert all(x is not None and math.isfinite(x) for x in f) and all(math.isfinite(x) for x in l)
    f0, f1, l0, l1 = sum(f[:3]) / 3, sum(f[-3:]) / 3, sum(l[:3]) / 3, sum(l[-3:]) / 3
    print(f"\nVFS-LEARNING: fused {f0:.1f} -> {f1:.2f}, float32 torch {l0:.1f} -> {l1:.2f}")
    assert f0 < -1000 and l0 < -1000, (f0, l0)
    assert 0.4 <= f0 / l0 <= 3.0, (f0, l0)
    assert f1 > 0.02 * f0, (f0, f1)
    assert l1 > 0.02 * l0, (l0, l1)
    assert abs(f1 - l1) <= 0.01 * abs(l0), (f1, l1)
    assert min(f[20:]) > 0.02 * f0
