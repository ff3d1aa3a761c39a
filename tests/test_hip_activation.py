"""GPU: the network kernels compiled for the other hidden activations (the reference's `fcnet_activation`: relu, elu, linear; csrc/cda_mlp_dev.inc ActT, entry points
<name>[_h<H>]_<act>) against the float64 statement of the same network (mlp.reference_outputs / reference_gradients with `activation`), float32 autograd through
ppo.ActorCritic(activation=...), and every layer above them: rollouts through the oracle, the league loop, policy files, evaluation, resume and learning.

relu, elu and linear are unbounded: the bfloat16 one-ulp flips that the tanh tests bound absolutely (|h| <= 1) are bounded here relative to max |h|."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACTS = ("relu", "elu", "linear")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


import mlp_variants as V      # noqa: E402  (the helpers every per-variant test of the network shares)

_obs, _train_forward, _images, _full_backward = V.obs, V.train_forward, V.images, V.full_backward


def _policy(act, n_hist=4, seed=3, scale=1.0, hidden=(256, 256)):
    return V.policy(n_hist, act, False, seed, scale, False, hidden)


@pytest.mark.parametrize("n_hist", [1, 4, 8])
@pytest.mark.parametrize("act", ACTS)
def test_forward_and_stored_activations_equal_the_rounded_reference(act, n_hist):
    from gym_continuousdoubleauction_amd import mlp
    n = 160                                                        # (the update's row images come in whole 32-row tiles)
    p = _policy(act, n_hist, scale=2.0)
    assert p.activation == act and p.L.suffix.endswith("_" + act)
    x = _obs(n, n_hist)
    out = p.forward(x.to(DEV)).cpu().double()
    ref, xb, h1, h2 = mlp.reference_outputs(p.theta, x, keep=True, activation=act)
    hmax = max(1.0, float(h1.abs().max()), float(h2.abs().max()))
    tol = 3e-3 * max(1.0, float(ref.abs().max())) * hmax
    assert (out[:, :25] - ref[:, :25]).abs().max() <= tol, (float((out[:, :25] - ref[:, :25]).abs().max()), tol)
    assert (out[:, 25:] == 0).all()
    ws = _train_forward(p, x)
    g1, g2 = _images(ws, n)
    # one bfloat16 ulp where float32 and float64 pre-activations round differently (2^-8 relative), and h2 inherits h1's flips
    assert (g1 - h1).abs().max() <= 2 ** -7 * max(1.0, float(h1.abs().max())) and (g1 != h1).double().mean() < 0.02
    assert (g2 - h2).abs().max() <= 2 ** -6 * max(1.0, float(h2.abs().max())) and (g2 != h2).double().mean() < 0.05
    assert torch.equal(ws["out"][:n].cpu().double(), out)          # the training forward and the rollout's forward: the same outputs bit for bit
    if act == "relu":
        assert bool((g1 >= 0).all()) and float((g1 == 0).double().mean()) > 0.2
    # the activation is applied: the tanh kernels give other outputs for the same parameters
    tanh = mlp.FusedPolicy(DEV, theta=p.theta.cpu()).forward(x.to(DEV)).cpu().double()
    assert float((tanh[:, :25] - out[:, :25]).abs().max()) > 1e-2


@pytest.mark.parametrize("act", ACTS)
def test_small_pre_activations(act):
    """most pre-activations |z| < 1e-3 (ELU's e^z - 1 near 0-): the stored activations against the float64 statement, and, with W1 = W2 = 0, each stored
    activation within one bfloat16 ulp of the float64 activation of the kernel's own float32 pre-activation (= the bias) over |z| from 1e-9 to 10"""
    from gym_continuousdoubleauction_amd import mlp
    n = 128
    th = mlp.init_theta(generator=torch.Generator().manual_seed(31))
    th[:mlp.OFF_LS] *= 2e-3
    p = mlp.FusedPolicy(DEV, theta=th, activation=act)
    x = _obs(n, seed=32) * 0.3
    ws = _train_forward(p, x)
    g1, g2 = _images(ws, n)
    _, _, h1, h2 = mlp.reference_outputs(p.theta, x, keep=True, activation=act)
    assert float((h1.abs() < 1e-3).double().mean()) > 0.5
    # (relative: one bfloat16 ulp; the 1e-9 floor covers pre-activations within float32 accumulation error of zero, ~1e-11 here)
    assert bool(((g1 - h1).abs() <= 2 ** -7 * h1.abs() + 1e-9).all()), float(((g1 - h1).abs() / h1.abs().clamp_min(1e-9)).max())
    assert bool(((g2 - h2).abs() <= 2 ** -6 * h2.abs() + 1e-9).all())
    # the biases alone: z = b exactly (zero weights)
    z = torch.cat([-torch.logspace(-9, 1, 240, dtype=torch.float64), torch.logspace(-9, 1, 16, dtype=torch.float64)]).float()
    th = torch.zeros(mlp.PARAMS)
    th[mlp.OFF_B1:mlp.OFF_W2] = torch.cat([z, z.flip(0)])
    th[mlp.OFF_B2:mlp.OFF_WO] = torch.cat([z.flip(0), z])
    p = mlp.FusedPolicy(DEV, theta=th, activation=act)
    g1, g2 = _images(_train_forward(p, _obs(32, seed=33)), 32)
    for g, b in ((g1, th[mlp.OFF_B1:mlp.OFF_W2]), (g2, th[mlp.OFF_B2:mlp.OFF_WO])):
        want = mlp.act_fn(act)(b.double()).expand(32, 512)
        ulp = torch.exp2(torch.floor(torch.log2(want.abs())) - 7)
        assert bool(((g - want).abs() <= ulp).all()), float(((g - want).abs() / ulp).max())


@pytest.mark.parametrize("n_hist", [1, 4, 8])
@pytest.mark.parametrize("act", ACTS)
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
    gref, dz1, dz2 = mlp.reference_gradients(p.theta, xb, h1, h2, d_out, activation=act)
    k2, k1 = mlp.unpack_rows(ws["dz2p"][:n * 512], n, 512, paired=True).double(), mlp.unpack_rows(ws["dz1p"][:n * 512], n, 512, paired=True).double()
    assert (k2 - dz2).abs().max() <= 2 ** -7 * dz2.abs().max() and (k1 - dz1).abs().max() <= 2 ** -6 * dz1.abs().max()
    if act == "relu":                                              # relu'(z) = 0 where the stored h is 0: those dz are exact zeros
        assert bool((k2[h2 == 0] == 0).all()) and bool((k1[h1 == 0] == 0).all())
    g_mine = torch.zeros(L.PARAMS, dtype=torch.float64)
    g_mine[L.OFF_W1:L.OFF_B1] = (k1.t() @ xb).reshape(-1); g_mine[L.OFF_B1:L.OFF_W2] = k1.sum(0)
    g_mine[L.OFF_W2:L.OFF_B2] = torch.stack([k2[:, :256].t() @ h1[:, :256], k2[:, 256:].t() @ h1[:, 256:]]).reshape(-1); g_mine[L.OFF_B2:L.OFF_WO] = k2.sum(0)
    g_mine[L.OFF_WO:L.OFF_LS] = gref[L.OFF_WO:L.OFF_LS]
    grad = ws["grad"].cpu().double()
    for lo, hi, name in ((L.OFF_W1, L.OFF_B1, "W1"), (L.OFF_B1, L.OFF_W2, "b1"), (L.OFF_W2, L.OFF_B2, "W2"), (L.OFF_B2, L.OFF_WO, "b2"),
                         (L.OFF_WO, L.OFF_BO, "Wo"), (L.OFF_BO, L.OFF_LS, "bo")):
        err = (grad[lo:hi] - g_mine[lo:hi]).abs().max()
        assert err <= 1e-4 * g_mine[lo:hi].abs().max() + 1e-12, (name, float(err))
        err = (grad[lo:hi] - gref[lo:hi]).abs().max()
        assert err <= 2e-2 * gref[lo:hi].abs().max(), (name, float(err))


@pytest.mark.parametrize("act", ACTS)
def test_whole_gradient_equals_float32_autograd_through_the_pytorch_network(act):
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
    lpd0, advd0, retd0 = lp_old.to(DEV), adv.to(DEV), ret.to(DEV)
    upd.minibatch_step(0, R, acts, lpd0, advd0, retd0, 0.2, 0.5, 0.01, 0.0, (0.9, 0.999), 1e-8, 0.5)
    torch.cuda.synchronize()
    grad = upd.grad.cpu().double()
    m = p.to_actor_critic().float()
    assert m.activation == act
    logp, ent, v = m.evaluate(x, (a_cat, a_price, a_off, a_cont), agents_per_row=A)
    ratio = (logp - lp_old).exp()
    loss = -torch.min(ratio * adv, ratio.clamp(0.8, 1.2) * adv).mean() + 0.5 * (v - ret).pow(2).mean() - 0.01 * ent.mean()
    loss.backward()
    gm = torch.zeros(mlp.PARAMS, dtype=torch.float64)
    H = 256
    gm[mlp.OFF_W1:mlp.OFF_B1] = m.l1.weight.grad.double().reshape(-1); gm[mlp.OFF_B1:mlp.OFF_W2] = m.l1.bias.grad.double()
    w2g = m.l2.weight.grad.double()
    gm[mlp.OFF_W2:mlp.OFF_B2] = torch.stack([w2g[:H, :H], w2g[H:, H:]]).reshape(-1); gm[mlp.OFF_B2:mlp.OFF_WO] = m.l2.bias.grad.double()
    wog = m.out.weight.grad.double(); blk = torch.zeros(32, H, dtype=torch.float64); blk[:24] = wog[:24, :H]; blk[24] = wog[24, H:]
    gm[mlp.OFF_WO:mlp.OFF_BO] = blk.reshape(-1)
    bog = m.out.bias.grad.double().clone(); bog[25:] = 0
    gm[mlp.OFF_BO:mlp.OFF_LS] = bog; gm[mlp.OFF_LS:] = m.log_std.grad.double()
    cos = float((grad * gm).sum() / (grad.norm() * gm.norm()))
    assert cos > 0.999, cos
    blocks = ((mlp.OFF_W1, mlp.OFF_B1, "W1"), (mlp.OFF_B1, mlp.OFF_W2, "b1"), (mlp.OFF_W2, mlp.OFF_B2, "W2"), (mlp.OFF_B2, mlp.OFF_WO, "b2"),
              (mlp.OFF_WO, mlp.OFF_BO, "Wo"), (mlp.OFF_BO, mlp.OFF_LS, "bo"), (mlp.OFF_LS, mlp.PARAMS, "log_std"))
    rel = {name: float((grad[lo:hi] - gm[lo:hi]).norm() / gm[lo:hi].norm()) for lo, hi, name in blocks}
    print(f"\nGRAD-VS-FLOAT32 {act}: cos {cos:.6f} " + " ".join(f"{k} {v:.4f}" for k, v in rel.items()))
    for lo, hi, name in blocks:
        a, b = grad[lo:hi], gm[lo:hi]
        # test_hip_mlp's 3 % per block, except relu: relu' is a 0 / 1 mask decided by the sign of the pre-activation, and the kernel's (bf16 operands) and
        # float32's disagree on units with |z| below the operand rounding - whole entries of h and dz flip, forward and backward.  Measured on MI355X:
        # W1 6.7 %, b1 6.5 %, W2 5.8 %, b2 5.8 %, Wo 2.4 %, bo 3.2 %, cos 0.9995 (elu <= 0.4 %, linear <= 1.9 %; profiles/activation/)
        bound = 1e-1 if act == "relu" else 3e-2
        assert (a - b).norm() <= bound * b.norm() + 1e-9, (name, rel)


@pytest.mark.parametrize("n_hist", [1, 4, 8])
@pytest.mark.parametrize("act", ACTS)
def test_fused_forward_loss_backward_equals_the_separate_kernels(act, n_hist):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd._lib import check
    N, T, A = 96, 40, 4
    env = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 16, "is_render": False, "auto_reset": True, "n_hist": n_hist}, n_markets=N, with_info=False)
    p = _policy(act, n_hist, seed=37)
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
                        h1=upd.h1p[:R * 512].clone(), h2=upd.h2p[:R * 512].clone(), dz2=upd.dz2p[:R * 512].float().clone(), dz1=upd.dz1p[:R * 512].float().clone()))
    a, b = res
    assert torch.equal(a["h1"].view(torch.int16), b["h1"].view(torch.int16)) and torch.equal(a["h2"].view(torch.int16), b["h2"].view(torch.int16))
    assert torch.equal(a["out"][:, :25], b["out"][:, :25])
    assert torch.allclose(a["d_out"], b["d_out"], rtol=2e-4, atol=2e-5 * float(a["d_out"].abs().max()))
    for k in ("dz2", "dz1"):
        assert (a[k] - b[k]).abs().max() <= 2e-2 * a[k].abs().max()
    assert torch.allclose(a["out6"], b["out6"], rtol=1e-4, atol=1e-7)
    assert (a["grad"] - b["grad"]).abs().max() <= 1e-3 * a["grad"].abs().max()
    env.close()


@pytest.mark.parametrize("act", ACTS)
def test_dead_units_stay_bit_zero_under_adam(act):
    from gym_continuousdoubleauction_amd import mlp
    g = torch.Generator().manual_seed(21)
    th0 = mlp.init_theta(generator=torch.Generator().manual_seed(4), hidden=(64, 128))
    p = mlp.FusedPolicy(DEV, theta=th0, activation=act)
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
    for step in range(6):
        upd.perm.copy_(torch.randperm(R, generator=g))
        upd.minibatch_step(0, R, None, None, None, None, 0.3, 1.0, 0.01, 1e-3, (0.9, 0.999), 1e-8, 0.5, records=(recd.data_ptr(), None, 0), obs_rows=xd)
    torch.cuda.synchronize()
    th1 = p.theta.cpu()
    dead = th0 == 0
    dead[mlp.OFF_LS:] = False
    assert int(dead.sum()) > 50000 and bool((th1[dead] == 0).all()) and mlp.hidden_widths(th1) == (64, 128)       # bit-zero, not small
    live = ~dead
    live[mlp.OFF_LS:] = False
    assert float((th1[live] - th0[live]).abs().max()) > 1e-4
    # the narrow network's outputs: the float64 statement of the trained parameters
    want = mlp.reference_outputs(th1, x, activation=act)
    _, _, h1, h2 = mlp.reference_outputs(th1, x, keep=True, activation=act)
    got = p.forward(xd).cpu().double()
    assert float((got - want)[:, :25].abs().max()) <= 3e-3 * max(1.0, float(want.abs().max())) * max(1.0, float(h2.abs().max()))


@pytest.mark.parametrize("act", ["relu", "elu"])
def test_shared_policy_rollout_replays_through_the_oracle_and_equals_the_two_launch_path(act, monkeypatch):
    """a non-tanh shared policy rolls out with two launches per step (k_policy_step is the tanh network's): the recorded actions replay through the oracle, the
    samples are what a single policy_step of the same kernels gives, and the rollout is bit for bit the one with CDA_POLICY_STEP=0"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    import oracle_lib as O
    N, A, T = 192, 4, 12
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("CDA_POLICY_STEP", flag)
        env = CDAVecEnv(cfg, n_markets=N, with_info=False)
        p = _policy(act, seed=29)
        env.reset(seed=500)
        roll = mlp.RolloutChains(env, p, T, groups=4, seed=99)
        buf = roll.run()
        torch.cuda.synchronize()
        runs.append({k: v.cpu().clone() for k, v in buf.items()})
        if flag == "1":
            cnt = roll.counter.clone()
            for t in (0, T - 1):
                o = p.policy_step(buf["obs"][t], A, seed=99, counter=cnt, draw=t)
                torch.cuda.synchronize()
                for k in ("category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp", "value"):
                    assert torch.equal(o[k].cpu(), runs[0][k][t]), (k, t)
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


def test_relu_league_trains_promotes_and_its_policies_evaluate_bit_for_bit(tmp_path):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    from gym_continuousdoubleauction_amd.league_train import save_league, train_league_fused
    cfg = {"num_of_agents": 8, "init_cash": 1000000, "max_step": 32, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=256, with_info=False)
    # (test_hip_league's promotion schedule: std_dev_multiplier -10 promotes the best trainable policy after iterations 1, 3, 5)
    bank, league, hist = train_league_fused(env, iters=6, horizon=16, num_trainable=2, min_iterations_between_champions=2, std_dev_multiplier=-10.0,
                                            max_champions=2, log=lambda s: None, activation="relu")
    assert bank.activation == "relu" and all(pol.activation == "relu" for pol in bank.policies) and bank.L.suffix == "_relu"
    assert len(hist) == 6 and all(math.isfinite(v) for h in hist for p in range(2) for v in h[f"policy_{p}"].values())
    assert [h["promoted"] for h in hist] == [None, "champion_1", None, "champion_2", None, "champion_3"]
    assert not torch.equal(bank.policies[0].theta, bank.policies[1].theta)
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    env.close()
    save_league(str(tmp_path / "lg"), bank, league)
    path = str(tmp_path / "lg" / "policy_0.pt")
    assert mlp.read_policy(path, with_activation=True)[1] == "relu"
    loaded = mlp.load_policy(path, DEV)
    assert loaded.activation == "relu" and torch.equal(loaded.theta.cpu().view(torch.int32), bank.theta[0].cpu().view(torch.int32))
    inmem = mlp.FusedPolicy(DEV, theta=bank.theta[0].cpu(), activation="relu")
    ev = CDAVecEnv(dict(cfg, num_of_agents=4), n_markets=128, with_info=False)
    ka, kb = {}, {}
    a = evaluate(ev, inmem, episodes=2, seed=1, keep=ka)
    b = evaluate(ev, path, episodes=2, seed=1, keep=kb)
    assert a["summary"] == b["summary"] and a["config"]["activation"] == "relu"
    for k in ka["actions"]:
        assert torch.equal(ka["actions"][k].view(torch.uint8), kb["actions"][k].view(torch.uint8)), k
    c = evaluate(ev, path, opponents=["random", str(tmp_path / "lg" / "policy_1.pt")], episodes=1, seed=2)
    assert c["nav_conservation_violations"] == 0
    # a tanh opponent against a relu policy is refused before anything runs
    tanh_path = str(tmp_path / "tanh.pt")
    mlp.save_policy(tanh_path, mlp.FusedPolicy(DEV, seed=5))
    with pytest.raises(ValueError, match="tanh"):
        evaluate(ev, path, opponents=[tanh_path], episodes=1)
    with pytest.raises(ValueError, match="tanh"):
        evaluate(ev, path, opponents=[mlp.FusedPolicy(DEV, seed=5)], episodes=1)
    ev.close()


def test_relu_ppo_resume_is_exact_and_a_tanh_run_refuses_its_checkpoint(tmp_path):
    import shutil
    from gym_continuousdoubleauction_amd import CDAVecEnv, ppo
    cfg = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 48, "is_render": False, "auto_reset": True}
    kw = dict(horizon=32, minibatch=256 * 32 * 4 // 2, chains=2, log=lambda *_: None, activation="relu")
    keep_a = {}
    a_dir, b_dir, c_dir = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    pol_a, _ = ppo.train_fused(CDAVecEnv(cfg, n_markets=256, with_info=False), iters=3, keep=keep_a, checkpoint_dir=a_dir, chkpt_freq=2, **kw)
    assert pol_a.activation == "relu"
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
    with pytest.raises(ValueError, match="activation"):
        ppo.train_fused(CDAVecEnv(cfg, n_markets=256, with_info=False), iters=3, checkpoint_dir=a_dir, restore=True,
                        **dict(kw, activation="tanh"))


def test_relu_fused_loop_improves_the_episode_return_and_tracks_the_float32_torch_loop():
    """test_hip_learning's run (40 iterations of 1024 markets x 4 agents x 32-step episodes at lr 3e-4) with relu networks in both loops, held to that test's bars
    except the starting point: the two loops draw their initial weights differently, and an untrained relu network's return depends on that draw far more than a
    tanh one's (measured on MI355X: fused -2594 -> -6.3, float32 torch -1182 -> -1.4; profiles/activation/relu_learning.txt)"""
    from learning_curve import curves
    c = curves(markets=1024, agents=4, episode=32, iters=40, lr=3e-4, seed=0, activation="relu")
    f, l = c["fused"], c["legacy"]
    assert all(x is not None and math.isfinite(x) for x in f) and all(math.isfinite(x) for x in l)
    f0, f1, l0, l1 = sum(f[:3]) / 3, sum(f[-3:]) / 3, sum(l[:3]) / 3, sum(l[-3:]) / 3
    print(f"\nRELU-LEARNING: fused {f0:.1f} -> {f1:.2f}, float32 torch {l0:.1f} -> {l1:.2f}")
    assert f0 < -1000 and l0 < -1000, (f0, l0)
    assert 0.4 <= f0 / l0 <= 3.0, (f0, l0)                      # (tanh: within 35 % of each other; relu measured 2.2 x)
    assert f1 > 0.02 * f0, (f0, f1)
    assert l1 > 0.02 * l0, (l0, l1)
    assert abs(f1 - l1) <= 0.01 * abs(l0), (f1, l1)
    assert min(f[20:]) > 0.02 * f0
