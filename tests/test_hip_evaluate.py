"""Evaluation on the fused network kernels: mode actions (cda_mlp_policy_act / cda_mlp_league_act), the greedy chains, policy files and evaluate()."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEPTHS = (1, 2, 3, 4, 6, 7, 8)
ULP1 = float(np.spacing(np.float32(1.0)))          # 2^-23


def _obs(N, obs_dim, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((N, obs_dim), generator=g) * 2).cuda()


def _mode_reference(out, log_std, head):
    """argmax of each categorical head (torch: lowest index on a tie), the means, and the mode's log-probability in float64"""
    o = out.double().cpu()
    heads = ((0, 9), (9, 19), (19, 22))
    idx = [torch.argmax(out[:, a:b].cpu(), dim=1) for a, b in heads]
    ls = log_std.double().cpu().view(1, 2) + (o[:, 25:27] if head else 0.0)
    lp = sum(o[:, a:b].gather(1, i.view(-1, 1)).view(-1) - torch.logsumexp(o[:, a:b], dim=1) for (a, b), i in zip(heads, idx))
    lp = lp - ls[:, 0] - ls[:, 1] - math.log(2 * math.pi)
    return idx, lp


def _check_mode(o, out, log_std, head, rows=None):
    """o: act()'s dict for [N, A]; out: forward() rows of the same markets"""
    rows = slice(None) if rows is None else rows
    A = o["category"].shape[1]
    (cat, price, off), lp = _mode_reference(out, log_std, head)
    for k, ref in (("category", cat), ("price", price), ("price_offset", off)):
        assert torch.equal(o[k][rows].cpu().long(), ref.view(-1, 1).expand(-1, A)), k
    means = out[:, 22:24].cpu()
    assert torch.equal(o["a_cont"][rows].cpu(), means.view(-1, 1, 2).expand(-1, A, 2))
    tol = 4 * ULP1           # (the device's 1 - 2 / (e^2x + 1) is accurate to a few ulp OF ONE, not of tanh near zero: an absolute bound)
    assert (o["size_mean"][rows].cpu() - torch.tanh(means[:, :1])).abs().max() <= tol
    assert (o["size_sigma"][rows].cpu() - torch.sigmoid(means[:, 1:])).abs().max() <= tol
    assert (o["logp"][rows].cpu().double() - lp.view(-1, 1)).abs().max() <= 2e-4


@pytest.mark.parametrize("n_hist", DEPTHS)
def test_mode_actions_are_the_argmax_and_the_means_of_the_forward_pass(n_hist):
    from gym_continuousdoubleauction_amd import mlp
    N, A = 200, 4
    for head in (False, True):
        p = mlp.FusedPolicy("cuda:0", seed=11 + n_hist, n_hist=n_hist, state_dependent_log_std=head)
        obs = _obs(N, 42 * n_hist, n_hist)
        out = p.forward(obs)
        o = p.act(obs, A)
        torch.cuda.synchronize()
        _check_mode(o, out, p.log_std, head)
        assert torch.equal(o["value"].cpu(), out[:, 24].cpu())
        o2 = p.act(obs, A)
        for k in o:
            assert torch.equal(o[k], o2[k]), k
    # all logits equal (zero output weights and biases of the three heads): index 0 in every head
    L = mlp.layout(n_hist)
    th = p.theta.detach().cpu().clone()
    wo = th[L.OFF_WO:L.OFF_BO].view(mlp.NOUT, mlp.HID)
    wo[:22] = 0
    th[L.OFF_BO:L.OFF_BO + 22] = 0
    z = mlp.FusedPolicy("cuda:0", theta=th).act(obs, A)
    for k in ("category", "price", "price_offset"):
        assert int(z[k].abs().max()) == 0, k


@pytest.mark.parametrize("n_hist", DEPTHS)
def test_league_mode_actions_are_greedy_on_network_slots_and_draw_on_random_ones(n_hist):
    from gym_continuousdoubleauction_amd import mlp
    N, A = 160, 4
    bank = mlp.PolicyBank("cuda:0", N, A, n_trainable=2, max_frozen=2, seed=3 + n_hist, random_seed=77, n_hist=n_hist, state_dependent_log_std=True)
    frozen = mlp.FusedPolicy("cuda:0", seed=99, n_hist=n_hist)
    row = bank.snapshot(0)
    bank.theta[row].copy_(frozen.theta); bank.wb[row].copy_(frozen.wb)
    slot = np.empty((N, A), np.int32)
    slot[:, 0], slot[:, 1] = 0, 1
    slot[:, 2] = np.where(np.arange(N) % 2 == 0, row, mlp.LEAGUE_RANDOM)
    slot[:, 3] = mlp.LEAGUE_RANDOM
    bank.set_slots(torch.from_numpy(slot))
    obs = _obs(N, 42 * n_hist, 100 + n_hist)
    c1, c2 = torch.tensor([5], dtype=torch.int64, device="cuda:0"), torch.tensor([9], dtype=torch.int64, device="cuda:0")
    g1 = bank.act(obs, seed=1, counter=c1, draw=3)
    g2 = bank.act(obs, seed=2, counter=c2, draw=4)
    s1 = bank.act(obs, seed=1, counter=c1, draw=3, greedy=False)
    torch.cuda.synchronize()
    nets = {0: bank.policies[0], 1: bank.policies[1], row: frozen}
    for net, pol in nets.items():
        out = pol.forward(obs)
        head = mlp.has_log_std_head(pol.theta)
        for a in range(A):
            rows = torch.from_numpy(np.nonzero(slot[:, a] == net)[0])
            if len(rows) == 0:
                continue
            sub = {k: v[rows][:, a:a + 1] for k, v in g1.items() if k != "value"}
            _check_mode(sub, out[rows.cuda()], pol.log_std, head)
            for k in sub:                                           # the network slots ignore seed / counter / draw
                assert torch.equal(g1[k][rows][:, a], g2[k][rows][:, a]), (net, k)
    rnd = torch.from_numpy(slot == mlp.LEAGUE_RANDOM).cuda()
    for k in ("category", "size_mean", "size_sigma", "price", "price_offset"):    # random-module slots: exactly the sampled step's draws
        assert torch.equal(g1[k][rnd], s1[k][rnd]), k
    for p in range(2):
        assert torch.equal(g1["value"][p].cpu(), bank.policies[p].forward(obs)[:, 24].cpu())


@pytest.mark.parametrize("N,A", [(512, 4), (256, 8)])
@pytest.mark.parametrize("league", [False, True])
def test_a_greedy_rollout_replays_through_the_oracle(N, A, league):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    import oracle_lib as O
    T = 64
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    if league:
        pol = mlp.PolicyBank("cuda:0", N, A, n_trainable=1, max_frozen=1, seed=21, random_seed=5)
        slot = np.full((N, A), mlp.LEAGUE_RANDOM, np.int32); slot[:, 0] = 0
        pol.set_slots(torch.from_numpy(slot))
    else:
        pol = mlp.FusedPolicy("cuda:0", seed=21)
    env.reset(seed=700)
    roll = mlp.RolloutChains(env, pol, T, groups=4, seed=3, greedy=True)
    buf = roll.run()
    torch.cuda.synchronize()
    b = {k: v.cpu() for k, v in buf.items()}
    ora = O.OracleEnv({k: v for k, v in cfg.items() if k != "auto_reset"}, N)
    o0 = ora.reset(seeds=(700 + np.arange(N)).astype(np.uint64))
    assert np.array_equal(b["obs"][0].numpy().view(np.uint32), o0.view(np.uint32))
    for t in range(T):
        oo, orw, ot, otr, _ = ora.step(b["category"][t].numpy(), b["size_mean"][t].numpy(), b["size_sigma"][t].numpy(), b["price"][t].numpy(), b["price_offset"][t].numpy())
        assert np.array_equal(b["reward"][t].numpy().view(np.uint64), orw.view(np.uint64)), t
        assert np.array_equal(b["obs"][t + 1].numpy().view(np.uint32), oo.view(np.uint32)), t
        assert np.array_equal(b["terminated"][t].numpy().astype(bool), np.asarray(ot).astype(bool)), t
        assert np.array_equal(b["truncated"][t].numpy().astype(bool), np.asarray(otr).astype(bool)), t
    if not league:                                                # every step's actions = act() on that step's observation
        for t in (0, T - 1):
            o = pol.act(buf["obs"][t], A)
            torch.cuda.synchronize()
            for k in ("category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp"):
                assert torch.equal(o[k].cpu(), b[k][t]), (k, t)
    assert (env.flags() == 0).all()
    env.close(); ora.close()


def _env(N, A, max_step):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    return CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}, n_markets=N, with_info=False)


@pytest.mark.parametrize("opponents", [None, ["random"]])
def test_evaluate_metrics_equal_an_oracle_replay_of_its_actions(opponents):
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    from episode_metrics_util import OracleEpisodeMetrics, assert_tables_equal
    import oracle_lib as O
    N, A, ms, seed = 64, 4, 32, 4
    env = _env(N, A, ms)
    keep = {}
    res = evaluate(env, mlp.FusedPolicy("cuda:0", seed=8), opponents=opponents, episodes=2, seed=seed, keep=keep)
    assert res["nav_conservation_violations"] == 0 and res["episodes"] >= N
    assert env.episode_metrics_on is False                            # restored
    acts = keep["actions"]
    ora = O.OracleEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": ms, "is_render": False}, N)
    ora.reset(seeds=(np.uint64(seed) * np.uint64(N) + np.arange(N, dtype=np.uint64)))
    em = OracleEpisodeMetrics(N, A, 1000000)
    for t in range(acts["category"].shape[0]):
        _, rew, term, trunc, info = ora.step(*(acts[k][t].numpy() for k in ("category", "size_mean", "size_sigma", "price", "price_offset")))
        ended = em.feed(info, rew, term, trunc, done_mask_of=lambda i: ora.get_state(i).done_mask)
        if len(ended):
            ora.reset(mask=(term | trunc).astype(np.uint8))
    n_mod = 1 if opponents is None else 1 + len(opponents)
    assert_tables_equal(*keep["tables"], *em.table(module_of=keep["modules"], n_modules=n_mod), what="evaluate")
    env.close(); ora.close()


def test_evaluate_is_deterministic_and_greedy_ignores_the_sampling_seed():
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    N, A = 128, 4
    env = _env(N, A, 32)
    p = mlp.FusedPolicy("cuda:0", seed=5)
    r1 = evaluate(env, p, opponents=["random"], trained_slots=2, episodes=2, seed=3)
    r2 = evaluate(env, p, opponents=["random"], trained_slots=2, episodes=2, seed=3)
    assert r1["summary"] == r2["summary"]
    bufs = []
    for s in (1, 2):                                                   # the chains' sampling seed does not reach a greedy rollout
        env.reset(seed=40)
        roll = mlp.RolloutChains(env, p, 16, groups=2, seed=s, greedy=True)
        b = roll.run()
        torch.cuda.synchronize()
        bufs.append({k: v.cpu().clone() for k, v in b.items()})
    for k in bufs[0]:
        assert torch.equal(bufs[0][k], bufs[1][k]), k
    env.close()


_TRAINED = {}


def _trained_policy():
    """train_fused on the setup of test_hip_learning.py::test_fused_loop_improves_the_episode_return_and_tracks_the_float32_torch_loop (once per process)"""
    if "p" not in _TRAINED:
        from gym_continuousdoubleauction_amd import ppo
        env = _env(1024, 4, 32)
        _TRAINED["p"], _ = ppo.train_fused(env, iters=40, horizon=32, lr=3e-4, seed=0, log=lambda s: None)
        env.close()
    return _TRAINED["p"]


def test_a_trained_saved_and_loaded_policy_evaluates_bit_for_bit_as_the_one_in_memory(tmp_path):
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    trained = _trained_policy()
    path = str(tmp_path / "trained.pt")
    mlp.save_policy(path, trained)
    loaded = mlp.load_policy(path, "cuda:0")
    assert torch.equal(loaded.theta.cpu().view(torch.int32), trained.theta.cpu().view(torch.int32))
    assert torch.equal(loaded.wb.view(torch.int16), trained.wb.view(torch.int16))
    ev = _env(256, 4, 32)
    a = evaluate(ev, trained, episodes=2, seed=1)
    b = evaluate(ev, path, episodes=2, seed=1)
    assert a["summary"] == b["summary"] and a["nav_conservation_violations"] == 0
    ev.close()


@pytest.mark.xfail(strict=True, reason="measured on MI355X: the trained and the untrained policy's greedy episodes both end with every NAV at init_cash (return 0.0 over "
                                       "2048 agent-episodes each) - the mode actions trade nothing, so the greedy return does not separate them")
def test_the_trained_policy_greedy_return_is_above_the_untrained_one():
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    trained = _trained_policy()
    ev = _env(256, 4, 32)
    a = evaluate(ev, trained, episodes=2, seed=1)
    u = evaluate(ev, mlp.FusedPolicy("cuda:0", seed=0), episodes=2, seed=1)
    ev.close()
    assert a["modules"]["policy"]["episode_return_mean"] > u["modules"]["policy"]["episode_return_mean"], (a["modules"]["policy"], u["modules"]["policy"])


def test_a_saved_league_policy_evaluates_against_random_and_a_champion(tmp_path):
    import json
    import os
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    from gym_continuousdoubleauction_amd.league_train import save_league, train_league_fused
    env = _env(256, 4, 32)
    bank, league, _ = train_league_fused(env, iters=4, horizon=32, num_trainable=2, seed=0, std_dev_multiplier=-100.0, min_iterations_between_champions=1, log=lambda s: None)
    assert league.net_of, "no champion was promoted"
    save_league(str(tmp_path), bank, league)
    with open(tmp_path / "league.json") as fh:
        lj = json.load(fh)
    pol = os.path.join(str(tmp_path), lj["trainable"][0]["file"])
    champ = os.path.join(str(tmp_path), lj["champions"][0]["file"])
    N, A = 96, 4
    ev = _env(N, A, 32)
    for k in (1, 2):
        r = evaluate(ev, pol, opponents=["random", champ], trained_slots=k, episodes=2, seed=2)
        assert set(r["modules"]) == {"policy", "opponent_0", "opponent_1"} and r["nav_conservation_violations"] == 0
        mods = r["modules"]
        assert mods["policy"]["slots"] == N * k and mods["opponent_0"]["slots"] == mods["opponent_1"]["slots"] == (N // 2) * (A - k)
        assert mods["policy"]["agent_episodes"] == k * r["episodes"]
        assert sum(m["agent_episodes"] for m in mods.values()) == A * r["episodes"]
    env.close(); ev.close()
