"""GPU: league self-play on the fused network kernels (include/cda_mlp.h `cda_league`, mlp.PolicyBank / RolloutChains, league_train.train_league_fused),
the episode-end capture with RLlib's time-limit bootstrap, the RLlib objective's extra loss terms (KL penalty, value-error clamp), and the episode record fed
from a fused rollout.  Reference: train/train.py:466-503, train/callbk/league_based_self_play_callback.py:1286-1344 (mapping fn), :780-1170 (champions),
train/model/model_handler.py:38-53 (RandomRLModule), train/episode_record.py:117-156, 197."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from update_check_util import _obs, check_gradient

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ACTION_KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset")


def _bank(N, A, k, frozen, seed=3, scale=2.0):
    """a bank whose nets all differ: k trainable + `frozen` snapshots, each with its own random parameters"""
    from gym_continuousdoubleauction_amd import mlp
    bank = mlp.PolicyBank(DEV, N, A, k, max_frozen=max(frozen, 1), seed=seed, random_seed=4242)
    for p in range(k):
        th = mlp.init_theta(generator=torch.Generator().manual_seed(seed + 100 * p))
        th[:mlp.OFF_LS] *= scale
        bank.policies[p].theta.copy_(th); bank.policies[p].pack()
    for f in range(frozen):
        row = bank.snapshot(0)
        th = mlp.init_theta(generator=torch.Generator().manual_seed(seed + 1000 + f))
        th[:mlp.OFF_LS] *= scale
        th[mlp.OFF_LS:] = torch.tensor([-0.3 - 0.1 * f, -0.7])
        bank.theta[row].copy_(th)
        pol = mlp.FusedPolicy(DEV, theta=th)                     # its packed operands, copied into the bank's row
        bank.wb[row].copy_(pol.wb)
    torch.cuda.synchronize()
    return bank


def test_device_assignment_equals_the_reference_mapping():
    """cda_league_assign (MT19937 + searchsorted on the device) against the golden cut from the reference's own get_mapping_fn, and against the numpy restatement"""
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd.league import LeagueSlotMapper
    with open(os.path.join(HERE, "golden", "league_mapping.json")) as fh:
        cases = json.load(fh)
    for c in cases:
        A, k = c["num_agents"], c["num_trainable"]
        if k < 1:
            continue
        N = len(c["episode_ids"])
        m = LeagueSlotMapper(A, k, c["num_fixed"], c["original_opponent_weight"], c["champion_weight"])
        bank = mlp.PolicyBank(DEV, N, A, k, max_frozen=max(1, len(c["champions"])))
        net_of = {}
        for ch in c["champions"]:
            m.add_champion(ch)
            net_of[ch] = bank.snapshot(0)
        slot_pool = torch.full((N, A), -7, dtype=torch.int32, device=DEV)
        m.assign_device(bank, episode_ids=c["episode_ids"], net_of=net_of, slot_pool=slot_pool)
        torch.cuda.synchronize()
        sp, sn = slot_pool.cpu().numpy(), bank.slot_net.cpu().numpy()
        names = np.array(m.available_modules, dtype=object)
        got = np.where(sp < 0, names[np.tile(np.arange(A), (N, 1))], names[np.minimum(np.maximum(sp, 0) + k, len(names) - 1)])
        assert got.tolist() == c["assignment"]
        want_net = np.array([[net_of.get(nm, -1) if a >= k else a for a, nm in enumerate(row)] for row in c["assignment"]])
        assert np.array_equal(sn, want_net)
        assert np.array_equal(np.where(sp < 0, np.arange(A)[None, :], sp + k), m.assign(c["episode_ids"]))     # the numpy restatement of the same rule
    # a larger batch against the numpy restatement alone
    m = LeagueSlotMapper(8, 2, 6, 1.0, 3.0)
    bank = mlp.PolicyBank(DEV, 3000, 8, 2, max_frozen=8)
    net_of = {m.add_champion(): bank.snapshot(1) for _ in range(5)}
    ids = [f"run-episode7-market{i}" for i in range(3000)]
    slot_pool = torch.zeros((3000, 8), dtype=torch.int32, device=DEV)
    m.assign_device(bank, episode_ids=ids, net_of=net_of, slot_pool=slot_pool)
    sp = slot_pool.cpu().numpy()
    assert np.array_equal(np.where(sp < 0, np.arange(8)[None, :], sp + 2), m.assign(ids))
    frac = float((bank.slot_net[:, 2:] >= 0).float().mean())          # 5 champions x 3 against 6 randoms x 1: 15 / 21
    assert abs(frac - 15 / 21) < 0.02, frac


def _league_step(bank, obs, A, seed, counter, draw, first=0, n=None, with_dist=True):
    from gym_continuousdoubleauction_amd._lib import lib, check
    N = obs.shape[0]
    n = N - first if n is None else n
    k = bank.n_trainable
    e = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)             # noqa: E731
    o = {"category": e((N, A), torch.int32), "size_mean": e((N, A), torch.float32), "size_sigma": e((N, A), torch.float32), "price": e((N, A), torch.int32),
         "price_offset": e((N, A), torch.int32), "a_cont": e((N, A, 2), torch.float32), "logp": e((N, A), torch.float32), "value": e((k, N), torch.float32),
         "rec": e((N, A, 8), torch.float32), "dist": e((k, N, 28), torch.float32)}
    check(lib().cda_mlp_league_step(C.byref(bank.struct()), obs.data_ptr(), first, n, A, seed, counter.data_ptr(), draw,
                                    *[o[key].data_ptr() for key in (*ACTION_KEYS, "a_cont", "logp", "value")], N, o["rec"].data_ptr(),
                                    o["dist"].data_ptr() if with_dist else None, N * 28, torch.cuda.current_stream().cuda_stream), "cda_mlp_league_step")
    torch.cuda.synchronize()
    return o


def test_league_step_routes_every_slot_to_its_module():
    """One launch serves every module: a slot played by net n gets bit for bit what cda_mlp_policy_step with n's parameters gives it (trainable or frozen), a random
    slot the counter-based uniform law, the trainable nets' values and distributions are their own."""
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd._lib import lib, check
    N, A, k, F = 300, 8, 2, 3
    bank = _bank(N, A, k, F)
    g = torch.Generator().manual_seed(9)
    sn = torch.randint(-1, k + F, (N, A), generator=g, dtype=torch.int32)
    sn[:, 0], sn[:, 1] = 0, 1
    sn[64:96, 2:] = -1                                        # a whole 32-row tile without any frozen net: those workgroups leave early
    bank.set_slots(sn)
    obs = _obs(N, seed=31).to(DEV)
    counter = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    o = _league_step(bank, obs, A, 77, counter, 3)
    snc = sn.numpy()
    for n in range(k + F):
        pol = mlp.FusedPolicy(DEV, theta=bank.theta[n].cpu())
        assert torch.equal(pol.wb, bank.wb[n])
        ref = pol.policy_step(obs, A, seed=77, counter=counter, draw=3)
        torch.cuda.synchronize()
        mask = torch.from_numpy(snc == n)
        assert int(mask.sum()) > 50
        for key in (*ACTION_KEYS, "logp"):
            assert torch.equal(o[key].cpu()[mask], ref[key].cpu()[mask]), (n, key)
        assert torch.equal(o["a_cont"].cpu()[mask], ref["a_cont"].cpu()[mask])
        if n < k:
            assert torch.equal(o["value"][n].cpu(), ref["value"].cpu())
            out = pol.forward(obs).cpu().double()
            want = torch.cat([torch.log_softmax(out[:, :9], -1), torch.log_softmax(out[:, 9:19], -1), torch.log_softmax(out[:, 19:22], -1), out[:, 22:24],
                              pol.log_std.cpu().double().expand(N, 2), torch.zeros(N, 2, dtype=torch.float64)], dim=1)      # ... | the log-stds sampled with | 2 zeros
            assert (o["dist"][n].cpu().double() - want).abs().max() <= 2e-5
    # the records carry the same words
    rec = o["rec"].cpu()
    for w, key in enumerate(("category", "price", "price_offset")):
        assert torch.equal(rec[..., w].contiguous().view(torch.int32), o[key].cpu())
    net_mask = torch.from_numpy(snc >= 0)
    assert torch.equal(rec[..., 3:5][net_mask], o["a_cont"].cpu()[net_mask]) and torch.equal(rec[..., 5][net_mask], o["logp"].cpu()[net_mask])
    # random slots: the stream of include/cda_random_agents.h keyed (random_seed + counter x golden ratio, market, step = draw, slot) - the host side of the same header
    rs = (bank.random_seed + 5 * 0x9e3779b97f4a7c15) & (2 ** 64 - 1)
    cat, price, off = (np.zeros((N, A), np.int32) for _ in range(3))
    mean, sigma = (np.zeros((N, A), np.float32) for _ in range(2))
    check(lib().cda_random_actions_host(rs, 0, 3, N, A, cat.ctypes.data, mean.ctypes.data, sigma.ctypes.data, price.ctypes.data, off.ctypes.data), "cda_random_actions_host")
    rmask = snc < 0
    for key, want in zip(ACTION_KEYS, (cat, mean, sigma, price, off)):
        assert np.array_equal(o[key].cpu().numpy()[rmask], want[rmask]), key
    assert (o["logp"].cpu().numpy()[rmask] == 0).all() and (o["a_cont"].cpu().numpy()[rmask] == 0).all()
    # a sub-range leaves the rest alone
    part = _league_step(bank, obs, A, 77, counter, 3, first=64, n=100)
    for key in (*ACTION_KEYS, "logp"):
        assert torch.equal(part[key][64:164], o[key][64:164]) and (part[key][:64] == 0).all() and (part[key][164:] == 0).all(), key
    assert torch.equal(part["value"][:, 64:164], o["value"][:, 64:164])


def test_random_slots_follow_the_uniform_law():
    """RandomRLModule's law (model_handler.py:38-53): category U{0..8}, price U{0..9}, price_offset U{0..2}, size_mean U[-1, 1), size_sigma U[0, 1)"""
    N, A, k = 4096, 8, 2
    bank = _bank(N, A, k, 0)
    obs = _obs(N, seed=2).to(DEV)
    counter = torch.ones(1, dtype=torch.int64, device=DEV)
    seen = []
    for draw in (0, 1):
        o = _league_step(bank, obs, A, 1, counter, draw, with_dist=False)
        cat, price, off = (o[key][:, k:].cpu().numpy().reshape(-1) for key in ("category", "price", "price_offset"))
        mean, sigma = o["size_mean"][:, k:].cpu().numpy().reshape(-1), o["size_sigma"][:, k:].cpu().numpy().reshape(-1)
        n = cat.size
        for x, m in ((cat, 9), (price, 10), (off, 3)):
            f = np.bincount(x, minlength=m) / n
            assert x.min() == 0 and x.max() == m - 1 and np.abs(f - 1 / m).max() < 4 * math.sqrt((1 / m) * (1 - 1 / m) / n), (m, f)
        assert -1 <= mean.min() and mean.max() < 1 and abs(mean.mean()) < 0.02 and abs(mean.std() - 2 / math.sqrt(12)) < 0.012
        assert 0 <= sigma.min() and sigma.max() < 1 and abs(sigma.mean() - 0.5) < 0.01 and abs(sigma.std() - 1 / math.sqrt(12)) < 0.01
        seen.append(cat.copy())
    assert not np.array_equal(seen[0], seen[1])                 # another step, other draws


def _replay(cfg, N, seed, b, T, with_fin=None):
    """the rollout's recorded actions through the CPU oracle (resetting where the env reset itself): obs / reward / flags bit for bit; returns the oracle's
    last observations [(t, market)] of the episodes that ended"""
    import oracle_lib as O
    ora = O.OracleEnv({key: v for key, v in cfg.items() if key != "auto_reset"}, N)
    o0 = ora.reset(seeds=(seed + np.arange(N)).astype(np.uint64))
    assert np.array_equal(b["obs"][0].numpy().view(np.uint32), o0.view(np.uint32))
    finals = {}
    for t in range(T):
        oo, orw, ot, otr, _ = ora.step(*[b[key][t].numpy() for key in ACTION_KEYS])
        assert np.array_equal(b["reward"][t].numpy().view(np.uint64), orw.view(np.uint64)), t
        assert np.array_equal(b["terminated"][t].numpy(), ot) and np.array_equal(b["truncated"][t].numpy(), otr), t
        done = (ot | otr).astype(bool)
        for j in np.nonzero(done)[0]:
            finals[(t, int(j))] = oo[j].copy()
        if done.any():
            oo = ora.reset(mask=done.astype(np.uint8)).copy()
        assert np.array_equal(b["obs"][t + 1].numpy().view(np.uint32), oo.view(np.uint32)), t
    ora.close()
    return finals


@pytest.mark.parametrize("groups,use_graphs", [(1, False), (1, True), (3, True)])
def test_league_rollout_replays_through_the_oracle(groups, use_graphs):
    """A league rollout as independent chains: the recorded actions of ALL slots (trainable, frozen, random) replayed through the CPU oracle reproduce the recorded
    observations and rewards bit for bit; every step's record is what a single league step on that step's observation gives; episode ends are captured."""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    N, A, k, F, T = 96, 8, 2, 2, 14
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 10, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    bank = _bank(N, A, k, F, seed=11, scale=1.0)
    sn = torch.randint(-1, k + F, (N, A), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    sn[:, 0], sn[:, 1] = 0, 1
    bank.set_slots(sn)
    env.reset(seed=500)
    roll = mlp.RolloutChains(env, bank, T, groups=groups, seed=99, use_graphs=use_graphs, capture_ends=True, with_dist=True)
    for rnd in range(2):
        buf = roll.run()
        torch.cuda.synchronize()
        b = {key: v.cpu() for key, v in buf.items()}
        if rnd == 0:
            finals = _replay(cfg, N, 500, b, T)
            # episode-end capture: every (t, market) that ended has a slot, its observation is the oracle's last one of that episode; nothing else has one
            fi = b["fin_index"].numpy()
            ended = (b["terminated"] | b["truncated"]).numpy().astype(bool)
            assert np.array_equal(fi >= 0, ended) and int(b["fin_count"]) == int(ended.sum()) == N and len(finals) == N
            assert sorted(fi[ended].tolist()) == list(range(N))
            for (t, j), want in finals.items():
                assert np.array_equal(b["fin_obs"][fi[t, j]].numpy().view(np.uint32), want.view(np.uint32)), (t, j)
        cnt = roll.counter.clone()
        for t in (0, T // 2, T - 1):
            o = _league_step(bank, buf["obs"][t], A, 99, cnt, t)
            for key in (*ACTION_KEYS, "a_cont", "logp"):
                assert torch.equal(o[key].cpu(), b[key][t]), (key, t)
            assert torch.equal(o["value"].cpu(), b["value"][:, t]) and torch.equal(o["rec"].cpu()[..., :6], b["record"][t][..., :6])
            assert torch.equal(o["dist"].cpu(), b["dist"][:, t])
        for p in range(k):
            assert torch.equal(bank.policies[p].forward(buf["obs"][T])[:, 24].cpu(), b["value"][p, T])
        assert torch.equal(roll.log_std_old.cpu(), bank.theta[:k, mlp.OFF_LS:].cpu())
    assert (roll.graphs is not None) == use_graphs                # (one chain on the default stream: captured on a side stream, not a silent fall-back to direct launches)
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    env.close()


def _gae_reference(rew, val, last_val, term, trunc, fin_val, gamma, lam):
    """ppo.gae's recursion with RLlib's time-limit bootstrap: rew / val [T, B], term / trunc [T, B] bool, fin_val [T, B] = V(last observation) where truncated"""
    T = rew.shape[0]
    adv = torch.zeros_like(rew)
    nxt, run = last_val.clone(), torch.zeros_like(last_val)
    for t in range(T - 1, -1, -1):
        done = term[t] | trunc[t]
        nd = (~done).float()
        boot = torch.where(trunc[t] & ~term[t], fin_val[t], torch.zeros_like(nxt))
        delta = rew[t] + gamma * (nxt * nd + boot) - val[t]
        run = delta + gamma * lam * nd * run
        adv[t] = run
        nxt = val[t]
    return adv, adv + val


@pytest.mark.parametrize("league", [False, True])
def test_gae_bootstraps_truncations_with_the_value_of_the_captured_observation(league):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    N, A, T, k = 64, 4, 21, 2
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 8, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    pol = _bank(N, A, k, 0, seed=21, scale=1.0) if league else mlp.FusedPolicy(DEV, seed=31)
    env.reset(seed=7)
    roll = mlp.RolloutChains(env, pol, T, groups=2, seed=5, capture_ends=True)
    buf = roll.run()
    rec, stats, count = roll.gae(gamma=0.97, lam=0.9, reward_scale=1e-3)
    torch.cuda.synchronize()
    b = {key: v.cpu() for key, v in buf.items()}
    term, trunc = b["terminated"].bool(), b["truncated"].bool()
    assert bool(trunc.any()) and int(b["fin_count"]) == int((term | trunc).sum())
    fi = b["fin_index"].long()
    r4 = b["record"]
    for p in range(k if league else 1):
        net = pol.policies[p] if league else pol
        fin_v = net.forward(buf["fin_obs"])[:, 24].cpu()
        assert torch.equal(fin_v[:int(b["fin_count"])], roll.fin_value[p].cpu()[:int(b["fin_count"])])
        fv = torch.where(fi >= 0, fin_v[fi.clamp(min=0)], torch.zeros(T, N))
        value = b["value"][p] if league else b["value"]
        slots = [p] if league else list(range(A))
        for a in slots:
            rew = b["reward"][:, :, a].float() * 1e-3
            adv, ret = _gae_reference(rew, value[:T], value[T], term, trunc, fv, 0.97, 0.9)
            assert torch.allclose(r4[..., a, 6], adv, rtol=1e-5, atol=1e-6) and torch.allclose(r4[..., a, 7], ret, rtol=1e-5, atol=1e-6), (p, a)
        a64 = r4[..., slots, 6].double()
        st = stats[p] if league else stats
        assert abs(float(st[0]) - float(a64.sum())) <= 1e-6 * float(a64.abs().sum()) and abs(float(st[1]) - float((a64 * a64).sum())) <= 1e-9 * float((a64 * a64).sum())
    if league:
        assert count == T * N and (r4[..., k:, 6:] == 0).all()       # the other slots' records feed no update
    env.close()


@pytest.mark.parametrize("A,slot,kl_coef,vf_clip", [(8, 1, 0.0, 0.0),       # a league update: only slot 1's samples of 8 feed the gradient
                                                    (4, None, 0.2, 0.7),     # one shared policy with RLlib's KL penalty and value clamp
                                                    (8, 0, 0.3, 0.5)])       # both
def test_masked_and_rllib_objective_gradient_equals_float32_autograd(A, slot, kl_coef, vf_clip):
    """The fused update's gradient - record stride selecting ONE slot per row (league), KL(old || new) exact per row, clamped value error - against loss.backward()
    through ppo.ActorCritic in float32 on the selected samples only."""
    check_gradient(A, slot, kl_coef, vf_clip)


@pytest.mark.parametrize("A,slot,kl_coef,vf_clip", [(4, None, 0.0, 0.0),     # one shared policy, plain PPO objective
                                                    (4, None, 0.2, 0.7),     # ... RLlib's objective: the KL's Gaussian part with per-row log-stds on both sides
                                                    (8, 1, 0.3, 0.5)])       # a league update
def test_state_dependent_log_std_head_gradient_equals_float32_autograd(A, slot, kl_coef, vf_clip):
    """RLlib's default module for Box actions (the reference's PPO modules, train/policy/policy_handler.py:69-76): the policy network emits two log-stds per row.  Output
    rows 25, 26 of the fused network are that head (offsets on top of the free vector): the loss scores every sample with its ROW's log-stds, sends d loss / d log_std of
    every row back through columns 25, 26, rows 25, 26 of Wo / bo get their gradient, the free vector none - against float64 autograd on the kernel's own outputs and
    float32 autograd through ppo.ActorCritic(state_dependent_log_std=True)."""
    check_gradient(A, slot, kl_coef, vf_clip, sd=True)


def test_fused_league_training_runs_the_reference_topology():
    """8 agents, 2 separately trained policies, pool of random modules + champions, two iterations per episode: steps counted, champions promoted through the
    reference's rule, the rollout graphs re-captured when a snapshot joins, opponents re-drawn at the episode boundary only, env invariants clean."""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    N, A, k = 256, 8, 2
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 32, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    logs, keep = [], {}
    bank, league, hist = train_league_fused(env, iters=6, horizon=16, num_trainable=k, min_iterations_between_champions=2, std_dev_multiplier=-10.0,
                                            log=logs.append, keep=keep, max_champions=2)
    assert len(hist) == 6
    for h in hist:
        for p in range(k):
            assert all(math.isfinite(v) for v in h[f"policy_{p}"].values())
    for p in range(k):
        assert float(bank.policies[p].adam_step.item()) == 6 * 4          # iterations x epochs (one minibatch per epoch)
        assert torch.isfinite(bank.policies[p].theta).all()
    assert not torch.equal(bank.policies[0].theta, bank.policies[1].theta)
    # std_dev_multiplier -10: the best trainable policy always clears the threshold, so the cooldown and the rolling window decide: promotions after
    # iterations 1, 3, 5 (episodes end every second iteration), the third one evicting champion_1
    assert [h["promoted"] for h in hist] == [None, "champion_1", None, "champion_2", None, "champion_3"]
    assert league.mapper.pool()[-2:] == ["champion_2", "champion_3"] and set(league.net_of) == {"champion_2", "champion_3"} and bank.n_frozen == 2
    assert keep["rollout"].graphs is not None                   # the rollout stayed on its captured graphs while champions joined (the launch grid covers the bank's capacity)
    assert "module_returns" in hist[1] and "policy_0" in hist[1]["module_returns"] and "module_returns" not in hist[0]
    sn = bank.slot_net.cpu()
    assert (sn[:, 0] == 0).all() and (sn[:, 1] == 1).all() and int(sn.max()) <= 3 and bool((sn[:, 2:] >= 2).any()) and bool((sn[:, 2:] == -1).any())
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    _, bad = env.nav_conservation()
    assert not bad.any()
    env.close()


def test_record_from_a_fused_rollout_equals_the_oracle_replayed_record(tmp_path):
    """Episode record straight from the rollout buffers (no per-step host call): the last S markets run as a chain with the info tensors; the Parquet rows equal the
    rows recorded step by step from the CPU oracle replaying the same actions (resets included), the schema is the reference recorder's, and the reference's
    NAV-conservation check holds at every episode end."""
    import pyarrow.parquet as pq
    import oracle_lib as O
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd.episode_record import BatchedEpisodeRecorder, schema
    N, A, T, S = 80, 4, 12, 3
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 9, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    pol = mlp.FusedPolicy(DEV, seed=3)
    env.reset(seed=900)
    roll = mlp.RolloutChains(env, pol, T, groups=2, seed=8, capture_ends=True, info_markets=S)
    rec = BatchedEpisodeRecorder(str(tmp_path / "fused"), num_agents=A, markets=range(N - S, N), run_id="t", rows_per_file=10 ** 9)
    rec.init_cash = 1000000
    rec.module_namer = lambda m: [f"policy_{a}" for a in range(A)]
    ref = BatchedEpisodeRecorder(str(tmp_path / "oracle"), num_agents=A, markets=range(N - S, N), run_id="t", rows_per_file=10 ** 9)
    ora = O.OracleEnv({key: v for key, v in cfg.items() if key != "auto_reset"}, N)
    ora.reset(seeds=(900 + np.arange(N)).astype(np.uint64))
    ordinal, t_in = 0, 0
    name = lambda e: [f"market{m}-episode{e}" for m in range(N - S, N)]      # noqa: E731
    ref.begin_episodes(name(0), module_ids=[[f"policy_{a}" for a in range(A)]] * S)
    for rnd in range(2):
        buf = roll.run()
        torch.cuda.synchronize()
        rec.record_rollout(roll, iteration=rnd)
        b = {key: v.cpu() for key, v in buf.items() if key in ACTION_KEYS}
        for t in range(T):
            acts = [b[key][t].numpy() for key in ACTION_KEYS]
            oo, orw, ot, otr, oi = ora.step(*acts)
            ref.iteration = rnd
            ref.record_step(oo, orw, oi, acts, step_index=t_in)
            t_in += 1
            done = (ot | otr).astype(bool)
            if done[N - S:].any():
                ref.finish(complete=True)
                ordinal += 1; t_in = 0
                ref.begin_episodes(name(ordinal), module_ids=[[f"policy_{a}" for a in range(A)]] * S)
            if done.any():
                ora.reset(mask=done.astype(np.uint8))
    got, want = pq.read_table(rec.close()), pq.read_table(ref.close())
    assert got.schema.equals(schema()) and got.schema.equals(pq.read_schema(os.path.join(HERE, "golden", "episode_record_ref.parquet")))
    assert got.num_rows == want.num_rows == 2 * T * S * A
    for col in want.schema.names:
        if col in ("wall_time",):
            continue
        g, w = got.column(col).to_pylist(), want.column(col).to_pylist()
        for i, (x, y) in enumerate(zip(g, w)):
            if isinstance(y, float):
                assert x is not None and np.float64(x).tobytes() == np.float64(y).tobytes(), (col, i, x, y)
            elif isinstance(y, list):
                assert np.array_equal(np.asarray(x, np.float64).view(np.uint64), np.asarray(y, np.float64).view(np.uint64)), (col, i)
            else:
                assert x == y, (col, i, x, y)
    assert rec.nav_checked == 2 * S and rec.nav_violations == 0      # 24 steps of 9-step episodes: two ends per recorded market
    # the rows of an unfinished episode are flagged
    assert got.to_pandas().groupby("episode_id")["episode_complete"].first().tolist().count(False) == S
    ora.close(); env.close()


def test_league_training_records_sampled_episodes_with_module_ids(tmp_path):
    """train_league_fused(recorder=..., info_markets=S): the sampled chain's episodes land in the reference's Parquet schema with the module that played each slot
    (the league's draw), one file per flush, the callback's NAV check at every episode end."""
    import pyarrow.parquet as pq
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd.episode_record import BatchedEpisodeRecorder, schema
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    N, A, S, T = 128, 8, 2, 16
    env = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": T, "is_render": False, "auto_reset": True}, n_markets=N, with_info=False)
    rec = BatchedEpisodeRecorder(str(tmp_path), num_agents=A, markets=range(N - S, N), run_id="lg")
    bank, league, hist = train_league_fused(env, iters=3, horizon=T, num_trainable=2, std_dev_multiplier=-10.0, log=lambda s: None, recorder=rec, info_markets=S, run_id="lg")
    path = rec.close()
    t = pq.read_table(path)
    assert t.schema.equals(schema()) and t.num_rows == 3 * S * T * A
    df = t.to_pandas()
    assert set(df["episode_id"]) == {f"lg-episode{e}-market{m}" for e in range(3) for m in (N - 2, N - 1)}
    assert (df[df.agent_id == "agent_0"]["module_id"] == "policy_0").all() and (df[df.agent_id == "agent_1"]["module_id"] == "policy_1").all()
    pool = df[~df.agent_id.isin(["agent_0", "agent_1"])]["module_id"]
    assert pool.str.match(r"^(policy_[2-7]|champion_\d+)$").all() and df["episode_complete"].all()
    assert rec.nav_checked == 3 * S and rec.nav_violations == 0
    # a module id is constant over an episode's rows of one agent, and the champions that were promoted can appear from the episode after their promotion only
    assert (df.groupby(["episode_id", "agent_id"])["module_id"].nunique() == 1).all()
    assert not df[df.episode_id.str.contains("episode0")]["module_id"].str.startswith("champion").any()
    env.close()


def test_every_slot_trainable_is_independent_learners():
    """num_trainable == num_agents: no pool, no draws - four separately trained policies, one per slot, each updated from its own slot's records"""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    N, A = 128, 4
    env = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 16, "is_render": False, "auto_reset": True}, n_markets=N, with_info=False)
    bank, league, hist = train_league_fused(env, iters=2, horizon=16, num_trainable=A, max_champions=4, min_iterations_between_champions=1, std_dev_multiplier=-10.0, log=lambda s: None)
    assert bank.n_trainable == A and all(float(p.adam_step.item()) == 2 * 4 for p in bank.policies)
    th = [p.theta.cpu() for p in bank.policies]
    assert all(torch.isfinite(t).all() for t in th) and all(not torch.equal(th[0], t) for t in th[1:])
    assert set(hist[-1]["module_returns"]) == {f"policy_{a}" for a in range(A)}
    assert (bank.slot_net.cpu() == torch.arange(A, dtype=torch.int32)).all()          # champions exist (the rule promoted one per iteration) but no slot ever draws one
    assert len(league.history) == 2 and (env.flags() == 0).all()
    env.close()


@pytest.mark.parametrize("league", [False, True])
def test_a_host_side_reset_between_rollouts_is_where_the_next_rollout_starts(league):
    """RolloutChains carries the last observation from rollout to rollout (the chains never write env.obs); when the markets are reset or stepped from the HOST in
    between (env.host_epoch), the next rollout starts from the env's own observation tensor - and replays through the oracle from that reset."""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    N, A, T = 64, 4, 9
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    actor = _bank(N, A, 2, 1, seed=5, scale=1.0) if league else mlp.FusedPolicy(DEV, seed=3)
    env.reset(seed=700)
    roll = mlp.RolloutChains(env, actor, T, groups=2, seed=17)
    b0 = {key: v.cpu().clone() for key, v in roll.run().items() if torch.is_tensor(v)}
    _replay(cfg, N, 700, b0, T)
    b1 = {key: v.cpu().clone() for key, v in roll.run().items() if torch.is_tensor(v)}          # no host call in between: continues where the first one ended
    assert torch.equal(b1["obs"][0], b0["obs"][T])
    first = env.reset(seed=9000).clone()
    b2 = {key: v.cpu().clone() for key, v in roll.run().items() if torch.is_tensor(v)}
    assert torch.equal(b2["obs"][0], first.cpu()) and not torch.equal(b2["obs"][0], b1["obs"][T])
    _replay(cfg, N, 9000, b2, T)
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    env.close()


def test_league_loop_trains_the_state_dependent_log_std_heads_of_both_policies():
    """train_league_fused(state_dependent_log_std=True) under RLLIB_DEFAULTS (KL rows with per-row log-stds): three iterations at 128 x 8 - losses finite, KL measured, the two
    trainable policies' head rows (25, 26 of Wo / bo) moved, their free log_std vectors did not, champions snapshot the head with the row, env invariants clean."""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp, ppo
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    N, A, k = 128, 8, 2
    env = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 16, "is_render": False, "auto_reset": True}, n_markets=N, with_info=False)
    keep = {}
    bank, league, hist = train_league_fused(env, iters=3, horizon=16, num_trainable=k, lr=3e-4, objective=dict(ppo.RLLIB_DEFAULTS), state_dependent_log_std=True,
                                            std_dev_multiplier=-10.0, min_iterations_between_champions=1, log=lambda s: None, keep=keep)
    L = mlp.layout(4)
    for p in range(k):
        pol = bank.policies[p]
        assert pol.state_dependent_log_std and mlp.has_log_std_head(pol.theta.cpu())
        fresh = mlp.init_theta(generator=torch.Generator().manual_seed(0 + 7919 * p), state_dependent_log_std=True)
        wo_now, wo_0 = pol.theta[L.OFF_WO:L.OFF_BO].view(32, 256).cpu(), fresh[L.OFF_WO:L.OFF_BO].view(32, 256)
        assert float((wo_now[25:27] - wo_0[25:27]).abs().max()) > 1e-5          # the head trained
        assert float(wo_now[27:].abs().max()) == 0.0                            # the padding rows stayed zero
        assert torch.equal(pol.theta[L.OFF_LS:].cpu(), fresh[L.OFF_LS:])          # the free vector is not an optimisation variable with the head
        for h in hist:
            assert all(math.isfinite(v) for v in h[f"policy_{p}"].values()) and h[f"policy_{p}"]["kl"] > 0
    assert len(league.history) >= 1 and mlp.has_log_std_head(bank.theta[k].cpu())     # a champion is a copy of the whole row, head included
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    env.close()
