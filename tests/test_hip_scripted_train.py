"""GPU: training against scripted opponents - the two new kernels (cda_league_assign_scripted against the host rule word for word, cda_gae_records_slots
against cda_gae_records_bootstrap bit for bit on the trained slots), the fused update's gradient over the leading slots of every row, and both loops end to
end: ppo.train_fused(trained_slots=, opponents=) and league_train.train_league_fused(scripted_opponents=), replayed through the CPU oracle, resumed, refused."""
import math
import os
import shutil

import numpy as np
import pytest
import torch

import scripted_train_util as ST

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCRIPTED = ["maker", "taker", "imbalance"]


# ---- assignment ---------------------------------------------------------------------------------------------------------------------------
def _pool(A, k, n_markets, scripted=True):
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd.league import LeagueSlotMapper
    m = LeagueSlotMapper(A, k, A - k, original_opponent_weight=1.0, champion_weight=3.0, scripted_weight=2.5)
    if scripted:
        for s in SCRIPTED:
            m.add_scripted(s)
    bank = mlp.PolicyBank(DEV, n_markets, A, k, max_frozen=2)
    net_of = {m.add_champion(): bank.snapshot(0) for _ in range(2)}
    return m, bank, net_of


@pytest.mark.parametrize("A,k", [(8, 2), (16, 1), (4, 3)])
@pytest.mark.parametrize("tag", ["assign-a", "assign-b"])
def test_assignment_with_scripted_pool_entries_equals_the_host_rule(A, k, tag):
    """N = 70 (no multiple of the 256-thread block), A - k random modules + maker, taker, imbalance + two champions with bank rows, weights 1.0 / 2.5 / 3.0.  The ids
    are a condition of the case: every pool class is drawn at least once (asserted with the numpy rule)."""
    N = 70
    ids = [f"{tag}-episode3-market{i}" for i in range(N)]
    m, bank, net_of = _pool(A, k, N)
    assert ST.classes_drawn(m, ids) == {"policy", "scripted", "champion"}
    want_net, want_script, want_pool = ST.host_assignment(m, ids, net_of)
    slot_script = torch.full((N, A), 9, dtype=torch.int32, device=DEV)
    slot_pool = torch.full((N, A), -7, dtype=torch.int32, device=DEV)
    bank.slot_net.fill_(77)
    m.assign_device(bank, episode_ids=ids, net_of=net_of, slot_pool=slot_pool, slot_script=slot_script)
    torch.cuda.synchronize()
    assert np.array_equal(bank.slot_net.cpu().numpy(), want_net)
    assert np.array_equal(slot_script.cpu().numpy(), want_script)
    assert np.array_equal(slot_pool.cpu().numpy(), want_pool)
    assert set(np.unique(want_script)) == {0, 1, 2, 3} and (want_script[:, :k] == 0).all() and (want_net[want_script != 0] == -1).all()
    # slot_pool may be NULL
    bank.slot_net.fill_(77); slot_script.fill_(9)
    m.assign_device(bank, episode_ids=ids, net_of=net_of, slot_script=slot_script)
    torch.cuda.synchronize()
    assert np.array_equal(bank.slot_net.cpu().numpy(), want_net) and np.array_equal(slot_script.cpu().numpy(), want_script)


@pytest.mark.parametrize("A,k", [(8, 2), (16, 1), (4, 3)])
def test_assignment_without_scripted_entries_equals_cda_league_assign(A, k):
    from gym_continuousdoubleauction_amd._lib import check, lib
    N = 70
    m, bank, net_of = _pool(A, k, N, scripted=False)
    for tag in ("assign-a", "assign-b"):
        ids = [f"{tag}-episode3-market{i}" for i in range(N)]
        sp0 = torch.full((N, A), -7, dtype=torch.int32, device=DEV)
        m.assign_device(bank, episode_ids=ids, net_of=net_of, slot_pool=sp0)
        torch.cuda.synchronize()
        sn0 = bank.slot_net.clone()
        crcs, cdf, nets = m._keep
        zeros = torch.zeros(len(m.pool()), dtype=torch.int32, device=DEV)
        sn1, ss1, sp1 = (torch.full((N, A), 5, dtype=torch.int32, device=DEV) for _ in range(3))
        check(lib().cda_league_assign_scripted(crcs.data_ptr(), N, A, k, cdf.data_ptr(), nets.data_ptr(), zeros.data_ptr(), len(m.pool()), sn1.data_ptr(), ss1.data_ptr(),
                                               sp1.data_ptr(), torch.cuda.current_stream().cuda_stream), "cda_league_assign_scripted")
        torch.cuda.synchronize()
        assert torch.equal(sn1, sn0) and torch.equal(sp1, sp0) and int(ss1.abs().sum()) == 0
        assert bool((sn0[:, k:] >= k).any()) and bool((sn0[:, k:] == -1).any())


# ---- GAE over the trained slots ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("capture_ends", [False, True])
def test_gae_over_the_trained_slots(k, capture_ends):
    """words 6, 7 of slots < k bit-equal to cda_gae_records_bootstrap(n_trainable = 0) on a copy of the same buffers, the other slots' words keep a sentinel, the
    sums are the float64 sums over the trained slots within tests/test_hip_league.py's bounds for this kernel, the count is T * N * k"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd._lib import check, lib
    N, A, T = 64, 4, 21
    env = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 8, "is_render": False, "auto_reset": True}, n_markets=N, with_info=False)
    env.reset(seed=7)
    roll = mlp.RolloutChains(env, mlp.FusedPolicy(DEV, seed=31), T, groups=2, seed=5, capture_ends=capture_ends)
    buf = roll.run()
    buf["record"].view(torch.int32)[..., 6] = 0x7fc0babe                                     # two NaN payloads nobody computes
    buf["record"].view(torch.int32)[..., 7] = 0x7fc0f00d
    ref = buf["record"].clone()
    rec, stats, count = roll.gae(gamma=0.97, lam=0.9, reward_scale=1e-3, n_slots=k)
    torch.cuda.synchronize()
    assert count == T * N * k and rec.data_ptr() == buf["record"].data_ptr()
    stats_ref = torch.zeros(2, dtype=torch.float64, device=DEV)
    fin = (buf["fin_index"].data_ptr(), roll.fin_value.data_ptr(), roll.fin_cap) if capture_ends else (None, None, 0)
    check(lib().cda_gae_records_bootstrap(buf["reward"].data_ptr(), buf["value"].data_ptr(), buf["terminated"].data_ptr(), buf["truncated"].data_ptr(), T, N, A, 0,
                                          1e-3, 0.97, 0.9, *fin, ref.data_ptr(), stats_ref.data_ptr(), torch.cuda.current_stream().cuda_stream), "cda_gae_records_bootstrap")
    torch.cuda.synchronize()
    got, want = buf["record"].view(torch.int32).cpu(), ref.view(torch.int32).cpu()
    assert bool(buf["truncated"].any()) and (not capture_ends or int(buf["fin_count"]) > 0)
    assert torch.equal(got[..., :k, :], want[..., :k, :])                                   # the trained slots: what the full launch writes there, bit for bit
    assert torch.equal(got[..., :6], want[..., :6])                                         # words 0 .. 5 of every record are not the kernel's
    assert bool((got[..., k:, 6] == 0x7fc0babe).all()) and bool((got[..., k:, 7] == 0x7fc0f00d).all())
    assert bool(torch.isfinite(buf["record"][..., :k, 6:]).all())
    a64 = buf["record"][..., :k, 6].double().cpu()
    st = stats.cpu()
    assert abs(float(st[0]) - float(a64.sum())) <= 1e-6 * float(a64.abs().sum()) and abs(float(st[1]) - float((a64 * a64).sum())) <= 1e-9 * float((a64 * a64).sum())
    env.close()


# ---- the update over the leading slots ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kl_coef,vf_clip", [(0.0, 0.0), (0.2, 0.7)])
def test_gradient_over_the_trained_slots_equals_float32_autograd(kl_coef, vf_clip):
    """a shared policy over the first 2 of 4 slots (FusedUpdate(policy, R, rows, 2), rec_stride = 32), the records of slots 2 and 3 NaN: update_check_util's
    checks and bands, every output and gradient finite"""
    cos, worst, ratios = ST.check_gradient_slots(4, 2, kl_coef, vf_clip)
    print(f"\nSLOTS-GRADIENT kl={kl_coef} vf_clip={vf_clip}: cos {cos:.6f}, worst block {worst:.4f}, {ratios}")


# ---- the shared loop ------------------------------------------------------------------------------------------------------------------------
S_CFG = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 16, "is_render": False, "auto_reset": True}
S_OPP = ["maker", "taker:p_trade_q32=1073741824"]
S_KW = dict(horizon=8, chains=2, trained_slots=2, seed=3)


def _shared_env(n=48):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    return CDAVecEnv(S_CFG, n_markets=n, with_info=False)


def _collector(keep, out):
    def log(_line):
        out.append(ST.snapshot_rollout(keep["rollout"]))
    return log


def test_shared_policy_trains_against_scripted_opponents():
    from gym_continuousdoubleauction_amd import ppo, scripted as S
    N, A, k, iters = 48, 4, 2, 3
    env = _shared_env(N)
    keep, rollouts = {}, []
    pol, hist = ppo.train_fused(env, iters=iters, opponents=S_OPP, keep=keep, log=_collector(keep, rollouts), **S_KW)
    assert not env.scripted and len(hist) == iters == len(rollouts)
    profiles = [S.parse_profile(o) for o in S_OPP]
    want_slots = S.opponent_slots(N, A, k, 2)
    assert all(np.array_equal(r["slots"], want_slots) for r in rollouts)
    # every rollout replays through the oracle; in the last one the scripted slots play the specification on the oracle's books
    acted = ST.replay_run(S_CFG, N, 3, rollouts, profiles, script_seed=3, base=0, check_scripts=(iters - 1,))
    assert len(acted) >= 3                                              # passes, market orders and quotes among them
    from gym_continuousdoubleauction_amd import mlp
    assert float(pol.adam_step.item()) == iters * 4 and bool(torch.isfinite(pol.theta).all())
    assert not torch.equal(pol.theta, mlp.FusedPolicy(DEV, seed=3).theta)
    assert keep["update"].A == k and keep["rollout"].trained_slots == k
    for h in hist:
        assert ST.finite({key: v for key, v in h.items() if key != "episode_metrics"}) and h["agent_steps"] == N * A * 8
        em = h["episode_metrics"]
        assert em["nav_conservation_violations"] == 0
    # the statistics are the trained slots': the last rollout's reward mean over slots 0, 1
    b = rollouts[-1]["b"]
    assert hist[-1]["mean_reward"] == pytest.approx(float(b["reward"][:, :, :k].mean()), rel=1e-12)
    assert hist[1]["episodes"] == N and hist[0]["episodes"] == 0        # max_step 16 = two rollouts: every market's episode ends in the second
    mods = hist[1]["episode_metrics"]["modules"]
    assert sorted(mods) == ["policy_0", "scripted_0_maker", "scripted_1_taker"]
    assert mods["policy_0"]["agent_episodes"] == N * k and mods["scripted_0_maker"]["agent_episodes"] + mods["scripted_1_taker"]["agent_episodes"] == N * (A - k)
    # the scripted slots' advantage / return words were never written (zero from the buffer's allocation), the trained ones were
    rec = keep["buffers"]["record"]
    assert bool((rec[..., k:, 6:] == 0).all()) and bool((rec[..., :k, 6] != 0).any())
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    _, bad = env.nav_conservation()
    assert not bad.any()
    env.close()


def test_shared_policy_trains_on_the_callers_own_scripts():
    """the caller attaches (profiles differing per market and slot) and passes trained_slots: the scripts stay attached afterwards"""
    from gym_continuousdoubleauction_amd import ppo
    N, A, k = 48, 4, 2
    env = _shared_env(N)
    slots = np.zeros((N, A), np.int32)
    slots[:, 2] = 1 + (np.arange(N) % 3)
    slots[:, 3] = 1 + ((np.arange(N) // 2) % 3)
    env.set_scripted(slots, ["maker", "imbalance", "pass"], seed=11)
    epoch = env.script_epoch
    pol, hist = ppo.train_fused(env, iters=1, log=lambda *_: None, **S_KW)
    assert env.scripted and env.script_epoch == epoch and float(pol.adam_step.item()) == 4
    assert sorted(hist[0]["episode_metrics"].get("modules", {})) == []          # (no episode has ended after 8 of 16 steps)
    env.close()


def _theta_and_bufs(pol_theta, keep):
    b = keep["buffers"]
    return pol_theta.clone(), {key: b[key].clone() for key in ("obs", "category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp", "value", "reward", "record")}


def test_shared_resume_is_exact(tmp_path):
    """four iterations straight against two + restore + two: theta and the last rollout's buffers bit for bit; another opponent list is refused"""
    from gym_continuousdoubleauction_amd import ppo
    quiet = dict(log=lambda *_: None, opponents=S_OPP, **S_KW)
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    keep_a, keep_b = {}, {}
    pol_a, hist_a = ppo.train_fused(_shared_env(), iters=4, keep=keep_a, checkpoint_dir=a_dir, chkpt_freq=2, **quiet)
    theta_a, bufs_a = _theta_and_bufs(pol_a.theta, keep_a)
    shutil.copytree(os.path.join(a_dir, "iter_2"), os.path.join(b_dir, "iter_2"))
    env_b = _shared_env()
    pol_b, hist_b = ppo.train_fused(env_b, iters=4, keep=keep_b, checkpoint_dir=b_dir, restore=True, **quiet)
    assert [h["iter"] for h in hist_b] == [2, 3] and not env_b.scripted
    theta_b, bufs_b = _theta_and_bufs(pol_b.theta, keep_b)
    for key in bufs_a:
        assert torch.equal(bufs_a[key].view(torch.uint8), bufs_b[key].view(torch.uint8)), key
    assert torch.equal(theta_a.view(torch.int32), theta_b.view(torch.int32))
    for kw, what in ((dict(opponents=["maker", "taker"], trained_slots=2), None),                     # the same profiles under another spelling: accepted
                     (dict(opponents=["maker", "taker:p_trade_q32=5"], trained_slots=2), "scripted_opponents"),
                     (dict(opponents=["maker"], trained_slots=2), "scripted_opponents"),
                     (dict(opponents=S_OPP, trained_slots=1), "trained_slots")):
        env = _shared_env()
        args = dict(dict(quiet, **kw), iters=4, checkpoint_dir=b_dir, restore=os.path.join(b_dir, "iter_2"), chkpt_freq=0)
        if what is None:
            ppo.train_fused(env, **dict(args, iters=2))                 # (the target is reached: nothing runs, nothing is refused)
        else:
            with pytest.raises(ValueError, match=what):
                ppo.train_fused(env, **args)
        assert not env.scripted
    with pytest.raises(ValueError, match="scripted_opponents"):            # ... and a run without opponents does not resume it either
        ppo.train_fused(_shared_env(), iters=4, log=lambda *_: None, horizon=8, chains=2, seed=3, checkpoint_dir=b_dir, restore=os.path.join(b_dir, "iter_2"))


# ---- the league loop ------------------------------------------------------------------------------------------------------------------------
L_CFG = {"num_of_agents": 8, "init_cash": 1000000, "max_step": 16, "is_render": False, "auto_reset": True}
L_KW = dict(horizon=8, num_trainable=2, chains=2, scripted_opponents=SCRIPTED, scripted_weight=2.5, max_champions=1, std_dev_multiplier=-10.0, seed=4, run_id="scr")


def _league_env(n=64):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    return CDAVecEnv(L_CFG, n_markets=n, with_info=False)


def test_league_draws_scripted_modules_per_episode(tmp_path):
    from gym_continuousdoubleauction_amd import scripted as S
    from gym_continuousdoubleauction_amd.league_train import save_league, train_league_fused
    N, A, k, iters = 64, 8, 2, 4
    env = _league_env(N)
    keep, rollouts, epochs, graphs = {}, [], [], []

    def log(_line):
        rollouts.append(ST.snapshot_rollout(keep["rollout"]))
        epochs.append(env.script_epoch)
        graphs.append(tuple(id(g) for g in keep["rollout"].graphs))
    bank, league, hist = train_league_fused(env, iters=iters, keep=keep, log=log, **L_KW)
    assert not env.scripted and len(hist) == iters
    m = league.mapper
    ids = ["scripted_0_maker", "scripted_1_taker", "scripted_2_imbalance"]
    assert m.available_modules[:k + (A - k) + 3] == [f"policy_{i}" for i in range(A)] + ids and m.pool()[-1].startswith("champion_")
    assert [h["promoted"] for h in hist] == [None, "champion_1", None, "champion_2"]
    # the last episode's draw (ids of episode 1, the pool as it stood then: champion_1 in its row) by the host rule, word for word
    from gym_continuousdoubleauction_amd.league import LeagueSlotMapper
    then = LeagueSlotMapper(A, k, A - k, 1.0, 3.0, scripted_weight=2.5)
    for s in SCRIPTED:
        then.add_scripted(s)
    then.add_champion("champion_1")
    want_net, want_script, want_pool = ST.host_assignment(then, [f"scr-episode1-market{i}" for i in range(N)], {"champion_1": k})
    assert np.array_equal(bank.slot_net.cpu().numpy(), want_net) and np.array_equal(keep["slot_pool"].cpu().numpy(), want_pool)
    assert np.array_equal(keep["slot_script"].cpu().numpy(), want_script) and np.array_equal(rollouts[-1]["slots"], want_script)
    assert bool((want_script != 0).any()) and bool((want_net[:, k:] == k).any()) and bool((want_net[:, k:] == -1).any())
    assert (rollouts[0]["slots"] != 0).any() and np.array_equal(rollouts[0]["slots"], rollouts[1]["slots"]) and not np.array_equal(rollouts[1]["slots"], rollouts[2]["slots"])
    # the rewrite of the slot table happened under ONE script epoch and the graphs captured in the first rollout
    assert len(set(epochs)) == 1 and len(set(graphs)) == 1 and keep["rollout"].graphs is not None
    for h in (hist[1], hist[3]):
        assert set(ids) <= set(h["module_returns"]) and set(ids) <= set(h["episode_metrics"]["modules"])
        assert all(math.isfinite(v) for v in h["module_returns"].values())
    assert all(h["episode_metrics"]["nav_conservation_violations"] == 0 for h in hist)
    for p in range(k):
        assert float(bank.policies[p].adam_step.item()) == iters * 4 and bool(torch.isfinite(bank.policies[p].theta).all())
    profiles = [S.parse_profile(s) for s in SCRIPTED]
    acted = ST.replay_run(L_CFG, N, 4, rollouts, profiles, script_seed=4, base=0, check_scripts=(iters - 1,))
    assert len(acted) >= 3
    lj = save_league(str(tmp_path / "league"), bank, league)
    assert [e["module"] for e in lj["scripted"]] == ids and lj["scripted"][1]["profile"] == S.profile_record("taker") and lj["scripted_weight"] == 2.5
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    _, bad = env.nav_conservation()
    assert not bad.any()
    env.close()


def test_league_pool_of_scripted_modules_only():
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    env = _league_env(32)
    keep = {}
    bank, league, hist = train_league_fused(env, iters=2, keep=keep, log=lambda *_: None, random_opponents=0, **dict(L_KW, max_champions=1, std_dev_multiplier=10.0))
    assert league.mapper.pool() == ["scripted_0_maker", "scripted_1_taker", "scripted_2_imbalance"] and not env.scripted
    ss = keep["slot_script"].cpu().numpy()
    assert (ss[:, :2] == 0).all() and (ss[:, 2:] >= 1).all() and set(np.unique(ss[:, 2:])) == {1, 2, 3} and bool((bank.slot_net[:, 2:] == -1).all())
    assert sorted(hist[1]["module_returns"]) == ["policy_0", "policy_1", "scripted_0_maker", "scripted_1_taker", "scripted_2_imbalance"]
    env.close()


def test_league_resume_is_exact(tmp_path):
    """max_step 16, horizon 8: an episode is two rollouts, chkpt_freq 2 a multiple of that.  Four iterations straight against two + restore + two."""
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    quiet = dict(log=lambda *_: None, **L_KW)
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    keep_a, keep_b = {}, {}
    bank_a, league_a, _ = train_league_fused(_league_env(), iters=4, keep=keep_a, checkpoint_dir=a_dir, chkpt_freq=2, **quiet)
    shutil.copytree(os.path.join(a_dir, "iter_2"), os.path.join(b_dir, "iter_2"))
    env_b = _league_env()
    bank_b, league_b, hist_b = train_league_fused(env_b, iters=4, keep=keep_b, checkpoint_dir=b_dir, restore=True, **quiet)
    assert [h["iter"] for h in hist_b] == [2, 3] and not env_b.scripted
    assert league_b.mapper.available_modules == league_a.mapper.available_modules and league_b.net_of == league_a.net_of
    assert torch.equal(keep_a["slot_pool"], keep_b["slot_pool"]) and torch.equal(keep_a["slot_script"], keep_b["slot_script"])
    for key in ("obs", "category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp", "value", "reward", "record"):
        assert torch.equal(keep_a["buffers"][key].view(torch.uint8), keep_b["buffers"][key].view(torch.uint8)), key
    assert torch.equal(bank_a.theta.view(torch.int32), bank_b.theta.view(torch.int32))
    ck = os.path.join(b_dir, "iter_2")
    for kw, what in ((dict(scripted_opponents=["maker", "taker"]), "scripted_opponents"), (dict(scripted_opponents=["taker", "maker", "imbalance"]), "scripted_opponents"),
                     (dict(scripted_weight=1.0), "scripted_weight"), (dict(scripted_opponents=None), "scripted")):
        env = _league_env()
        with pytest.raises(ValueError, match=what):
            train_league_fused(env, iters=4, checkpoint_dir=b_dir, restore=ck, **dict(quiet, **kw))
        assert not env.scripted


# ---- refusals on a real env -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gym_continuousdoubleauction_amd import mlp, ppo
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    N, A = 48, 4
    env = _shared_env(N)
    env.reset(seed=1)
    quiet = dict(iters=1, log=lambda *_: None, horizon=8, chains=2)
    good = np.tile(np.array([[0, 0, 1, 2]], np.int32), (N, 1))
    below, hole = good.copy(), good.copy()
    below[7, 1] = 2
    hole[9, 2] = 0
    env.set_scripted(good, ["maker", "taker"], seed=1)
    with pytest.raises(ValueError, match="scripted"):
        ppo.train_fused(env, **quiet)                                            # no slot count
    with pytest.raises(ValueError, match="scripted"):
        train_league_fused(env, **quiet)
    with pytest.raises(ValueError, match="scripted"):
        ppo.train_fused(env, opponents=["maker"], trained_slots=2, **quiet)      # its own scripts on top of the caller's
    for k in (0, 4, 5):
        with pytest.raises(ValueError, match="trained_slots"):
            ppo.train_fused(env, trained_slots=k, **quiet)
    with pytest.raises(ValueError, match="not scripted"):
        ppo.train_fused(env, trained_slots=1, **quiet)                           # slot 1 is at or above k = 1 and unscripted
    with pytest.raises(ValueError, match="trained slot"):
        ppo.train_fused(env, trained_slots=3, **quiet)                           # slot 2 is scripted and below k = 3
    with pytest.raises(ValueError, match="data-parallel"):
        ppo.train_fused(env, trained_slots=2, world=2, allreduce=lambda t: t, **quiet)
    # the shared-policy chains look at the placement once per script epoch: at construction, and again when the scripts changed
    pol = mlp.FusedPolicy(DEV, seed=1)
    chains = mlp.RolloutChains(env, pol, 4, groups=2, seed=5, trained_slots=2, use_graphs=False)
    chains.run()
    checked = chains._script_checked
    chains.run()
    assert chains._script_checked == checked == env.script_epoch
    env.set_scripted(hole, ["maker", "taker"], seed=1)
    with pytest.raises(ValueError, match="not scripted"):
        chains.run()
    with pytest.raises(ValueError, match="not scripted"):
        mlp.RolloutChains(env, pol, 4, groups=2, seed=5, trained_slots=2)
    env.set_scripted(below, ["maker", "taker"], seed=1)
    with pytest.raises(ValueError, match="trained slot"):
        mlp.RolloutChains(env, pol, 4, groups=2, seed=5, trained_slots=2)
    with pytest.raises(ValueError, match="trained_slots"):
        mlp.RolloutChains(env, pol, 4, groups=2, seed=5, trained_slots=4)
    with pytest.raises(ValueError, match="n_slots"):
        mlp.RolloutChains(env, pol, 4, groups=2, seed=5).gae(n_slots=5)
    env.clear_scripted()
    for kw, what in ((dict(trained_slots=0), "trained_slots"), (dict(trained_slots=4), "trained_slots"), (dict(trained_slots=2, world=2, allreduce=lambda t: t), "data-parallel")):
        with pytest.raises(ValueError, match=what):
            ppo.train_fused(env, opponents=["maker"], **dict(quiet, **kw))
        assert not env.scripted
    with pytest.raises(ValueError, match="data-parallel"):
        train_league_fused(env, scripted_opponents=["maker"], world=2, allreduce=lambda t: t, **quiet)
    assert not env.scripted
    # an exception inside the run still detaches what the loop attached
    with pytest.raises(ValueError, match="horizon"):
        train_league_fused(env, scripted_opponents=["maker"], iters=1, log=lambda *_: None, horizon=5)
    assert not env.scripted
    with pytest.raises(ValueError, match="multiples of 32"):
        ppo.train_fused(env, opponents=["maker"], trained_slots=2, iters=1, log=lambda *_: None, horizon=5)
    assert not env.scripted
    env.close()
