"""GPU: the one-launch rollout step of every network that is not the default one (include/cda.h cda_net_step_range, csrc/cda_kernels.inc k_net_step: the policy
evaluated INSIDE the step kernel, the hidden activation and the trunk read from the kernel's arguments) against the two launches it replaces - that network's
cda_mlp_policy_step (k_mlp_fwd<SAMPLE> of the _relu / _elu / _linear / _vfs object) followed by cda_step_range_capture (k_step) - bit for bit; its refusals; the
rollout chains that now take it; and a training run over both paths."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DEV = "cuda:0"
KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset")
ACTS = ("tanh", "relu", "elu", "linear")          # mlp.ACTIVATIONS: the index is the kernel's code


def _bufs(N, A, cap, obs_dim=168):
    e = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)          # noqa: E731
    return {"category": e((N, A), torch.int32), "size_mean": e((N, A), torch.float32), "size_sigma": e((N, A), torch.float32), "price": e((N, A), torch.int32),
            "price_offset": e((N, A), torch.int32), "a_cont": e((N, A, 2), torch.float32), "logp": e((N, A), torch.float32), "value": e((N,), torch.float32),
            "rec": e((N, A, 8), torch.float32), "dist": e((N, 28), torch.float32), "obs": e((N, obs_dim), torch.float32), "reward": e((N, A), torch.float64),
            "term": e((N,), torch.uint8), "trunc": e((N,), torch.uint8), "fin_obs": e((cap, obs_dim), torch.float32), "fin_count": e((1,), torch.int32),
            "fin_index": torch.full((N,), -1, dtype=torch.int32, device=DEV)}


def _net_step(L, env, act, vfs, first, n, p, obs, seed, counter, t, b, cap, st):
    return L.cda_net_step_range(env._h, act, vfs, first, n, p.wb.data_ptr(), p.theta.data_ptr(), obs.data_ptr(), seed, counter.data_ptr(), t,
                                *[b[k].data_ptr() for k in KEYS], b["a_cont"].data_ptr(), b["logp"].data_ptr(), b["value"].data_ptr(), b["rec"].data_ptr(),
                                b["dist"].data_ptr(), b["obs"].data_ptr(), b["reward"].data_ptr(), b["term"].data_ptr(), b["trunc"].data_ptr(),
                                b["fin_obs"].data_ptr(), cap, b["fin_count"].data_ptr(), b["fin_index"].data_ptr(), st)


# (activation, shared trunk, agents, markets, max_step, cash, deep book, n_hist, state-dependent log-std head, episode metrics)
# every (activation, trunk) pair but the default's at depth 4; every other compiled depth once with each trunk; the log-std head with each trunk; 2, 3, 4 and 8 agents;
# one deep-book case on a shared trunk; one pair with the tallying instances
CASES = [("relu", 0, 4, 150, 7, 1000000, False, 4, False, False), ("elu", 0, 8, 70, 5, 20000, False, 4, False, False), ("linear", 0, 2, 33, 6, 1000000, False, 4, False, False),
         ("tanh", 1, 4, 150, 7, 1000000, False, 4, True, False), ("relu", 1, 4, 40, 4096, 1000000, True, 4, False, False), ("elu", 1, 3, 45, 5, 1000000, False, 4, False, False),
         ("linear", 1, 8, 50, 9, 20000, False, 4, False, False),
         ("relu", 0, 4, 70, 6, 1000000, False, 1, False, False), ("elu", 1, 4, 70, 6, 1000000, False, 1, False, True),
         ("elu", 0, 8, 50, 9, 20000, False, 2, True, False), ("tanh", 1, 8, 50, 9, 20000, False, 2, False, False),
         ("linear", 0, 4, 70, 6, 1000000, False, 3, False, False), ("relu", 1, 3, 45, 5, 1000000, False, 3, False, False),
         ("elu", 0, 8, 50, 9, 20000, False, 6, False, True), ("linear", 1, 4, 45, 5, 1000000, False, 6, False, False),
         ("relu", 0, 4, 45, 5, 1000000, False, 7, False, False), ("tanh", 1, 2, 33, 6, 1000000, False, 7, False, False),
         ("linear", 0, 3, 45, 5, 1000000, False, 8, False, False), ("elu", 1, 4, 70, 6, 1000000, False, 8, False, False)]


@pytest.mark.parametrize("act,vfs,A,N,max_step,cash,deep,H,sd,metrics", CASES)
def test_net_step_equals_the_networks_policy_launch_followed_by_the_step_launch(act, vfs, A, N, max_step, cash, deep, H, sd, metrics):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd._lib import check, lib
    L = lib()
    T, seed, code = 14, 77, ACTS.index(act)
    cfg = {"num_of_agents": A, "init_cash": cash, "max_step": max_step, "is_render": False, "auto_reset": True, "n_hist": H}
    envs = [CDAVecEnv(cfg, n_markets=N, with_info=False) for _ in range(2)]
    if metrics:
        for e in envs:
            e.enable_episode_metrics()
    OBSD = 42 * H
    assert L.cda_net_step_supported(envs[1]._h, code, vfs) == 1
    th = mlp.init_theta(OBSD, generator=torch.Generator().manual_seed(5), state_dependent_log_std=sd, vf_share_layers=bool(vfs))
    th[:mlp.layout(H, act, bool(vfs)).OFF_LS] *= 1.5
    p = mlp.FusedPolicy(DEV, theta=th, n_hist=H, activation=act, vf_share_layers=bool(vfs))
    assert p.state_dependent_log_std == sd and p.activation == act and p.vf_share_layers == bool(vfs)
    obs = [e.reset(seed=900).clone() for e in envs]
    if deep:                                                      # four markets far beyond the LDS tile: the general build (HBM tier) steps them, inside both kernels
        from fuzz_cases import prefill_book
        for i in (0, 7, 16, N - 1):
            for e in envs:
                prefill_book(e, i, np.random.default_rng(50 + i), A, 400, 400)
    counter = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    cap = N * (T // max_step + 2)
    b1, b2 = _bufs(N, A, cap, OBSD), _bufs(N, A, cap, OBSD)
    st = torch.cuda.current_stream().cuda_stream
    ends = 0
    launches0 = L.cda_policy_step_launch_count(envs[1]._h)
    for t in range(T):
        for b in (b1, b2):
            b["fin_index"].fill_(-1); b["fin_count"].zero_()
        # the two launches of this network's own object
        p.policy_step(obs[0], A, seed, counter, t, outs={k: b1[k] for k in (*KEYS, "a_cont", "logp", "value")})
        check(L.cda_step_range_capture(envs[0]._h, 0, N, *[b1[k].data_ptr() for k in KEYS], None, b1["obs"].data_ptr(), b1["reward"].data_ptr(), b1["term"].data_ptr(),
                                       b1["trunc"].data_ptr(), None, b1["fin_obs"].data_ptr(), cap, b1["fin_count"].data_ptr(), b1["fin_index"].data_ptr(), st), "step")
        # one launch - as two ranges whose boundary is no multiple of the workgroup's sixteen markets
        cut = N // 2 + 3
        for first, n in ((0, cut), (cut, N - cut)):
            check(_net_step(L, envs[1], code, vfs, first, n, p, obs[1], seed, counter, t, b2, cap, st), "net step")
        torch.cuda.synchronize()
        for k in (*KEYS, "a_cont", "logp", "value", "obs", "reward", "term", "trunc"):
            assert torch.equal(b1[k], b2[k]), (k, t)
        # the sample record is the sampled action as the update's loss reads it; the distribution row is the row's normalised log-probabilities | means | log-stds
        rec = b2["rec"].cpu()
        assert torch.equal(rec[..., 0].contiguous().view(torch.int32), b2["category"].cpu()) and torch.equal(rec[..., 1].contiguous().view(torch.int32), b2["price"].cpu())
        assert torch.equal(rec[..., 2].contiguous().view(torch.int32), b2["price_offset"].cpu()) and torch.equal(rec[..., 3:5], b2["a_cont"].cpu()) and torch.equal(rec[..., 5], b2["logp"].cpu())
        out = p.forward(obs[1]).cpu()
        ls_rows = p.log_std.cpu().double() + out[:, 25:27].double()
        assert (float(out[:, 25:27].abs().max()) > 0.05) == sd
        want = torch.cat([torch.log_softmax(out[:, :9].double(), -1), torch.log_softmax(out[:, 9:19].double(), -1), torch.log_softmax(out[:, 19:22].double(), -1), out[:, 22:24].double(),
                          ls_rows, torch.zeros(N, 2, dtype=torch.float64)], 1)
        assert (b2["dist"].cpu().double() - want).abs().max() < 1e-5
        # episode ends: the same markets captured, the same last observations (slots are handed out by an atomic: compared through the index)
        f1, f2 = b1["fin_index"].cpu(), b2["fin_index"].cpu()
        assert torch.equal(f1 >= 0, f2 >= 0) and int(b1["fin_count"]) == int(b2["fin_count"]) == int((f1 >= 0).sum())
        done = (b1["term"] | b1["trunc"]).cpu().bool()
        assert torch.equal(f1 >= 0, done)
        for j in torch.nonzero(done).flatten().tolist():
            assert torch.equal(b1["fin_obs"][f1[j]], b2["fin_obs"][f2[j]]), (t, j)
        ends += int(done.sum())
        obs = [b1["obs"].clone(), b2["obs"].clone()]
    assert L.cda_policy_step_launch_count(envs[1]._h) - launches0 == 2 * T and L.cda_policy_step_launch_count(envs[0]._h) == 0
    assert ends > 0 or deep                                       # auto resets and episode-end captures happened inside the kernel
    for e in envs:
        assert (e.flags() == 0).all() and (e.check_invariants() == 0).all()
    for i in (0, N // 2, N - 1):                                  # and the markets themselves: record for record
        assert bytes(envs[0].get_state(i)) == bytes(envs[1].get_state(i)), i
        for side in (0, 1):
            assert np.array_equal(envs[0].get_book(i, side), envs[1].get_book(i, side)), (i, side)
    if deep:
        assert int(envs[1].book_peak().max()) > 256
    if metrics:                                                   # the TALLY instances: the episodes' tables, sum for sum
        m0, m1 = envs[0].collect_episode_metrics(), envs[1].collect_episode_metrics()
        torch.cuda.synchronize()
        assert torch.equal(m0[0], m1[0]) and torch.equal(m0[1], m1[1]) and float(m0[1].abs().sum()) > 0
    for e in envs:
        e.close()


def test_the_default_network_through_the_net_entry_point_is_the_policy_step():
    """(0, 0) forwards to cda_policy_step_range: byte for byte its outputs on a twin env, and both count as one-launch steps"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd._lib import check, lib
    L = lib()
    A, N, T, seed = 4, 70, 8, 31
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 5, "is_render": False, "auto_reset": True}
    envs = [CDAVecEnv(cfg, n_markets=N, with_info=False) for _ in range(2)]
    p = mlp.FusedPolicy(DEV, seed=3)
    obs = [e.reset(seed=41).clone() for e in envs]
    counter = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    cap = N * (T // 5 + 2)
    b1, b2 = _bufs(N, A, cap), _bufs(N, A, cap)
    st = torch.cuda.current_stream().cuda_stream
    for t in range(T):
        for b in (b1, b2):
            b["fin_index"].fill_(-1); b["fin_count"].zero_()
        check(L.cda_policy_step_range(envs[0]._h, 0, N, p.wb.data_ptr(), p.theta.data_ptr(), obs[0].data_ptr(), seed, counter.data_ptr(), t,
                                      *[b1[k].data_ptr() for k in KEYS], b1["a_cont"].data_ptr(), b1["logp"].data_ptr(), b1["value"].data_ptr(), b1["rec"].data_ptr(),
                                      b1["dist"].data_ptr(), b1["obs"].data_ptr(), b1["reward"].data_ptr(), b1["term"].data_ptr(), b1["trunc"].data_ptr(),
                                      b1["fin_obs"].data_ptr(), cap, b1["fin_count"].data_ptr(), b1["fin_index"].data_ptr(), st), "policy step")
        check(_net_step(L, envs[1], 0, 0, 0, N, p, obs[1], seed, counter, t, b2, cap, st), "net step")
        torch.cuda.synchronize()
        f1, f2 = b1["fin_index"].cpu(), b2["fin_index"].cpu()
        assert torch.equal(f1 >= 0, f2 >= 0)
        for j in torch.nonzero(f1 >= 0).flatten().tolist():
            assert torch.equal(b1["fin_obs"][f1[j]], b2["fin_obs"][f2[j]]), (t, j)
        for k in b1:
            if k not in ("fin_obs", "fin_index"):
                assert torch.equal(b1[k].view(torch.uint8), b2[k].view(torch.uint8)), (k, t)
        obs = [b1["obs"].clone(), b2["obs"].clone()]
    assert L.cda_policy_step_launch_count(envs[0]._h) == L.cda_policy_step_launch_count(envs[1]._h) == T
    for i in (0, N - 1):
        assert bytes(envs[0].get_state(i)) == bytes(envs[1].get_state(i)), i
    for e in envs:
        e.close()


def test_bad_codes_and_unsupported_envs_are_refused_before_any_launch():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd._lib import lib
    L = lib()
    one = C.c_void_p(64)
    tail = (0, 32, one, one, one, 1, one, 0, *([one] * 5), *([one] * 5), *([one] * 4), None, 0, None, None, None)
    base = dict(init_cash=1000000, max_step=64, is_render=False, auto_reset=True)
    env = CDAVecEnv(dict(base, num_of_agents=4), n_markets=32, with_info=False)
    for act, vfs in ((4, 0), (-1, 0), (1, 2), (4, 1), (0, -1)):
        assert L.cda_net_step_supported(env._h, act, vfs) == -1 and L.cda_net_step_advised(env._h, act, vfs) == -1
        assert L.cda_net_step_range(env._h, act, vfs, *tail) == -1
    for act in range(4):
        for vfs in (0, 1):
            assert (L.cda_net_step_supported(env._h, act, vfs), L.cda_net_step_advised(env._h, act, vfs)) == (1, 1)
    # the trade tape: no one-launch instance writes it - refused while it is on, back when it is off
    env.enable_tape(64)
    assert L.cda_net_step_supported(env._h, 1, 1) == 0 and L.cda_net_step_range(env._h, 1, 1, *tail) == -4
    env.disable_tape()
    assert L.cda_net_step_supported(env._h, 1, 1) == 1
    assert L.cda_policy_step_launch_count(env._h) == 0
    env.close()
    for cfg in ({"num_of_agents": 12}, {"num_of_agents": 4, "book_capacity": 512}, {"num_of_agents": 4, "n_hist": 5}):
        env = CDAVecEnv(dict(base, **cfg), n_markets=32, with_info=False)
        for act, vfs in ((1, 0), (0, 1), (3, 1)):
            assert L.cda_net_step_supported(env._h, act, vfs) == 0 and L.cda_net_step_advised(env._h, act, vfs) == 0, cfg
            assert L.cda_net_step_range(env._h, act, vfs, *tail) == -4, cfg
        assert L.cda_policy_step_launch_count(env._h) == 0
        env.close()


@pytest.mark.parametrize("act,vfs", [("relu", False), ("elu", False), ("linear", False), ("tanh", True), ("relu", True)])
def test_rollout_chains_take_the_one_launch_and_equal_the_two_launch_rollout(act, vfs, monkeypatch):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    N, A, T, G = 192, 4, 12, 4
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}
    runs = {}
    for name, flag, graphs in (("default", None, False), ("two", "0", False), ("forced", "2", False), ("graphs", None, True)):
        if flag is None:
            monkeypatch.delenv("CDA_POLICY_STEP", raising=False)
        else:
            monkeypatch.setenv("CDA_POLICY_STEP", flag)
        env = CDAVecEnv(cfg, n_markets=N, with_info=False)
        p = mlp.FusedPolicy(DEV, seed=29, activation=act, vf_share_layers=vfs)
        env.reset(seed=500)
        roll = mlp.RolloutChains(env, p, T, groups=G, seed=99, use_graphs=graphs)
        assert roll.launches_per_step == (2 if flag == "0" else 1), name
        assert roll.policy_step_launches() == 0
        buf = roll.run()
        torch.cuda.synchronize()
        runs[name] = {k: v.cpu().clone() for k, v in buf.items()}
        assert roll.launches_per_step == (2 if flag == "0" else 1), name
        if graphs:
            assert roll.policy_step_launches() == T * G              # (the capture's enqueue; replays do not count)
        else:
            assert roll.policy_step_launches() == (0 if flag == "0" else T * G), name
            roll.run()
            torch.cuda.synchronize()
            assert roll.policy_step_launches() == (0 if flag == "0" else 2 * T * G), name
        assert (env.flags() == 0).all()
        env.close()
    a = runs["default"]
    for name in ("two", "forced", "graphs"):
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), runs[name][k].view(torch.uint8)), (name, k)
    if (act, vfs) == ("relu", True):                              # ... and the recorded actions replay through the oracle
        import oracle_lib as O
        ora = O.OracleEnv({k: v for k, v in cfg.items() if k != "auto_reset"}, N)
        o0 = ora.reset(seeds=(500 + np.arange(N)).astype(np.uint64))
        assert np.array_equal(a["obs"][0].numpy().view(np.uint32), o0.view(np.uint32))
        for t in range(T):
            oo, orw, *_ = ora.step(a["category"][t].numpy(), a["size_mean"][t].numpy(), a["size_sigma"][t].numpy(), a["price"][t].numpy(), a["price_offset"][t].numpy())
            assert np.array_equal(a["reward"][t].numpy().view(np.uint64), orw.view(np.uint64)), t
            assert np.array_equal(a["obs"][t + 1].numpy().view(np.uint32), oo.view(np.uint32)), t
        ora.close()


def test_training_a_relu_shared_trunk_is_the_same_run_on_either_path(monkeypatch):
    """the rollouts of the two paths are bit-identical and the update is deterministic (resumed runs are bit-identical): the same parameters, the same losses"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, ppo
    cfg = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 48, "is_render": False, "auto_reset": True}
    out = []
    for flag in (None, "0"):
        if flag is None:
            monkeypatch.delenv("CDA_POLICY_STEP", raising=False)
        else:
            monkeypatch.setenv("CDA_POLICY_STEP", flag)
        keep = {}
        env = CDAVecEnv(cfg, n_markets=256, with_info=False)
        pol, hist = ppo.train_fused(env, iters=2, horizon=16, minibatch=256 * 16 * 4 // 2, chains=2, log=lambda *_: None, activation="relu", vf_share_layers=True, keep=keep)
        torch.cuda.synchronize()
        assert keep["rollout"].launches_per_step == (1 if flag is None else 2)
        assert (keep["rollout"].policy_step_launches() > 0) == (flag is None)
        out.append((pol.theta.cpu().clone(), hist))
        env.close()
    (th_a, h_a), (th_b, h_b) = out
    assert torch.equal(th_a.view(torch.int32), th_b.view(torch.int32))
    timing = ("agent_steps_per_s", "rollout_s", "update_s")
    assert len(h_a) == len(h_b) == 2
    for x, y in zip(h_a, h_b):
        assert {k: v for k, v in x.items() if k not in timing} == {k: v for k, v in y.items() if k not in timing}
        assert all(k in x for k in ("pg_loss", "v_loss", "entropy"))
