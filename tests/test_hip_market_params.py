"""GPU: per-market environment parameters (include/cda.h cda_market_params, CDAVecEnv(market_configs=...)).

Many configurations in ONE env must behave, market for market, exactly like one env per configuration: the golden traces of the reference replay bit for
bit with one market per trace, and a heterogeneous batch equals the homogeneous envs row for row on every path (the step with and without info tensors,
market groups, the one-launch episode, the policy inside the step kernel and the two-launch rollout, episode metrics, snapshots, the fused trainers)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import golden_util as G                                       # noqa: E402

pytestmark = pytest.mark.gpu

class RowsHipEnv:
    """tests/hip_env.HipEnv over ONE CDAVecEnv whose markets carry their own configs"""

    def __init__(self, config, market_configs):
        from hip_env import HipEnv
        from gym_continuousdoubleauction_amd.vec_env import CDAVecEnv
        self._inner = HipEnv.__new__(HipEnv)
        self._inner.env = CDAVecEnv(config, n_markets=len(market_configs), device="cuda:0", with_info=True, market_configs=market_configs)
        self._inner.n, self._inner.A = self._inner.env.n_markets, self._inner.env.num_agents
        self.env = self._inner.env

    def __getattr__(self, k):
        return getattr(self._inner, k)


def _golden_shapes():
    """the golden traces grouped by their shape keys (the keys one env must share)"""
    groups = {}
    for n in G.trace_names():
        rec = G.load(n)
        c = rec["config"]
        key = (c.get("num_of_agents", 5), c.get("n_hist", 4))
        groups.setdefault(key, []).append(rec)
    return groups


SHAPES = _golden_shapes()


@pytest.mark.parametrize("shape", [(4, 4), (8, 4)], ids=["A4", "A8"])
def test_every_golden_trace_of_a_shape_replays_in_one_env(shape):
    from gym_continuousdoubleauction_amd.market_params import PER_MARKET_KEYS
    recs = SHAPES[shape]
    assert len(recs) >= 10
    base = {"num_of_agents": shape[0], "n_hist": shape[1], "max_step": max(int(r["config"].get("max_step", 64)) for r in recs), "is_render": False}
    rows = [{k: v for k, v in r["config"].items() if k in PER_MARKET_KEYS} for r in recs]
    for row in rows:
        row.setdefault("max_step", 64)
    assert len({json.dumps(r, sort_keys=True) for r in rows}) >= (6 if shape[0] == 4 else 3)     # many distinct configs in the one env
    env = RowsHipEnv(base, rows)
    assert G.run_group(env, recs, state_every=8) > 0
    assert (env.flags() == 0).all()
    for i, r in enumerate(recs):
        eff = env.env.market_config(i)
        for k, v in rows[i].items():
            assert eff[k] == v, (r["name"], k)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- heterogeneous == homogeneous
BASE = {"num_of_agents": 4, "n_hist": 4, "max_step": 256, "is_render": False, "auto_reset": True}


def _configs(k=8, seed=7):
    from fuzz_cases import random_config
    from gym_continuousdoubleauction_amd.market_params import PER_MARKET_KEYS
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < k:
        cfg, _law, _p = random_config(rng)
        row = {kk: v for kk, v in cfg.items() if kk in PER_MARKET_KEYS}
        row["max_step"] = int(rng.choice([40, 64, 100, 256]))      # episodes end (and auto reset) at different steps in different markets
        out.append(row)
    out[0]["tick_size"], out[1]["init_cash"], out[2]["init_cash"] = 5, 400, 50000000000
    return out


def _envs(n, configs, groups=1, with_info=True, extra=None):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    base = dict(BASE, **(extra or {}))
    k = len(configs)
    het = CDAVecEnv(base, n_markets=n, with_info=with_info, groups=groups, market_configs=[configs[m % k] for m in range(n)])
    homs = [CDAVecEnv(dict(base, **c), n_markets=n, with_info=with_info, groups=groups) for c in configs]
    return het, homs


def _bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint8).reshape(a.shape[0], -1) if a.ndim else a


def _rows_equal(het_t, hom_ts, what):
    k = len(hom_ts)
    h = _bits(het_t)
    for j, ht in enumerate(hom_ts):
        assert np.array_equal(h[j::k], _bits(ht)[j::k]), f"{what}: config {j}"


def _state_bytes(env, m):
    import ctypes as C
    s = env.get_state(m)
    return C.string_at(C.addressof(s), C.sizeof(s))


@pytest.mark.parametrize("groups", [1, 4])
def test_heterogeneous_env_equals_the_homogeneous_envs_row_for_row(groups):
    N, T, seed, aseed = 1024, 256, 31, 5
    configs = _configs()
    het, homs = _envs(N, configs, groups=groups)
    for e in [het] + homs:
        e.reset(seed=seed)
    acts = het.random_actions_device(0, T, action_seed=aseed)
    for t in range(T):
        a = [x[t] for x in acts]
        outs = [e.step(*a) for e in [het] + homs]
        for e in [het] + homs:
            e.join()
        for idx, name in enumerate(("obs", "reward", "terminated", "truncated")):
            _rows_equal(outs[0][idx], [o[idx] for o in outs[1:]], f"step {t} {name}")
        for name in outs[0][4]:
            _rows_equal(outs[0][4][name], [o[4][name] for o in outs[1:]], f"step {t} info.{name}")
    k = len(configs)
    for m in (0, 1, 2, 3, 5, 8, 13, 100, 517, N - 1):
        assert _state_bytes(het, m) == _state_bytes(homs[m % k], m), m
    _rows_equal(het.flags(), [h.flags() for h in homs], "flags")
    for e in [het] + homs:
        e.close()


def test_heterogeneous_env_equals_the_oracle_with_each_markets_config():
    from oracle_lib import OracleEnv
    N, T, seed = 32, 256, 3
    configs = [dict(c, max_step=256) for c in _configs(seed=11)]       # (no auto reset on this path: every episode runs the whole replay)
    k = len(configs)
    het, homs = _envs(N, configs, extra={"auto_reset": False})
    for e in homs:
        e.close()
    oras = [OracleEnv(dict(BASE, auto_reset=False, **c), n_markets=N) for c in configs]
    seeds = np.arange(N, dtype=np.uint64) + np.uint64(seed)
    het.reset(seed=seed)
    for o in oras:
        o.reset(seeds=seeds)
    for t in range(T):
        a = [x.cpu().numpy()[0] for x in het.random_actions_device(t, 1, action_seed=9)]
        obs, rew, term, trunc, _ = het.step(*[torch.from_numpy(x).cuda() for x in a])
        obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
        for j, o in enumerate(oras):
            oo, orw, ot, otr, _ = o.step(*a)
            assert np.array_equal(G.f32_bits(obs[j::k]), G.f32_bits(oo[j::k])), (t, j)
            assert np.array_equal(G.f64_bits(rew[j::k]), G.f64_bits(orw[j::k])), (t, j)
            assert np.array_equal(term.cpu().numpy()[j::k].astype(np.uint8), np.asarray(ot)[j::k].astype(np.uint8)), (t, j)
            assert np.array_equal(trunc.cpu().numpy()[j::k].astype(np.uint8), np.asarray(otr)[j::k].astype(np.uint8)), (t, j)
    het.close()
    for o in oras:
        o.close()


def test_one_launch_episodes_and_the_sweep_equal_the_per_config_runs():
    from gym_continuousdoubleauction_amd import cda_rand
    N, T, seed = 1024, 256, 4
    configs = _configs(seed=5)
    k = len(configs)
    het, homs = _envs(N, configs, with_info=False, extra={"auto_reset": False})
    outs = []
    for e in [het] + homs:
        e.reset(seed=seed)
        outs.append([x.clone() for x in e.run_random(T, action_seed=seed)])
    for i, name in enumerate(("obs", "return", "terminated", "truncated", "steps")):
        _rows_equal(outs[0][i], [o[i] for o in outs[1:]], f"run_random {name}")
    for m in (0, 7, 9, N - 1):
        assert _state_bytes(het, m) == _state_bytes(homs[m % k], m)
    got = cda_rand.sweep(configs, N // k, T, seed=seed, base={"num_of_agents": 4, "n_hist": 4, "max_step": 256})
    for j, g in enumerate(got):
        r = outs[j + 1][1].cpu().numpy()[j::k]
        s = outs[j + 1][4].cpu().numpy()[j::k].astype(np.float64)
        assert g["markets"] == N // k and g["config"] == configs[j]
        assert g["return_mean"] == r.mean(axis=0).tolist() and g["return_std"] == r.std(axis=0).tolist()
        assert g["steps_mean"] == float(s.mean()) and g["steps_std"] == float(s.std())
    for e in [het] + homs:
        e.close()


@pytest.mark.parametrize("one_launch", ["2", "0"], ids=["policy_step", "two_launches"])
def test_policy_in_the_loop_equals_the_homogeneous_envs(one_launch, monkeypatch):
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd._lib import lib
    monkeypatch.setenv("CDA_POLICY_STEP", one_launch)
    N, T = 256, 48
    configs = _configs(k=4, seed=13)
    het, homs = _envs(N, configs, with_info=False)
    if one_launch == "2":
        assert lib().cda_policy_step_supported(het._h) == 1
    bufs = []
    for e in [het] + homs:
        e.reset(seed=12)
        roll = mlp.RolloutChains(e, mlp.FusedPolicy("cuda:0", seed=3), T, groups=2, seed=17)
        bufs.append({kk: v.clone() for kk, v in roll.run().items() if isinstance(v, torch.Tensor)})
        torch.cuda.synchronize()
    k = len(configs)
    for name in ("category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp", "value", "reward", "record", "terminated", "truncated"):
        if name not in bufs[0]:
            continue
        h = bufs[0][name].cpu().numpy()
        ax = 1 if h.ndim >= 2 and h.shape[0] != N and h.shape[1] == N else 0     # [T, N, ...] rollout buffers, [N, ...] otherwise
        for j in range(k):
            o = bufs[j + 1][name].cpu().numpy()
            sl = (slice(None), slice(j, None, k)) if ax == 1 else (slice(j, None, k),)
            assert np.array_equal(np.ascontiguousarray(h[sl]).view(np.uint8), np.ascontiguousarray(o[sl]).view(np.uint8)), (name, j)
    for e in [het] + homs:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- episode metrics, NAV conservation
def test_episode_metrics_and_nav_conservation_with_per_market_init_cash():
    N, T = 256, 120
    configs = _configs(k=4, seed=21)
    configs[3]["init_cash"] = 3000
    k = len(configs)
    het, homs = _envs(N, configs, with_info=False)
    for e in [het] + homs:
        e.reset(seed=8)
        e.enable_episode_metrics(True)
    acts = het.random_actions_device(0, T, action_seed=2)
    for t in range(T):
        for e in [het] + homs:
            e.step(*[x[t] for x in acts])
    _, bad_h = het.nav_conservation()
    assert not bool(bad_h.any())
    agent_h, env_h = [x.clone() for x in het.collect_episode_metrics(clear=False)]
    assert float(env_h[1]) == 0.0                                  # CDA_EM_ENV_NAV_VIOLATIONS
    assert not (het.flags().cpu().numpy() & 8).any()
    # the per-market summaries: the env row of a heterogeneous env sums its markets; compare with the sum of the homogeneous envs' rows of the same markets
    from gym_continuousdoubleauction_amd import _capi as K
    eps = 0.0
    for j, e in enumerate(homs):
        _, bad = e.nav_conservation()
        assert not bool(bad.any())
    # market for market: the summaries live in the arena rows, reachable through a snapshot-free path: collect per module with module_of = market % k
    mod = torch.arange(N * het.num_agents, device="cuda:0", dtype=torch.int32).view(N, het.num_agents) // het.num_agents % k
    agent_m, _ = het.collect_episode_metrics(module_of=mod.contiguous(), n_modules=k, clear=False)
    for j, e in enumerate(homs):
        mj = torch.full((N, e.num_agents), 1, device="cuda:0", dtype=torch.int32)
        mj[j::k] = 0
        a_j, _ = e.collect_episode_metrics(module_of=mj, n_modules=2, clear=False)
        np.testing.assert_allclose(agent_m.cpu().numpy()[j], a_j.cpu().numpy()[0], rtol=1e-12, atol=0, err_msg=f"config {j}")
        eps += float(a_j.cpu().numpy()[0][K.EM_EPISODES])
    assert eps > 0
    for e in [het] + homs:
        e.close()


def test_a_ledger_fault_in_one_market_of_a_heterogeneous_env_is_reported():
    from decimal import Decimal
    from gym_continuousdoubleauction_amd import _capi as K
    from gym_continuousdoubleauction_amd import episode_metrics as EM
    N, victim = 64, 37
    configs = [{"init_cash": 400 + 1000 * j, "max_step": 6 + j} for j in range(4)]
    from gym_continuousdoubleauction_amd import CDAVecEnv
    env = CDAVecEnv(dict(BASE, max_step=16), n_markets=N, with_info=False, market_configs=[configs[m % 4] for m in range(N)])
    env.reset(seed=99)
    env.enable_episode_metrics(True)
    acts = env.random_actions_device(0, 20, action_seed=3)
    for t in range(2):
        env.step(*[x[t] for x in acts])
    st = env.get_state(victim)
    for field in ("cash", "nav", "prev_nav", "max_nav"):
        d = getattr(st.acc[2], field)
        setattr(st.acc[2], field, K.decimal_to_dec(K.dec_to_decimal(d) + Decimal("1234.5")))
    env.set_state(victim, st)
    for t in range(2, 20):
        env.step(*[x[t] for x in acts])
    torch.cuda.synchronize()
    flags = env.flags().cpu().numpy()
    assert flags[victim] & K.FLAG_NAV_CONSERVATION and not (np.delete(flags, victim) & K.FLAG_NAV_CONSERVATION).any()
    s = EM.summarise(*env.collect_episode_metrics())
    assert s["nav_conservation_violations"] == 1 and s["nav_conservation_error"] == 1234.5
    env.close()


# ---------------------------------------------------------------------------------------------------------------- set_market_configs, snapshots, trainers
def test_set_market_configs_mid_run_resets_exactly_the_changed_markets():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    N, k = 64, 4
    configs = _configs(k=k, seed=3)
    new = {"tick_size": 3, "init_cash": 5000, "max_step": 50, "order_penalty": 0.7}
    env = CDAVecEnv(BASE, n_markets=N, with_info=True, market_configs=[configs[m % k] for m in range(N)])
    ref_old = CDAVecEnv(BASE, n_markets=N, with_info=True, market_configs=[configs[m % k] for m in range(N)])
    ref_new = CDAVecEnv(dict(BASE, **new), n_markets=N, with_info=True)
    for e in (env, ref_old):
        e.reset(seed=1)
    acts = env.random_actions_device(0, 60, action_seed=4)
    for t in range(20):
        for e in (env, ref_old):
            e.step(*[x[t] for x in acts])
    changed = [3, 4, 5, 40]
    env.set_market_configs([new] * len(changed), markets=changed, seeds=[70 + i for i in range(len(changed))])
    sd = np.zeros(N, np.uint64)
    sd[changed] = [70 + i for i in range(len(changed))]
    ref_new.reset(seed=sd)
    assert env.market_config(4)["tick_size"] == 3 and env.market_config(6) == ref_old.market_config(6)
    for t in range(20, 60):
        o = env.step(*[x[t] for x in acts])
        o_old = ref_old.step(*[x[t] for x in acts])
        o_new = ref_new.step(*[x[t] for x in acts])           # (the action rows the changed markets get)
        for i in range(4):
            a, b, c = _bits(o[i]), _bits(o_old[i]), _bits(o_new[i])
            keep = [m for m in range(N) if m not in changed]
            assert np.array_equal(a[keep], b[keep]) and np.array_equal(a[changed], c[changed]), (t, i)
    for e in (env, ref_old, ref_new):
        e.close()


def test_a_snapshot_of_a_heterogeneous_env_restores_with_its_rows(tmp_path):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd.snapshot import load_snapshot, save_snapshot
    N, k = 128, 4
    configs = _configs(k=k, seed=17)
    mc = [configs[m % k] for m in range(N)]
    a = CDAVecEnv(BASE, n_markets=N, with_info=True, market_configs=mc)
    a.reset(seed=5)
    acts = a.random_actions_device(0, 80, action_seed=6)
    for t in range(30):
        a.step(*[x[t] for x in acts])
    snap = a.snapshot()
    assert snap.market_params is not None and len(snap.market_params) == N
    save_snapshot(tmp_path / "s.snap", snap)
    b = CDAVecEnv(BASE, n_markets=N, with_info=True)               # a fresh env without rows: the snapshot brings them
    b.restore(load_snapshot(tmp_path / "s.snap"))
    assert b.market_config(1) == a.market_config(1)
    for t in range(30, 80):
        oa = a.step(*[x[t] for x in acts])
        ob = b.step(*[x[t] for x in acts])
        for i in range(4):
            assert np.array_equal(_bits(oa[i]), _bits(ob[i])), (t, i)
    a.close(); b.close()


def test_ppo_resume_with_market_configs_is_exact(tmp_path):
    from gym_continuousdoubleauction_amd import CDAVecEnv, ppo
    from gym_continuousdoubleauction_amd.market_params import round_robin
    cfg = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 48, "is_render": False, "auto_reset": True}
    mc = round_robin([{"tick_size": 2, "max_step": 40}, {"init_cash": 3000}, {"trade_penalty": 0.4, "initial_price_min": 500, "initial_price_max": 700}], 256)
    kw = dict(horizon=32, minibatch=256 * 32 * 4 // 2, chains=2)
    env = lambda: CDAVecEnv(cfg, n_markets=256, with_info=False, market_configs=mc)      # noqa: E731
    keep_a, keep_b = {}, {}
    ppo.train_fused(env(), iters=3, log=lambda *_: None, keep=keep_a, checkpoint_dir=str(tmp_path / "a"), chkpt_freq=2, **kw)
    ra = {kk: keep_a["buffers"][kk].clone() for kk in ("obs", "category", "reward", "record", "logp", "value")}
    ppo.train_fused(env(), iters=3, log=lambda *_: None, keep=keep_b, checkpoint_dir=str(tmp_path / "a"), restore=str(tmp_path / "a" / "iter_2"), **kw)
    for kk, v in ra.items():
        assert torch.equal(v, keep_b["buffers"][kk]), kk


def test_one_league_iteration_on_a_heterogeneous_env():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    cfg = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 64, "is_render": False, "auto_reset": True}
    mc = [{"tick_size": 1 + m % 3, "init_cash": 1000000 + 1000 * (m % 5)} for m in range(256)]
    env = CDAVecEnv(cfg, n_markets=256, with_info=False, market_configs=mc)
    _bank, _league, hist = train_league_fused(env, iters=1, log=lambda *_: None, horizon=32, num_trainable=2, chains=2, minibatch=256 * 32 // 2)
    assert hist and all(np.isfinite(float(v)) for h in hist for kk, v in h.items() if "loss" in kk and isinstance(v, (int, float)))
    env.close()
