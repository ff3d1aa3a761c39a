"""GPU: the stateful opponents on the device (csrc/cda_stateful.inc k_stateful_actions; CDAVecEnv.set_stateful / stateful_actions / stateful_state; the rollout
chains; evaluate) against the specification (gym_continuousdoubleauction_amd/stateful.py), word for word - the five action arrays as bits and the whole state
tensor.  The specification keeps its own copy of the state and reads independent views of the device's markets: book_levels, book_agents, get_state,
market_config - at two steps also host dumps of the books.  The closed-loop case is stateful_util's, the one tests/test_stateful_host.py plays on the oracle."""
import dataclasses

import numpy as np
import pytest
import torch

import stateful_util as U
from gym_continuousdoubleauction_amd import _capi as K
from gym_continuousdoubleauction_amd import stateful as F
from gym_continuousdoubleauction_amd.stateful import Profile

pytestmark = pytest.mark.gpu

KEYS = U.KEYS
RICH = 10 ** 12
SENTINEL = 0x5a5a5a5a5a5a5a5a


def grid(n, a):
    return np.meshgrid(np.arange(n), np.arange(a), indexing="ij")


def check_step(env, spec_state, draw, counter=0, tally=None, tag="", dumps=False):
    """one call of stateful_actions against the specification advanced from spec_state [N, A, 4] on independent views; returns (the device's action dict, the
    new specification state).  Slots the table does not name are not compared (and keep spec_state's words)."""
    n, a = env.n_markets, env.num_agents
    slots, profiles = env.stateful_slots(), env.stateful_profiles()
    on, pix = slots != 0, np.maximum(slots - 1, 0)
    m, j = grid(n, a)
    views = U.views_of_env(env)
    if dumps:                                                # the same views from host dumps of the books: an error the report kernels and the walk shared would show here
        assert np.array_equal(views, U.views_of_env(env, dumps=True)), tag
    sa = env._stateful
    want, new = F.play(profiles, pix, views, spec_state, sa.seed, counter, sa.market_index_base + m, draw, j, branches=None)
    if tally is not None:                                    # (the tally counts attached slots only)
        F.play(profiles, pix[on], views[on], spec_state[on], sa.seed, counter, (sa.market_index_base + m)[on], draw, j[on], branches=tally)
    new = np.where(on[:, :, None], new, spec_state)
    got = env.stateful_actions(draw=draw, counter=counter)
    for k, w in zip(KEYS, want):
        g = got[k].cpu().numpy()
        assert np.array_equal(g[on].view(np.uint32), w[on].view(np.uint32)), (tag, k, np.argwhere((g != w) & on)[:4])
    st = env.stateful_state().cpu().numpy()
    assert np.array_equal(st, new), (tag, "state", np.argwhere(st != new)[:4])
    return got, new


@pytest.mark.parametrize("n,a,tile", U.SHAPES)
def test_device_equals_specification_through_an_episode(n, a, tile):
    """every slot stateful, the six profiles of the shared case mixed across slots, ticks 1 and 5 across markets, episodes of six steps: the in-kernel reset
    happens three times in 24 steps, and every slot's memory restarts with it"""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    env = CDAVecEnv(dict(U.case_config(a, tile), auto_reset=True), n_markets=n, device="cuda:0", with_info=False, market_configs=[{"tick_size": t} for t in U.case_ticks(n)])
    if tile:
        assert env.book_capacity == tile
    env.reset(seed=U.RESET_SEED)
    env.set_stateful(U.mixed_slots(n, a), U.CASE, seed=U.SEED, market_index_base=U.BASE)
    assert env.stateful and env.stateful_state().shape == (n, a, F.STATE_WORDS) and not bool(env.stateful_state().any())
    ref = U.oracle_episode(n, a)
    state, tally = np.zeros((n, a, F.STATE_WORDS), np.int64), {}
    for t in range(U.STEPS):
        got, state = check_step(env, state, t, tally=tally, tag=f"step {t}", dumps=t in (4, 15))
        for k, key in enumerate(KEYS):                       # ... and what the oracle run played, step for step
            assert np.array_equal(got[key].cpu().numpy().view(np.uint32), ref["actions"][k][t].view(np.uint32)), (t, key)
        env.step(got)
    assert tally == ref["tally"] and U.TRADING <= set(tally)
    assert int(env.get_state(0).t_step) == U.STEPS % U.MAX_STEP
    assert (env.flags().cpu().numpy() == 0).all() and (env.check_invariants().cpu().numpy() == 0).all()
    env.close()


def _mid_episode_env(n=12, a=8, steps=9, max_step=64):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 10 ** 9, "max_step": max_step, "is_render": False, "auto_reset": True}, n_markets=n, device="cuda:0", with_info=False)
    env.reset(seed=77)
    env.set_stateful(U.mixed_slots(n, a), U.CASE, seed=3)
    state = np.zeros((n, a, F.STATE_WORDS), np.int64)
    for t in range(steps):
        got, state = check_step(env, state, t, tag=f"warm {t}")
        env.step(got)
    return env, state


def test_idempotence_on_the_device():
    env, state = _mid_episode_env()
    a1, state = check_step(env, state, 9, tag="first call")
    s1 = env.stateful_state().clone()
    a2 = env.stateful_actions(draw=10)                       # the same t_step: no update, so not even the value law's draw number matters
    assert all(torch.equal(a1[k].view(torch.int32), a2[k].view(torch.int32)) for k in KEYS) and torch.equal(env.stateful_state(), s1)
    assert len(set(a1["category"].cpu().numpy().reshape(-1).tolist())) >= 3
    env.close()


def test_other_slots_keep_their_bytes():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from test_hip_scripted import MIXED
    from test_hip_scripted import mixed_slots as scripted_mix
    n, a = 24, 8
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 10 ** 9, "max_step": 4096, "is_render": False}, n_markets=n, device="cuda:0", with_info=False)
    env.reset(seed=4)
    m, j = grid(n, a)
    kind = (m + j) % 3                                       # 0: stateless, 1: stateful, 2: in neither table
    sl_script = np.where(kind == 0, scripted_mix(n, a), 0).astype(np.int32)
    sl_state = np.where(kind == 1, U.mixed_slots(n, a), 0).astype(np.int32)
    sl_state[5] = 0                                          # a market without any stateful slot
    g = torch.Generator().manual_seed(1)
    out = {k: torch.randint(-2 ** 31, 2 ** 31 - 1, (n, a) + sh, generator=g, dtype=torch.int64).to(torch.int32).to("cuda:0") for k, sh in
           (("category", ()), ("size_mean", ()), ("size_sigma", ()), ("price", ()), ("price_offset", ()), ("a_cont", (2,)), ("logp", ()), ("record", (8,)))}
    out = {k: (v if k in ("category", "price", "price_offset") else v.view(torch.float32)) for k, v in out.items()}
    before = {k: v.clone() for k, v in out.items()}
    env.stateful_actions(draw=3, out=out)                    # nothing attached: nothing is written
    assert all(torch.equal(out[k].view(torch.int32), before[k].view(torch.int32)) for k in out)
    env.set_scripted(sl_script, MIXED, seed=8)
    env.set_stateful(sl_state, U.CASE, seed=9, market_index_base=70)
    env.run_scripted(20, others="random", action_seed=3)     # both families play; books stand afterwards
    assert env.book_counts().cpu().numpy()[:, :, 0].sum() > 0
    only_script = {k: v.clone() for k, v in before.items()}
    env.scripted_actions(draw=3, out=only_script)            # what k_script_actions alone writes
    env.stateful_state().fill_(SENTINEL)                     # (a foreign tag: every stateful slot starts fresh at this call)
    env.scripted_actions(draw=3, out=out)
    env.stateful_actions(draw=3, out=out, first_market=2, n_markets=20)      # ... and markets outside the range are not touched
    on = torch.from_numpy(sl_state != 0).to("cuda:0")
    on[:2] = False; on[22:] = False
    for k in out:
        assert torch.equal(out[k].view(torch.int32)[~on], only_script[k].view(torch.int32)[~on]), k
    unnamed = torch.from_numpy((sl_script == 0) & (sl_state == 0)).to("cuda:0")
    for k in out:
        assert torch.equal(out[k].view(torch.int32)[unnamed], before[k].view(torch.int32)[unnamed]), k
    st = env.stateful_state().cpu().numpy()
    onh = on.cpu().numpy()
    assert (st[~onh] == SENTINEL).all()
    pix = np.maximum(sl_state - 1, 0)
    want, new = F.play(U.CASE, pix, U.views_of_env(env), np.full((n, a, 4), SENTINEL, np.int64), 9, 0, 70 + m, 3, j)
    assert np.array_equal(st[onh], new[onh]) and ((st[onh][:, 0] >> 32) == sl_state[onh]).all()
    for k, w in zip(KEYS, want):
        assert np.array_equal(out[k].cpu().numpy()[onh].view(np.uint32), w[onh].view(np.uint32)), k
    rec = out["record"].view(torch.int32)[on].cpu().numpy()
    assert np.array_equal(rec[:, 0], want[0][onh]) and np.array_equal(rec[:, 1], want[3][onh]) and np.array_equal(rec[:, 2], want[4][onh]) and (rec[:, 3:6] == 0).all()
    assert np.array_equal(rec[:, 6:], before["record"].view(torch.int32)[on].cpu().numpy()[:, 6:])       # the advantage / return words are the update's
    assert (out["a_cont"][on] == 0).all() and (out["logp"][on] == 0).all()
    env.close()


def test_deep_book():
    """four markets prefilled with 400 + 400 orders: both sides continue in the HBM ring behind the 256-order tile; the execution law's own-order count runs beyond
    one 64-order pass of the walk, and with orders resting it modifies"""
    from fuzz_cases import prefill_book
    from hip_env import HipEnv
    from test_hip_book_report import _ring_meta
    a = 4
    hip = HipEnv({"num_of_agents": a, "init_cash": RICH, "max_step": 4096, "is_render": False}, 4, with_info=False)
    hip.reset(np.arange(70, 74, dtype=np.uint64))
    for i in range(4):
        prefill_book(hip, i, np.random.default_rng(60 + i), a, 400, 400)
    env = hip.env
    for i in range(4):
        tails, _ = _ring_meta(env, i)
        assert tails[0] > 0 and tails[1] > 0, (i, tails)
    sz = dict(size_mean=0.02, size_sigma=0.01)
    deep = [Profile(law=F.LAW_EXECUTION, target=5000, start_step=0, duration=10, patience=50, **sz), Profile(law=F.LAW_EXECUTION, target=-5000, start_step=0, duration=10, patience=2, **sz),
            Profile(law=F.LAW_TREND, max_position=10 ** 6, fast_shift=0, slow_shift=1, warmup=0, **sz), Profile(law=F.LAW_VALUE, max_position=10 ** 6, p_move_q32=1 << 32, **sz)]
    env.set_stateful(U.mixed_slots(4, a, 4), deep, seed=5)
    assert (env.book_agents().cpu().numpy()[:, :, :, 0] > 64).any()     # own-order counts beyond one pass of the walk
    state, tally, cats = np.zeros((4, a, 4), np.int64), {}, set()
    for t in range(6):
        got, state = check_step(env, state, t, tally=tally, tag=f"prefilled, step {t}", dumps=t == 1)
        cats |= set(got["category"].cpu().numpy().reshape(-1).tolist())
        env.step(got)
    assert {"exec_passive_modify", "exec_market"} <= set(tally) and cats & {3, 7}, (tally, cats)
    assert (env.check_invariants().cpu().numpy() == 0).all()
    hip.close()


CHAIN_N, CHAIN_A, CHAIN_T = 32, 8, 12
CHAIN_CFG = {"num_of_agents": CHAIN_A, "init_cash": 1000000, "max_step": 8, "is_render": False}      # a 12-step horizon crosses an auto reset


def _chain_env(stateful):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    env = CDAVecEnv(dict(CHAIN_CFG, auto_reset=True), n_markets=CHAIN_N, device="cuda:0", with_info=False)
    env.reset(seed=300)
    if stateful:
        slots = U.mixed_slots(CHAIN_N, CHAIN_A)
        slots[:, :2] = 0
        env.set_stateful(slots, U.CASE, seed=13, market_index_base=64)
    return env


def _driver(kind):
    from gym_continuousdoubleauction_amd import mlp
    pol = mlp.FusedPolicy("cuda:0", seed=1)
    if kind == "shared":
        return pol, dict(greedy=False)
    other = mlp.FusedPolicy("cuda:0", seed=2)
    bank = mlp.PolicyBank("cuda:0", CHAIN_N, CHAIN_A, n_trainable=1, max_frozen=1, random_seed=13)
    bank.theta[0].copy_(pol.theta); bank.wb[0].copy_(pol.wb)
    bank.n_frozen += 1
    bank.theta[1].copy_(other.theta); bank.wb[1].copy_(other.wb)
    bank._refresh()
    slot_net = np.full((CHAIN_N, CHAIN_A), mlp.LEAGUE_RANDOM, np.int32)
    slot_net[:, 0], slot_net[:, 1] = 0, 1
    bank.set_slots(torch.from_numpy(slot_net))
    return bank, dict(greedy=True)


@pytest.mark.parametrize("kind", ["league_eval", "shared"])
def test_chains(kind):
    """a 12-step graph-captured chain, 32 x 8, slots 2 .. 7 stateful, two chains, episodes of 8 steps - against a per-step loop on a twin env that takes the network
    slots' recorded actions and asks stateful_actions for the rest: every action buffer, every observation and the final state tensor bit for bit"""
    from gym_continuousdoubleauction_amd import mlp
    T = CHAIN_T
    env, twin = _chain_env(True), _chain_env(True)
    driver, kw = _driver(kind)
    chains = mlp.RolloutChains(env, driver, T, groups=2, seed=5, **kw)
    assert chains.use_graphs and chains.launches_per_step == 2
    b = {k: v.clone() for k, v in chains.run().items()}
    assert chains.graphs is not None
    counter = int(chains.counter.item())
    torch.cuda.synchronize()
    on = torch.from_numpy(env.stateful_slots() != 0).to("cuda:0")
    assert torch.equal(b["obs"][0], twin.obs)
    acted, state = set(), np.zeros((CHAIN_N, CHAIN_A, 4), np.int64)
    for t in range(T):
        acts = {k: b[k][t].clone() for k in KEYS}
        for k in KEYS:                                       # the stateful slots' words must come from the twin's own launch
            acts[k][on] = 0
        sa = twin._stateful
        m, j = grid(CHAIN_N, CHAIN_A)
        _want, state = F.play(twin.stateful_profiles(), np.maximum(twin.stateful_slots() - 1, 0), U.views_of_env(twin), state, sa.seed, counter, 64 + m, t, j)
        state = np.where((twin.stateful_slots() != 0)[:, :, None], state, 0)
        twin.stateful_actions(draw=t, counter=counter, out=acts)
        for k in KEYS:
            assert torch.equal(acts[k].view(torch.int32), b[k][t].view(torch.int32)), (t, k)
        assert (b["logp"][t][on] == 0).all() and (b["a_cont"][t][on] == 0).all()
        acted |= set(acts["category"][on].cpu().numpy().tolist())
        obs, rew, *_ = twin.step(acts)
        assert torch.equal(obs.view(torch.int32), b["obs"][t + 1].view(torch.int32)) and torch.equal(rew.view(torch.int64), b["reward"][t].view(torch.int64)), t
    assert torch.equal(env.stateful_state(), twin.stateful_state())
    assert np.array_equal(env.stateful_state().cpu().numpy(), state)         # ... and both are the specification's
    assert int(twin.get_state(0).t_step) == T - CHAIN_CFG["max_step"] and len(acted) >= 4
    assert (env.flags().cpu().numpy() == 0).all() and (env.check_invariants().cpu().numpy() == 0).all()
    env.close(); twin.close()


def test_epochs_and_refusals():
    from gym_continuousdoubleauction_amd import league_train, mlp, ppo
    from gym_continuousdoubleauction_amd._lib import lib
    from test_hip_scripted import MIXED
    env = _chain_env(False)
    supported = int(lib().cda_policy_step_supported(env._h))
    assert supported == 1 and int(lib().cda_stateful_attached(env._h)) == 0 and not env.stateful
    chains = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=1), 4, groups=2, seed=5)
    chains.run()
    torch.cuda.synchronize()
    e0 = int(lib().cda_stateful_epoch(env._h))
    slots = U.mixed_slots(CHAIN_N, CHAIN_A)
    slots[:, :2] = 0
    env.set_stateful(slots, U.CASE, seed=1)
    assert int(lib().cda_stateful_epoch(env._h)) == e0 + 1 and env.stateful_epoch == 1 and int(lib().cda_policy_step_supported(env._h)) == 0
    assert int(lib().cda_net_step_supported(env._h, 0, 0)) == 0 and int(lib().cda_stateful_attached(env._h)) == 1
    with pytest.raises(RuntimeError, match="stateful"):
        chains.run()                                         # attached after the capture
    chains2 = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=1), 4, groups=2, seed=5)
    chains2.run()
    torch.cuda.synchronize()
    # the training loops refuse stateful specs, and an env that has stateful opponents attached
    for train, kw in ((ppo.train_fused, dict(opponents=["maker", "trend"], trained_slots=2)), (league_train.train_league_fused, dict(scripted_opponents=["execution:target=-40"])),
                      (ppo.train_fused, {}), (league_train.train_league_fused, {})):
        with pytest.raises(ValueError, match="stateful"):
            train(env, iters=1, **kw)
    # a stateful slot below n_trainable
    bank, kw = _driver("league_eval")
    slots[:, 0] = 1
    env.set_stateful(slots, U.CASE, seed=1)
    with pytest.raises(ValueError, match="trainable"):
        mlp.RolloutChains(env, bank, 4, groups=2, seed=5, **kw).run()
    # refused, and the env is unchanged afterwards: an invalid profile, a slot value out of range, an unaligned state pointer, an overlap with set_scripted
    e1 = int(lib().cda_stateful_epoch(env._h))
    sa = env._stateful
    kept = sa.state.clone()
    bad = torch.from_numpy(F.profiles_array([dataclasses.replace(U.CASE[0], slow_shift=13)], validate=False).view(np.uint8).copy()).to("cuda:0")
    assert lib().cda_stateful_attach(env._h, sa.slot_table.data_ptr(), bad.data_ptr(), 1, sa.state.data_ptr(), 0, 0) == K.ERR_INVALID
    big = torch.full((CHAIN_N, CHAIN_A), 2, dtype=torch.int32, device="cuda:0")
    good = torch.from_numpy(F.profiles_array([U.CASE[0]]).view(np.uint8).copy()).to("cuda:0")
    assert lib().cda_stateful_attach(env._h, big.data_ptr(), good.data_ptr(), 1, sa.state.data_ptr(), 0, 0) == K.ERR_INVALID
    ones = torch.ones((CHAIN_N, CHAIN_A), dtype=torch.int32, device="cuda:0")
    for off in (8, 16, 24):
        assert lib().cda_stateful_attach(env._h, ones.data_ptr(), good.data_ptr(), 1, sa.state.data_ptr() + off, 0, 0) == K.ERR_INVALID
    assert int(lib().cda_stateful_epoch(env._h)) == e1 and int(lib().cda_stateful_attached(env._h)) == 1 and torch.equal(sa.state, kept)
    with pytest.raises(ValueError):
        env.set_stateful(slots, [dataclasses.replace(U.CASE[1], duration=0)])
    with pytest.raises(ValueError):
        env.set_stateful(np.full((CHAIN_N, CHAIN_A), 7), U.CASE)
    env.clear_stateful()
    assert int(lib().cda_stateful_epoch(env._h)) == e1 + 1
    with pytest.raises(RuntimeError, match="stateful"):
        chains2.run()                                        # detached after the capture
    sc = np.zeros((CHAIN_N, CHAIN_A), np.int32)
    sc[:, 3] = 2
    env.set_scripted(sc, MIXED, seed=1)
    with pytest.raises(ValueError, match="set_scripted"):
        env.set_stateful(slots, U.CASE)                      # slot 3 is scripted at this moment
    assert not env.stateful and int(lib().cda_stateful_attached(env._h)) == 0 and int(lib().cda_stateful_epoch(env._h)) == e1 + 1
    slots[:, 3] = 0
    env.set_stateful(slots, U.CASE)                          # ... and beside the scripts, on other slots, it attaches
    env.clear_stateful(); env.clear_scripted()
    assert int(lib().cda_policy_step_supported(env._h)) == supported and not env.stateful
    with pytest.raises(RuntimeError):
        env.stateful_state()
    with pytest.raises(RuntimeError):
        env.run_scripted(1)
    env.close()


def test_snapshot_carries_the_state_beside_it():
    env, state = _mid_episode_env(n=12, a=8, steps=5, max_step=12)       # 10 more steps cross the episode's end
    snap, kept = env.snapshot(), env.stateful_state().clone()

    def ten(state):
        acts = []
        for t in range(5, 15):
            got, state = check_step(env, state, t, tag=f"step {t}")
            acts.append({k: got[k].clone() for k in KEYS})
            env.step(got)
        return acts, env.stateful_state().clone()

    first, end1 = ten(state)
    assert not torch.equal(end1, kept)
    env.restore(snap)
    env.stateful_state().copy_(kept)
    second, end2 = ten(state)
    assert torch.equal(end1, end2)
    for x, y in zip(first, second):
        assert all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in KEYS)
    assert len({int(c) for x in first for c in x["category"].cpu().numpy().reshape(-1)}) >= 4
    env.close()


def test_evaluate_against_stateful_opponents():
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    env = CDAVecEnv({"num_of_agents": 4, "init_cash": 1000000, "max_step": 32, "is_render": False, "auto_reset": True}, n_markets=48, device="cuda:0", with_info=False)
    res = evaluate(env, mlp.FusedPolicy("cuda:0", seed=3), opponents=["trend", "execution:target=-40"], episodes=2, seed=6)
    assert not env.stateful and not env.scripted and res["nav_conservation_violations"] == 0
    mods = res["modules"]
    assert sorted(mods) == ["opponent_0", "opponent_1", "policy"]
    assert res["stateful_modules"] == {"opponent_0": "stateful_0_trend", "opponent_1": "stateful_1_execution"}
    assert mods["opponent_0"]["module"] == "stateful_0_trend" and mods["opponent_1"]["module"] == "stateful_1_execution"
    for name, mres in mods.items():
        assert mres["agent_episodes"] > 0, name
    assert res["config"]["opponents"] == ["trend", "execution:target=-40"]
    env.close()
