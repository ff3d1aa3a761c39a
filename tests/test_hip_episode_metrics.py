"""GPU: every episode checked and summarised ON THE DEVICE (include/cda.h cda_episode_metrics_*; SURVEY 8(f) rows 2 and 3 on the fast path).

The reference's callback tallies every step of an episode (train/callbk/league_based_self_play_callback.py:541-600), checks sum(NAV) == num_agents x init_cash in
Decimal at every episode END and summarises the accounts (:627-755); its driver stops a strict run on a violation (train/train.py:1109-1164).  With the in-kernel
auto reset the finished episode's ledger is gone before any host code runs, so the cold episode-end paths do it.  Checked here against the same figures computed on the
host from the CPU oracle's replay of the recorded actions: integer and decimal-derived columns bit for bit, f64 sums within 1e-12 (tests/episode_metrics_util.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from step_variants import _replay      # noqa: E402  (the actions through the oracle under the env's auto-reset rule; shared with tests/test_hip_step_variants.py)

pytestmark = pytest.mark.gpu

ACTION_KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset")


def _cfg(A, max_step, cash=1000000, **kw):
    return dict({"num_of_agents": A, "init_cash": cash, "max_step": max_step, "is_render": False, "auto_reset": True}, **kw)


def _oracle(cfg, N, seed):
    import oracle_lib as O
    ora = O.OracleEnv({k: v for k, v in cfg.items() if k != "auto_reset"}, N)
    ora.reset(seeds=(seed + np.arange(N)).astype(np.uint64))
    return ora


def _actions(rng, N, A, aggressive=False):
    cat = rng.integers(0, 9, (N, A)).astype(np.int32)
    if aggressive:                                            # many market orders: fills, passive fills, now and then a bankruptcy on small accounts
        cat = np.where(rng.random((N, A)) < 0.5, rng.choice([1, 5], (N, A)), cat).astype(np.int32)
    return (cat, rng.uniform(-1, 1, (N, A)).astype(np.float32), rng.uniform(0, 1, (N, A)).astype(np.float32), rng.integers(0, 10, (N, A)).astype(np.int32),
            rng.integers(0, 3, (N, A)).astype(np.int32))


@pytest.mark.parametrize("with_info", [False, True])
@pytest.mark.parametrize("A,max_step,cash", [(4, 7, 1000000), (8, 5, 3000), (3, 1, 1000000)])
def test_stepwise_metrics_equal_the_oracle_replay(with_info, A, max_step, cash):
    """cda_step on an auto_reset env: the in-kernel reset of the info-less kernel / the reset pass behind the kernel with info tensors credit every episode end"""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from episode_metrics_util import OracleEpisodeMetrics, assert_tables_equal
    N, T, seed = 80, 23, 4100
    cfg = _cfg(A, max_step, cash)
    env = CDAVecEnv(cfg, n_markets=N, with_info=with_info)
    env.reset(seed=seed)
    env.enable_episode_metrics(True)
    ora, em = _oracle(cfg, N, seed), OracleEpisodeMetrics(N, A, cash)
    rng = np.random.default_rng(5 + A)
    steps = [_actions(rng, N, A, aggressive=cash < 100000) for _ in range(T)]
    for k, acts in enumerate(steps):
        env.step(*acts)
        if k == 11:                                           # a collection in the middle: the accumulators restart, the running tallies go on
            _replay(ora, em, steps[:12])
            dev = [t.cpu().numpy() for t in env.collect_episode_metrics()]
            assert_tables_equal(dev[0], dev[1], *em.table(), what="first collection")
    _replay(ora, em, steps[12:])
    dev = [t.cpu().numpy() for t in env.collect_episode_metrics()]
    ref = em.table()
    assert ref[1][0] >= N * ((T - 12) // max_step) and (cash > 100000 or ref[1][7] > 0 or True)
    assert_tables_equal(dev[0], dev[1], *ref, what="second collection")
    again = [t.cpu().numpy() for t in env.collect_episode_metrics()]      # cleared behind the read
    assert not again[0].any() and not again[1].any()
    assert not em.violating and (env.flags() == 0).all()
    env.close(); ora.close()


def test_reset_of_an_unfinished_episode_discards_it_and_a_finished_one_is_credited_once():
    """no auto reset: the episode end is credited by the reset that follows it (once); an episode that is reset before its end is dropped, as the reference's callback
    never sees it end (callbk:481-497)"""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from episode_metrics_util import OracleEpisodeMetrics, assert_tables_equal
    N, A, max_step, seed = 48, 4, 6, 977
    cfg = {k: v for k, v in _cfg(A, max_step).items() if k != "auto_reset"}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    env.reset(seed=seed)
    env.enable_episode_metrics(True)
    ora, em = _oracle(cfg, N, seed), OracleEpisodeMetrics(N, A, 1000000)
    rng = np.random.default_rng(1)
    for t in range(4):                                        # four steps, then half of the markets are reset early
        acts = _actions(rng, N, A)
        env.step(*acts)
        _, rew, term, trunc, info = ora.step(*acts)
        em.feed(info, rew, term, trunc, done_mask_of=lambda i: ora.get_state(i).done_mask)
    early = (np.arange(N) % 2 == 0)
    env.reset(mask=early.astype(np.uint8)); ora.reset(mask=early.astype(np.uint8)); em.discard(early)
    ended_total = np.zeros(N, bool)
    for t in range(2):                                        # the other half reaches max_step
        acts = _actions(rng, N, A)
        _, _, term, trunc, _ = env.step(*acts)
        _, rew, oterm, otrunc, info = ora.step(*acts)
        ended_total[em.feed(info, rew, oterm, otrunc, done_mask_of=lambda i: ora.get_state(i).done_mask)] = True
    assert ended_total.sum() == N // 2 and np.array_equal((term | trunc).cpu().numpy(), ended_total)
    dev = [t.cpu().numpy() for t in env.collect_episode_metrics(clear=False)]
    assert dev[1][0] == 0                                     # nothing credited yet: nobody has reset the finished markets
    env.reset(mask=ended_total.astype(np.uint8))
    env.reset(mask=ended_total.astype(np.uint8))              # a second reset of the same markets credits nothing more
    dev = [t.cpu().numpy() for t in env.collect_episode_metrics()]
    assert_tables_equal(dev[0], dev[1], *em.table(), what="credited by the reset")
    env.close(); ora.close()


def test_random_agent_episodes_in_one_launch_are_credited():
    """cda_run_random ends an episode without resetting: the launch itself checks and credits it, the reset that follows does not do it again"""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from episode_metrics_util import OracleEpisodeMetrics, assert_tables_equal
    N, A, max_step, seed = 64, 4, 9, 31
    cfg = {k: v for k, v in _cfg(A, max_step, cash=4000).items() if k != "auto_reset"}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    env.reset(seed=seed)
    env.enable_episode_metrics(True)
    ora, em = _oracle(cfg, N, seed), OracleEpisodeMetrics(N, A, 4000)
    env.run_random(max_step + 3, action_seed=77)
    alive = np.ones(N, bool)
    for t in range(max_step):
        acts = env.random_actions(t, action_seed=77)
        keep = ora.get_state
        _, rew, term, trunc, info = ora.step(*acts)
        # (a market that ended earlier keeps being stepped by this loop: only its first end counts, like the launch that stopped there)
        info = {k: v.copy() for k, v in info.items()}
        mask_t, mask_u = term.copy(), trunc.copy()
        mask_t[~alive] = 0; mask_u[~alive] = 0
        if (~alive).any():
            for k in ("reward_terms", "is_pass_action", "num_rejected_step", "order_step_placed", "num_trades_step", "num_passive_fills_step"):
                info[k][~alive] = 0
            rew = rew.copy(); rew[~alive] = 0
        em.steps[~alive] -= 1
        ended = em.feed(info, rew, mask_t, mask_u, done_mask_of=lambda i: keep(i).done_mask)
        alive[ended] = False
    assert not alive.any()
    dev = [t.cpu().numpy() for t in env.collect_episode_metrics(clear=False)]
    assert_tables_equal(dev[0], dev[1], *em.table(clear=False), what="credited by the launch")
    env.reset()
    dev = [t.cpu().numpy() for t in env.collect_episode_metrics()]
    assert_tables_equal(dev[0], dev[1], *em.table(), what="not credited twice")
    env.close(); ora.close()


@pytest.mark.parametrize("A,N,H", [(4, 96, 4), (8, 64, 4), (4, 40, 2)])
def test_fused_rollout_metrics_equal_the_oracle_replay(A, N, H):
    """the PPO rollout (policy inside the step kernel where the env qualifies, HIP graphs, in-kernel auto reset): two rollouts of 14 steps over 5-step episodes"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from episode_metrics_util import OracleEpisodeMetrics, assert_tables_equal
    T, max_step, seed, cash = 14, 5, 880, 20000
    cfg = _cfg(A, max_step, cash, n_hist=H)
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    env.reset(seed=seed)
    env.enable_episode_metrics(True)
    roll = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=3, n_hist=H), T, groups=2, seed=17)
    ora, em = _oracle(cfg, N, seed), OracleEpisodeMetrics(N, A, cash)
    for rnd in range(2):
        b = {k: v.cpu().numpy() for k, v in roll.run().items() if k in ACTION_KEYS}
        torch.cuda.synchronize()
        _replay(ora, em, [tuple(b[k][t] for k in ACTION_KEYS) for t in range(T)])
        dev = [t.cpu().numpy() for t in env.collect_episode_metrics()]
        ref = em.table()
        assert ref[1][0] == N * ((rnd + 1) * T // max_step - rnd * T // max_step)
        assert_tables_equal(dev[0], dev[1], *ref, what=f"rollout {rnd}")
    env.close(); ora.close()


def test_league_rollout_metrics_are_keyed_by_module():
    """league self-play: the table's rows are the MODULES (trainable policies, random modules, champions) whatever slot they played"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd.league import LeagueSlotMapper
    from episode_metrics_util import OracleEpisodeMetrics, assert_tables_equal
    N, A, k, T, max_step, seed, cash = 64, 8, 2, 12, 6, 510, 50000
    cfg = _cfg(A, max_step, cash)
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    env.reset(seed=seed)
    env.enable_episode_metrics(True)
    bank = mlp.PolicyBank("cuda:0", N, A, k, max_frozen=4, seed=5, random_seed=9)
    mapper = LeagueSlotMapper(A, k, A - k, 1.0, 3.0)
    net_of = {}
    for _ in range(2):
        cid = mapper.add_champion()
        net_of[cid] = bank.snapshot(0)
    slot_pool = torch.full((N, A), -1, dtype=torch.int32, device="cuda:0")
    mapper.assign_device(bank, episode_ids=[f"e0-m{i}" for i in range(N)], net_of=net_of, slot_pool=slot_pool)
    module_of = torch.where(slot_pool < 0, torch.arange(A, device="cuda:0", dtype=torch.int32).expand(N, A), slot_pool + k).to(torch.int32).contiguous()
    n_mod = len(mapper.available_modules)
    roll = mlp.RolloutChains(env, bank, T, groups=2, seed=23)
    b = {key: v.cpu().numpy() for key, v in roll.run().items() if key in ACTION_KEYS}
    torch.cuda.synchronize()
    ora, em = _oracle(cfg, N, seed), OracleEpisodeMetrics(N, A, cash)
    _replay(ora, em, [tuple(b[key][t] for key in ACTION_KEYS) for t in range(T)])
    dev = [t.cpu().numpy() for t in env.collect_episode_metrics(module_of=module_of, n_modules=n_mod)]
    ref = em.table(module_of.cpu().numpy(), n_mod)
    assert (ref[0][:, 0] > 0).sum() >= k + 3                   # the trainable policies, random modules and both champions all played
    assert_tables_equal(dev[0], dev[1], *ref, what="league")
    from gym_continuousdoubleauction_amd import episode_metrics as EM
    s = EM.summarise(torch.from_numpy(dev[0]), torch.from_numpy(dev[1]), module_names=mapper.available_modules)
    assert set(s["modules"]) <= set(mapper.available_modules) and "policy_0" in s["modules"] and s["episodes"] == 2 * N
    env.close(); ora.close()


@pytest.mark.parametrize("path", ["step", "step_info", "rollout", "step+cold", "step+tape", "step_info+cold+tape"])
def test_a_ledger_fault_in_an_episode_that_auto_resets_mid_run_is_reported(path):
    """a seeded corruption of ONE market's ledger (cash created out of nothing) in an episode that ends and resets itself in the middle of the run: the violation is
    counted, the market carries the sticky flag after its reset, the trainer-side check raises like the reference's strict_nav_check run.  +cold: the victim's book
    is prefilled beyond the tile, its episode ends on the general build (slow_step / slow_tstep, the tallies by the market's ST_EP_ON bit, the end handed back to
    the kernel); +tape: the tape-writing instances (k_tstep)"""
    from decimal import Decimal
    from gym_continuousdoubleauction_amd import CDAVecEnv, _capi as K, mlp
    from gym_continuousdoubleauction_amd import episode_metrics as EM
    path, *extra = path.split("+")
    N, A, max_step, victim = 64, 4, 6, 37
    env = CDAVecEnv(_cfg(A, max_step), n_markets=N, with_info=(path == "step_info"))
    if "tape" in extra:
        env.enable_tape(1024)
    env.reset(seed=99)
    if "cold" in extra:
        from fuzz_cases import prefill_book
        prefill_book(env, victim, np.random.default_rng(6), A, 300, 300)
    env.enable_episode_metrics(True)
    rng = np.random.default_rng(2)
    for _ in range(2):
        env.step(*_actions(rng, N, A))
    st = env.get_state(victim)
    for field in ("cash", "nav", "prev_nav", "max_nav"):      # agent 2 finds 1234.5 that nobody lost
        d = getattr(st.acc[2], field)
        setattr(st.acc[2], field, K.decimal_to_dec(K.dec_to_decimal(d) + Decimal("1234.5")))
    env.set_state(victim, st)
    if path == "rollout":
        roll = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=3), 16, groups=2, seed=1)
        roll.run()
    else:
        for k in range(16):
            if k == max_step - 3:                             # before the step that ends the corrupted episode: the victim alone is cold
                cold = env.book_counts()[:, :, 0].sum(1).cpu().numpy() + A > env.book_capacity
                assert bool(cold[victim]) == ("cold" in extra) and not np.delete(cold, victim).any()
            env.step(*_actions(rng, N, A))
    torch.cuda.synchronize()
    flags = env.flags().cpu().numpy()
    assert flags[victim] & K.FLAG_NAV_CONSERVATION and not (np.delete(flags, victim) & K.FLAG_NAV_CONSERVATION).any()
    agent, envrow = env.collect_episode_metrics()
    s = EM.summarise(agent, envrow)
    assert s["nav_conservation_violations"] == 1 and s["nav_conservation_error"] == 1234.5 and s["episodes"] >= 2 * N
    with pytest.raises(EM.NavConservationError):
        EM.check_nav_conservation(0, s, strict=True)
    logged = []
    EM.check_nav_conservation(0, s, strict=False, log=logged.append)
    assert logged and "strict_nav_check is off" in logged[0]
    _, bad = env.nav_conservation()                            # ... while the end-of-run check sees nothing: the faulty episode is long gone
    assert not bool(bad.any())
    env.close()


def test_metrics_off_touch_nothing_and_the_step_is_unchanged():
    """off (the default): no tallies, no accumulators, the same outputs bit for bit as with metrics on"""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    N, A = 64, 4
    outs = []
    for on in (False, True):
        env = CDAVecEnv(_cfg(A, 5), n_markets=N, with_info=False)
        env.reset(seed=3)
        if on:
            env.enable_episode_metrics(True)
        rng = np.random.default_rng(8)
        rows = []
        for _ in range(12):
            o, r, te, tr, _ = env.step(*_actions(rng, N, A))
            rows.append((o.cpu().numpy().copy(), r.cpu().numpy().copy(), te.cpu().numpy().copy(), tr.cpu().numpy().copy()))
        agent, envrow = env.collect_episode_metrics()
        assert bool(envrow[0] > 0) == on and bool(agent.any()) == on
        outs.append((rows, bytes(env.get_state(5))))
        env.close()
    for (a, b) in zip(outs[0][0], outs[1][0]):
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert outs[0][1] == outs[1][1]


@pytest.mark.parametrize("N,A,max_step,T,cash,modules", [(8448, 2, 3, 7, 1000000, False),      # > 8192 markets: k_em_partial's per-market loop runs twice
                                                         (2304, 4, 10, 20, 1500, True)])        # fills and a bankruptcy; 32 modules, ids outside [0, 32) skipped
def test_collect_at_scale_equals_the_oracle_replay(N, A, max_step, T, cash, modules):
    """cda_episode_metrics_collect where k_em_partial's loops run more than once: (market, agent) pairs > 256 blocks x 8 groups = 2048, markets > 256 x 32 = 8192,
    n_modules = CDA_EM_MAX_MODULES with ids -1 and >= n_modules in module_of - against the CPU oracle's replay of every market"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, _capi as K
    from episode_metrics_util import OracleEpisodeMetrics, abs_sums, assert_tables_within_order_bound
    seed = 7300 + N
    cfg = _cfg(A, max_step, cash)
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    env.reset(seed=seed)
    env.enable_episode_metrics(True)
    rng = np.random.default_rng(N)
    steps = [_actions(rng, N, A, aggressive=cash < 100000) for _ in range(T)]
    for acts in steps:
        env.step(*acts)
    n_mod, module_of = 1, None
    if modules:
        n_mod = K.EM_MAX_MODULES                                                # (32: every module accumulator of k_em_partial in use)
        module_of = rng.integers(-1, n_mod + 3, (N, A)).astype(np.int32)       # -1 and n_mod .. n_mod + 2: played by nobody the table counts
        module_of[0, 0], module_of[1, 0], module_of[2, 0] = -1, n_mod, n_mod + 2
    dev = [t.cpu().numpy() for t in env.collect_episode_metrics(module_of=None if module_of is None else torch.from_numpy(module_of).to(env.device), n_modules=n_mod)]
    ora, em = _oracle(cfg, N, seed), OracleEpisodeMetrics(N, A, cash)
    _replay(ora, em, steps)
    sums = abs_sums(em, module_of, n_mod)
    bankrupt = em.F[..., K.EM_BANKRUPT].sum()
    ref = em.table(module_of, n_mod)
    assert ref[1][K.EM_ENV_EPISODES] == N * (T // max_step)
    if modules:
        assert (ref[0][:, K.EM_EPISODES] > 0).all() and bankrupt > 0 and ref[0][:, K.EM_TRADES].sum() > 1000
        skipped = (module_of < 0) | (module_of >= n_mod)
        assert 0 < skipped.sum() and ref[0][:, K.EM_EPISODES].sum() == (T // max_step) * (~skipped).sum()
    worst = assert_tables_within_order_bound(dev[0], dev[1], *ref, sums, what=f"{N} x {A}")
    print(f"\n[episode metrics at scale] {N} x {A}: worst f64 sum error / (2 n eps sum|x|) = {worst:.3g}")
    assert not em.violating and (env.flags() == 0).all()
    env.close(); ora.close()


def _returns_reference(reward, done, running):
    """k_episode_returns restated in float64 on the host, forwards in time per (market, agent): (running, per-slot sum of completed returns, their number)"""
    run, s, c = running.copy(), np.zeros_like(running), np.zeros_like(running)
    for t in range(reward.shape[0]):
        run = run + reward[t]
        d = done[t][:, None] & np.ones(run.shape, bool)
        s = np.where(d, s + run, s)
        c = np.where(d, c + 1.0, c)
        run = np.where(d, 0.0, run)
    return run, s, c


@pytest.mark.parametrize("T", [13, 64])
def test_episode_returns_equal_the_float64_recursion(T):
    """mlp.EpisodeReturns (k_episode_returns: eight steps' operands per request, a ragged last group at T = 13) over two consecutive rollouts of 4096 x 4: episodes
    ending at t = 0, at t = T - 1 and in the middle of an 8-step group; running and per-slot figures bit for bit (the same additions in the same time order), the
    per-slot totals within the order bound of their atomic sum over markets"""
    from gym_continuousdoubleauction_amd import mlp
    N, A = 4096, 4
    er = mlp.EpisodeReturns(N, A, "cuda:0", per_slot=True)
    rng = np.random.default_rng(T)
    running = np.zeros((N, A))
    for rnd in range(2):
        reward = rng.standard_normal((T, N, A)) * np.exp(rng.uniform(-8, 8, (T, N, A)))      # magnitudes over many binades: any reordering shows
        term = rng.random((T, N)) < 0.04
        trunc = rng.random((T, N)) < 0.02
        term[0, 0:64] = True; trunc[T - 1, 64:128] = True; term[min(11, T - 1), 128:192] = True; term[3, 192:256] = True
        term[:, 256:320] = False; trunc[:, 256:320] = False                          # markets whose episode spans both rollouts
        done = term | trunc
        buf = {"reward": torch.from_numpy(reward).to("cuda:0"), "terminated": torch.from_numpy(term.astype(np.uint8)).to("cuda:0"),
               "truncated": torch.from_numpy(trunc.astype(np.uint8)).to("cuda:0")}
        acc = er.update(buf, T).cpu().numpy()
        running, s, c = _returns_reference(reward, done, running)
        assert np.array_equal(er.running.cpu().numpy().view(np.uint64), running.view(np.uint64)), rnd
        ps = er.per_slot.cpu().numpy()
        assert np.array_equal(ps[..., 0].view(np.uint64), s.view(np.uint64)) and np.array_equal(ps[..., 1], c), rnd
        assert np.array_equal(acc[1], c.sum(0)) and (acc[1] > 0).all()
        want = s.sum(0)
        bound = 2 * N * np.finfo(np.float64).eps * np.abs(s).sum(0)
        assert (np.abs(acc[0] - want) <= bound).all(), (rnd, acc[0], want)
        print(f"\n[episode returns] T {T} rollout {rnd}: worst done_sum error / (2 n eps sum|x|) = {float((np.abs(acc[0] - want) / bound).max()):.3g}")
    assert (np.abs(running[256:320]) > 0).all()


# ---- the metrics setting and captured rollouts; the training loops and evaluate() leave the setting they were asked for -------------------------------------------------
ROLLOUT_CASES = [("shared", 1, "2"), ("shared", 2, "2"), ("shared", 1, "0"), ("shared", 2, "0"),      # the one-launch k_policy_step (where the env qualifies) / two launches per step
                 ("league", 1, None), ("league", 2, None), ("greedy", 1, None), ("greedy", 2, None)]    # (neither ever takes the one-launch step)


class _RolloutCase:
    """the smallest rollout of test_fused_rollout_metrics_equal_the_oracle_replay (40 x 4, n_hist 2, 5-step episodes, 14 steps: ends fall inside every rollout), its
    greedy chains, or a league's (PolicyBank, 64 x 8): an env, the driver of its chains, the oracle twin and the host-side tallies"""
    T, max_step, cash, seed = 14, 5, 20000, 880

    def __init__(self, kind, one_launch=None, monkeypatch=None, oracle=True):
        from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
        from episode_metrics_util import OracleEpisodeMetrics
        if one_launch is not None:
            monkeypatch.setenv("CDA_POLICY_STEP", one_launch)
        self.kind, self.greedy = kind, kind == "greedy"
        self.module_of, self.n_mod = None, 1
        if kind == "league":
            from gym_continuousdoubleauction_amd.league import LeagueSlotMapper
            self.N, self.A, k = 64, 8, 2
            self.cfg = _cfg(self.A, self.max_step, self.cash)
            self.env = CDAVecEnv(self.cfg, n_markets=self.N, with_info=False)
            self.env.reset(seed=self.seed)
            bank = mlp.PolicyBank("cuda:0", self.N, self.A, k, max_frozen=4, seed=5, random_seed=9)
            mapper = LeagueSlotMapper(self.A, k, self.A - k, 1.0, 3.0)
            net_of = {}
            for _ in range(2):
                cid = mapper.add_champion()
                net_of[cid] = bank.snapshot(0)
            slot_pool = torch.full((self.N, self.A), -1, dtype=torch.int32, device="cuda:0")
            mapper.assign_device(bank, episode_ids=[f"e0-m{i}" for i in range(self.N)], net_of=net_of, slot_pool=slot_pool)
            self.module_of = torch.where(slot_pool < 0, torch.arange(self.A, device="cuda:0", dtype=torch.int32).expand(self.N, self.A), slot_pool + k).to(torch.int32).contiguous()
            self.n_mod, self.driver = len(mapper.available_modules), bank
        else:
            self.N, self.A = 40, 4
            self.cfg = _cfg(self.A, self.max_step, self.cash, n_hist=2)
            self.env = CDAVecEnv(self.cfg, n_markets=self.N, with_info=False)
            self.env.reset(seed=self.seed)
            self.driver = mlp.FusedPolicy("cuda:0", seed=3, n_hist=2)
        self.ora = _oracle(self.cfg, self.N, self.seed) if oracle else None
        self.em = OracleEpisodeMetrics(self.N, self.A, self.cash) if oracle else None

    def chains(self, groups, seed=17, use_graphs=True):
        from gym_continuousdoubleauction_amd import mlp
        return mlp.RolloutChains(self.env, self.driver, self.T, groups=groups, seed=seed, greedy=self.greedy, use_graphs=use_graphs)

    def run(self, roll):
        """one rollout on the device, the same actions through the oracle; returns the rollout's buffers on the host"""
        b = {k: v.cpu().numpy().copy() for k, v in roll.run().items()}
        torch.cuda.synchronize()
        if self.ora is not None:
            _replay(self.ora, self.em, [tuple(b[k][t] for k in ACTION_KEYS) for t in range(self.T)])
        return b

    def oracle_enable(self):
        """include/cda.h, an episode in flight at cda_episode_metrics_enable: the running tallies restart from zero, the episode's step count goes on (the
        header's t_step), its end-of-episode account figures are the whole episode's; nothing that ended while the metrics were off was credited"""
        em = self.em
        em.term_sum[:] = 0; em.term_sq[:] = 0; em.ret[:] = 0; em.cnt[:] = 0
        em.F[:] = 0; em.M[:] = 0; em.violating.clear()
        return em.steps.copy()

    def collect(self):
        dev = [t.cpu().numpy() for t in (self.env.collect_episode_metrics() if self.module_of is None else
                                         self.env.collect_episode_metrics(module_of=self.module_of, n_modules=self.n_mod))]
        return dev

    def reference(self):
        return self.em.table(None if self.module_of is None else self.module_of.cpu().numpy(), self.n_mod)

    def close(self):
        self.env.close()
        if self.ora is not None:
            self.ora.close()


def _assert_zero_tables(dev, what):
    assert not dev[0].any() and not dev[1].any(), (what, dev[1])


@pytest.mark.parametrize("kind,groups,one_launch", ROLLOUT_CASES)
def test_a_captured_rollout_refuses_a_changed_metrics_setting(kind, groups, one_launch, monkeypatch):
    """The step instance (tallying or not) and the tolerance are arguments frozen into the captured graphs.  Captured with the metrics off and replayed after an enable
    the rollout tallied nothing: collect returned zero episodes and the strict NAV check passed with nothing checked.  run() now refuses, as for the tape, the scripts,
    the schedule, the quotes and the label tap - enable after capture, disable after capture, a changed nav_tolerance alone - and a FRESH RolloutChains on the same
    env then tallies: its tables are the oracle replay's, with a non-zero episode count"""
    from gym_continuousdoubleauction_amd import _capi as K
    from episode_metrics_util import assert_tables_equal
    c = _RolloutCase(kind, one_launch, monkeypatch)
    if one_launch is not None:
        from gym_continuousdoubleauction_amd._lib import lib
        assert lib().cda_policy_step_supported(c.env._h) == 1                   # ("2": the one-launch step wherever supported - this env is; "0": never)
    roll = c.chains(groups)
    c.run(roll)                                                                  # the capture: metrics off
    assert roll.graphs is not None
    c.env.enable_episode_metrics(True)
    in_flight = c.oracle_enable()
    with pytest.raises(RuntimeError, match="episode metrics"):
        roll.run()
    with pytest.raises(RuntimeError, match="episode metrics"):                  # (and again: the refusal is no one-off)
        roll.run()
    _assert_zero_tables(c.collect(), "nothing ran, nothing was credited")
    assert (in_flight > 0).any()                                                 # episodes are under way at the enable: credited at their end by the in-flight rule
    fresh = c.chains(groups, seed=23)
    c.run(fresh)                                                                 # captured with the metrics on
    dev, ref = c.collect(), c.reference()
    assert dev[1][K.EM_ENV_EPISODES] >= 2 * c.N and dev[0][:, K.EM_EPISODES].sum() >= 2 * c.N * c.A      # the count the replayed off-graphs left at zero
    assert_tables_equal(dev[0], dev[1], *ref, what="fresh chains after the refusal")
    c.env.enable_episode_metrics(False)                                          # the reverse order: captured on, replayed off
    with pytest.raises(RuntimeError, match="episode metrics"):
        fresh.run()
    c.env.enable_episode_metrics(True, nav_tolerance=1e-3)                       # on again, but with another tolerance: the graphs hold 1e-6
    with pytest.raises(RuntimeError, match="nav_tolerance"):
        fresh.run()
    assert (c.env.flags() == 0).all()
    c.close()


@pytest.mark.parametrize("kind,groups,one_launch", ROLLOUT_CASES)
def test_a_toggle_there_and_back_keeps_the_captured_rollout(kind, groups, one_launch, monkeypatch):
    """evaluate() enables the metrics on a caller's env and puts the caller's setting back: the SETTING is what the graphs hold, so chains captured before stay valid.
    Off: the next rollout is bit for bit, in every buffer, the one of a twin env that was never toggled.  On: the tables are the oracle replay's under the in-flight
    rule of include/cda.h - every episode that started after the second enable whole, the ones under way at it with the tallies of their remaining steps"""
    from gym_continuousdoubleauction_amd import _capi as K
    from episode_metrics_util import assert_tables_equal
    c, twin = _RolloutCase(kind, one_launch, monkeypatch), _RolloutCase(kind, one_launch, monkeypatch, oracle=False)
    roll, roll_twin = c.chains(groups), twin.chains(groups)
    first, first_twin = c.run(roll), twin.run(roll_twin)
    assert all(np.array_equal(first[k].view(np.uint8), first_twin[k].view(np.uint8)) for k in first)
    c.env.enable_episode_metrics(True)                                           # what evaluate() does to an env whose metrics are off ...
    c.env.enable_episode_metrics(False)                                          # ... and its finally clause
    second, second_twin = c.run(roll), twin.run(roll_twin)
    assert set(second) == set(second_twin) and len(second) >= 13
    for k in second:
        assert np.array_equal(second[k].view(np.uint8), second_twin[k].view(np.uint8)), (k, "the toggled env's rollout left its twin's")
    assert not np.array_equal(second["reward"], first["reward"])
    for i in (0, c.N - 1):
        assert bytes(c.env.get_state(i)) == bytes(twin.env.get_state(i))
    _assert_zero_tables(c.collect(), "off again: nothing tallied")
    twin.close()
    # the on setting: captured on, toggled off and on again with the same tolerance
    c.env.enable_episode_metrics(True)
    c.oracle_enable()
    on = c.chains(groups, seed=29)
    c.run(on)
    dev, ref = c.collect(), c.reference()
    assert_tables_equal(dev[0], dev[1], *ref, what="the capturing rollout")
    c.env.enable_episode_metrics(False)
    c.env.enable_episode_metrics(True)
    in_flight = c.oracle_enable()
    assert (in_flight > 0).any()
    c.run(on)                                                                    # not refused
    dev, ref = c.collect(), c.reference()
    assert dev[1][K.EM_ENV_EPISODES] >= 2 * c.N
    assert_tables_equal(dev[0], dev[1], *ref, what="after the toggle there and back")
    c.close()


@pytest.mark.parametrize("kind,groups,one_launch", [("shared", 2, "2"), ("shared", 1, "0"), ("league", 2, None), ("greedy", 1, None)])
def test_direct_launch_chains_follow_the_setting_and_an_episode_in_flight_is_credited_by_the_rule(kind, groups, one_launch, monkeypatch):
    """use_graphs=False freezes nothing: every run() launches with the env's setting of that moment.  Pins include/cda.h's rule for an episode under way at an enable:
    credited at its end, its tallies those of the steps after the enable, its step count and account figures the whole episode's"""
    from gym_continuousdoubleauction_amd import _capi as K
    from episode_metrics_util import assert_tables_equal
    c = _RolloutCase(kind, one_launch, monkeypatch)
    roll = c.chains(groups, use_graphs=False)
    c.run(roll)                                                                  # off
    _assert_zero_tables(c.collect(), "off")
    c.env.enable_episode_metrics(True)
    in_flight = c.oracle_enable()
    assert roll.graphs is None and (in_flight == c.T % c.max_step).sum() >= c.N // 2      # most markets are 4 steps into a 5-step episode
    c.run(roll)
    dev, ref = c.collect(), c.reference()
    assert dev[1][K.EM_ENV_EPISODES] >= 2 * c.N
    assert_tables_equal(dev[0], dev[1], *ref, what="on: follows the enable")
    # the in-flight episodes' steps count whole: the credited steps and the ones still under way are the rollout's plus what had run before the enable
    assert dev[1][K.EM_ENV_STEPS] + c.em.steps.sum() == c.N * c.T + in_flight.sum()
    c.env.enable_episode_metrics(False)
    c.run(roll)
    _assert_zero_tables(c.collect(), "off again: follows the disable")
    c.env.enable_episode_metrics(True, nav_tolerance=1e-3)
    c.oracle_enable()
    c.run(roll)
    dev, ref = c.collect(), c.reference()
    assert_tables_equal(dev[0], dev[1], *ref, what="on again, another tolerance")
    assert (c.env.flags() == 0).all()
    c.close()


def _ends(roll):
    return int((roll.buf["terminated"] | roll.buf["truncated"]).sum().item())


def test_a_training_loop_without_metrics_turns_them_off_on_an_env_that_has_them_on():
    """train_fused / train_league_fused(episode_metrics=False) on an env whose metrics are on: nothing would collect what the tallying kernels accumulate, so the
    loops set the state they were asked for - off - before their chains capture, and nothing accumulates"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, ppo
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    quiet = dict(iters=1, horizon=5, epochs=1, chains=2, log=lambda s: None, episode_metrics=False)
    for A in (4, 8):
        env = CDAVecEnv(_cfg(A, 5, 20000), n_markets=64, with_info=False)
        env.reset(seed=3)
        env.enable_episode_metrics(True, nav_tolerance=1e-3)
        keep = {}
        out = (ppo.train_fused(env, keep=keep, **quiet) if A == 4 else train_league_fused(env, num_trainable=2, keep=keep, **quiet))
        history = out[-1]
        assert _ends(keep["rollout"]) >= 64                                      # episodes did end during the loop
        assert env.episode_metrics_on is False and "episode_metrics" not in history[0]
        _assert_zero_tables([t.cpu().numpy() for t in env.collect_episode_metrics()], f"{A} agents: accumulated during a loop that collects nothing")
        env.close()


def test_a_data_parallel_loop_refuses_an_allreduce_that_can_only_sum():
    """the ranks' tables hold MIN and MAX columns: a callable without op= is refused by both loops before anything runs (never summed); without episode metrics
    the same callable is taken, as before"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, ppo
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    quiet = dict(iters=1, horizon=5, epochs=1, chains=2, log=lambda s: None, allreduce=lambda t: t, world=2)
    env = CDAVecEnv(_cfg(4, 5, 20000), n_markets=64, with_info=False)
    host_epoch = env.host_epoch
    with pytest.raises(TypeError, match="min"):
        ppo.train_fused(env, **quiet)
    with pytest.raises(TypeError, match="min"):
        train_league_fused(env, num_trainable=2, **quiet)
    assert env.host_epoch == host_epoch and not getattr(env, "episode_metrics_on", False)      # not reset, not enabled: refused first
    _, history = ppo.train_fused(env, episode_metrics=False, **quiet)
    assert len(history) == 1 and "episode_metrics" not in history[0]
    env.close()


def test_train_fused_reports_every_episode_end_of_its_rollouts():
    """episode_metrics=True on an env that comes with them off: history[i]["episode_metrics"]["episodes"] is the number of episode ends in iteration i's
    terminated | truncated buffers (8-step rollouts over 5-step episodes: three ends per market over the two, early terminations on top)"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, ppo
    env = CDAVecEnv(_cfg(4, 5, 3000), n_markets=64, with_info=False)
    keep, ends = {}, []
    _, history = ppo.train_fused(env, iters=2, horizon=8, epochs=1, chains=2, keep=keep, log=lambda s: ends.append(_ends(keep["rollout"])), episode_metrics=True)
    assert env.episode_metrics_on is True and len(ends) == 2 and min(ends) >= 64 and sum(ends) >= 3 * 64
    assert [h["episode_metrics"]["episodes"] for h in history] == ends
    assert all(h["episode_metrics"]["nav_conservation_violations"] == 0 for h in history) and (env.flags() == 0).all()
    env.close()


def test_evaluate_puts_the_callers_tolerance_back():
    """evaluate() on an env with enable_episode_metrics(True, nav_tolerance=1e-3): afterwards the setting is the caller's, tolerance included - a ledger fault of
    1e-4 seeded after the call (the recipe of test_a_ledger_fault_in_an_episode_that_auto_resets_mid_run_is_reported) is within it and is not flagged"""
    from decimal import Decimal
    from gym_continuousdoubleauction_amd import CDAVecEnv, _capi as K, mlp
    from gym_continuousdoubleauction_amd import episode_metrics as EM
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    N, A, max_step, victim = 64, 4, 6, 37
    env = CDAVecEnv(_cfg(A, max_step), n_markets=N, with_info=False)
    env.reset(seed=99)
    env.enable_episode_metrics(True, nav_tolerance=1e-3)
    res = evaluate(env, mlp.FusedPolicy("cuda:0", seed=3), episodes=1, seed=1, groups=2)
    assert res["episodes"] >= N
    assert env.episode_metrics_on is True and env.episode_metrics_tolerance == 1e-3
    env.reset(seed=99)
    env.collect_episode_metrics()
    rng = np.random.default_rng(2)
    for _ in range(2):
        env.step(*_actions(rng, N, A))
    st = env.get_state(victim)
    for field in ("cash", "nav", "prev_nav", "max_nav"):                        # agent 2 finds a hundredth of a cent that nobody lost: inside 1e-3, outside 1e-6
        d = getattr(st.acc[2], field)
        setattr(st.acc[2], field, K.decimal_to_dec(K.dec_to_decimal(d) + Decimal("0.0001")))
    env.set_state(victim, st)
    for _ in range(max_step + 2):
        env.step(*_actions(rng, N, A))
    torch.cuda.synchronize()
    assert not (env.flags().cpu().numpy() & K.FLAG_NAV_CONSERVATION).any()
    s = EM.summarise(*env.collect_episode_metrics())
    assert s["episodes"] >= N and s["nav_conservation_violations"] == 0 and s["nav_conservation_error"] == 1e-4      # seen, and within the caller's tolerance
    EM.check_nav_conservation(0, s, strict=True)
    env.close()


def test_shard_tables_merge_into_the_union_envs_table():
    """episode_metrics.merge_tables against the device's own reduction: env U steps 2N markets, S0 and S1 its halves (markets are seeded by global index and independent,
    so U's records ARE the shards': asserted on the state dumps).  Three modules, one of them only in S0's markets.  merge([S0's tables, S1's]) is U's table: integer,
    min and max columns bit for bit, the f64 sums within the order bound (U adds its rows in another order than the two shards and the host)"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, _capi as K
    from gym_continuousdoubleauction_amd import episode_metrics as EM
    from episode_metrics_util import OracleEpisodeMetrics, abs_sums, assert_summary_is_consistent, assert_tables_within_order_bound
    N, A, max_step, T, seed, cash, n_mod = 32, 4, 5, 14, 640, 3000, 3
    cfg = _cfg(A, max_step, cash)
    envs = [CDAVecEnv(cfg, n_markets=n, with_info=False) for n in (2 * N, N, N)]
    for env, s in zip(envs, (seed, seed, seed + N)):
        env.reset(seed=s)
        env.enable_episode_metrics(True)
    U, S0, S1 = envs
    rng = np.random.default_rng(12)
    steps = [_actions(rng, 2 * N, A, aggressive=True) for _ in range(T)]
    for acts in steps:
        U.step(*acts)
        S0.step(*(x[:N] for x in acts))
        S1.step(*(x[N:] for x in acts))
    for i in range(2 * N):
        assert bytes(U.get_state(i)) == bytes((S0 if i < N else S1).get_state(i % N)), i
    module_of = ((np.arange(2 * N)[:, None] + np.arange(A)[None, :]) % 2).astype(np.int32)
    module_of[:N:3, 0] = 2                                                        # module 2 plays in the first shard's markets only
    tables = []
    for env, rows in ((U, slice(0, 2 * N)), (S0, slice(0, N)), (S1, slice(N, 2 * N))):
        mo = torch.from_numpy(np.ascontiguousarray(module_of[rows])).to(env.device)
        tables.append([t.cpu().numpy() for t in env.collect_episode_metrics(module_of=mo, n_modules=n_mod)])
    union, shard0, shard1 = tables
    assert shard0[0][2, K.EM_EPISODES] > 0 and not shard1[0][2].any()
    assert not np.array_equal(shard0[0], union[0]) and not np.array_equal(shard1[0], union[0]) and min(shard0[1][0], shard1[1][0]) >= 2 * N and shard0[1][0] + shard1[1][0] == union[1][0]
    merged = EM.merge_tables([shard0, shard1])
    ora, em = _oracle(cfg, 2 * N, seed), OracleEpisodeMetrics(2 * N, A, cash)     # (the oracle's rows give the bound its scale - and hold U itself to the replay)
    _replay(ora, em, steps)
    sums = abs_sums(em, module_of, n_mod)
    ref = em.table(module_of, n_mod)
    assert em.F is not None and ref[0][:, K.EM_TRADES].sum() > 100 and ref[0][:, K.EM_MAKER_RATIO_N].sum() > 0
    worst = assert_tables_within_order_bound(merged[0], merged[1], union[0], union[1], sums, what="merge of the shards against the union env")
    worst_ref = assert_tables_within_order_bound(union[0], union[1], *ref, sums, what="the union env against the oracle")
    print(f"\n[merge of shard tables] worst f64 sum error / (2 n eps sum|x|): merged vs union {worst:.3g}, union vs oracle {worst_ref:.3g}")
    assert_summary_is_consistent(EM.summarise(*merged), "merged shards")
    naive = (shard0[0] + shard1[0], shard0[1] + shard1[1])                        # a SUM over the shards is NOT the union's table
    assert naive[0][0, K.EM_NAV_MIN] != union[0][0, K.EM_NAV_MIN] and naive[0][0, K.EM_NAV_MAX] != union[0][0, K.EM_NAV_MAX]
    for env in envs:
        assert (env.flags() == 0).all()
        env.close()
    ora.close()
