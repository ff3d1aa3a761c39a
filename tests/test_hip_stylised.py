"""GPU: the stylised-facts report (include/cda.h cda_quote_returns, cda_tape_signs, cda_tape_flow_returns; CDAVecEnv.quote_returns / tape_signs /
tape_flow_returns).  The device must equal the numpy specification (gym_continuousdoubleauction_amd/stylised.py, which tests/test_stylised_host.py pins to a
plain-loop restatement) WORD FOR WORD, with the specification fed from host dumps of the same rings: quote_series and tape_last.  Integers only: every comparison
is exact.  The main run's seed was chosen with the CPU oracle so that a market has more than one pass (64) of fills and of defined returns, a missing return and
clipped histogram mass; the test asserts all four from the dumps."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_hip_tape import _actions

pytestmark = pytest.mark.gpu

N, A, MAX_STEP, STEPS = 16, 8, 80, 200                             # two and a half episodes: a complete previous one, a shorter current one
SEED = 0                                                           # reset seeds 900 + SEED ..., actions default_rng(SEED)
LAGS, FLOW_LAGS, BARS, HIST_HALF = (1, 2, 8, 70), (0, 1, 5), (1, 3), 2
INVALID, UNSUPPORTED = -1, -4


def _np(t):
    return t.cpu().numpy()


def _env(n=N, a=A, max_step=MAX_STEP, quote_cap=128, tape_cap=512, rows=None, **kw):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    cfg = dict({"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}, **kw)
    env = CDAVecEnv(cfg, n_markets=n, device="cuda:0", with_info=False, market_configs=rows)
    env.enable_tape(tape_cap)
    env.enable_quotes(quote_cap)
    return env


def _play(env, steps, seed=SEED):
    env.reset(seed=np.arange(900 + seed, 900 + seed + env.n_markets, dtype=np.uint64))
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        env.step(*_actions(rng, env.n_markets, env.num_agents))


def _dumps(env, which):
    """the host dumps the specification is fed from: per market (quote rows, quotes' info row, tape rows, tape records lost)"""
    qrec, qcnt, qinfo = (_np(x) for x in env.quote_series(episode=which))
    trec, tcnt = (_np(x) for x in env.tape_last(env.tape_capacity, episode=which))
    total = _np(env.tape_counts()["n_episode" if which == "current" else "n_previous"])
    return [(qrec[m, :qcnt[m]], qinfo[m], trec[m, :tcnt[m]], int(total[m]) - int(tcnt[m])) for m in range(env.n_markets)]


def _ticks(env):
    return env.market_rows()["tick_size"].astype(np.int64) if env.per_market else np.full(env.n_markets, int(env.config.get("tick_size", 1)), np.int64)


def _check(env, tag, lags=LAGS, flow_lags=FLOW_LAGS, bars=BARS, hist_half=HIST_HALF):
    """all three reductions of both remembered episodes against the specification on the dumps; what the dumps held, for the callers' coverage assertions"""
    from gym_continuousdoubleauction_amd import stylised as SF
    ticks, n = _ticks(env), env.n_markets
    seen = {"fills": 0, "returns": 0, "missing": 0, "ends": 0, "quotes_lost": 0, "tape_lost": 0, "bars_excluded": 0, "all_lost": 0, "lag_pairs": 0, "flow_n": 0}
    for which in ("current", "previous"):
        dumps = _dumps(env, which)
        sbase, slag, sinfo = (_np(x) for x in env.tape_signs(lags, episode=which))
        assert sbase.dtype == np.int64 and sbase.shape == (n, 8) and slag.shape == (n, len(lags), 4) and sinfo.dtype == np.int32 and sinfo.shape == (n, 4)
        for m, (q, qinfo, t, tlost) in enumerate(dumps):
            want = SF.signs_from_records(t, lags)
            assert np.array_equal(sbase[m], want[0]) and np.array_equal(slag[m], want[1]), (tag, which, m, sbase[m], want[0], slag[m], want[1])
            assert sinfo[m].tolist() == [len(t), tlost, 0, 0], (tag, which, m, sinfo[m], len(t), tlost)
            seen["fills"] = max(seen["fills"], len(t)); seen["tape_lost"] += tlost; seen["lag_pairs"] += int(want[1][:, 0].sum())
        for bar in bars:
            rbase, rlag, rhist, rinfo = (_np(x) for x in env.quote_returns(lags, bar, hist_half, episode=which))
            flag, fbase, finfo = (_np(x) for x in env.tape_flow_returns(flow_lags, bar, episode=which))
            assert rbase.shape == (n, 8) and rlag.shape == (n, len(lags), 4) and rhist.shape == (n, 2 * hist_half + 1) and rhist.dtype == np.int64
            assert flag.shape == (n, len(flow_lags), 6) and fbase.shape == (n, 4) and flag.dtype == np.int64
            for m, (q, qinfo, t, tlost) in enumerate(dumps):
                ctx = (tag, which, bar, m)
                want = SF.returns_from_quotes(q, lags, bar, hist_half, int(ticks[m]))
                for got, w, name in zip((rbase[m], rlag[m], rhist[m]), want, ("base", "lagged", "hist")):
                    assert np.array_equal(got, w), (ctx, name, got, w)
                assert np.array_equal(rinfo[m], qinfo), (ctx, rinfo[m], qinfo)
                wl, wb = SF.flow_returns_from_records(t, q, flow_lags, bar, tlost)
                assert np.array_equal(flag[m], wl) and np.array_equal(fbase[m], wb), (ctx, flag[m], wl, fbase[m], wb)
                assert finfo[m].tolist() == [len(t), tlost, int(qinfo[1]), 0], (ctx, finfo[m])
                if bar == 1:
                    seen["returns"] = max(seen["returns"], int(want[0][1])); seen["missing"] += int(want[0][2]); seen["ends"] += int(want[2][0] + want[2][-1])
                    seen["quotes_lost"] += int(qinfo[1])
                seen["bars_excluded"] += int(wb[2]); seen["all_lost"] += int(tlost > 0 and len(t) == 0); seen["flow_n"] += int(wl[:, 0].sum())
    return seen


def _clean(env, flags_before=None):
    flags = _np(env.flags())
    assert (_np(env.check_invariants()) == 0).all()
    assert (flags == 0).all() if flags_before is None else np.array_equal(flags, flags_before)


# ---- 1. the main run: rings that hold both episodes ------------------------------------------------------------------------------------------
def test_the_three_reductions_equal_the_specification_on_both_episodes():
    from gym_continuousdoubleauction_amd import quotes as Q
    from gym_continuousdoubleauction_amd import stylised as SF
    env = _env()
    _play(env, STEPS)
    seen = _check(env, "main")
    # not vacuous, from the dumps: more than one pass of fills and of defined returns, a missing return, clipped mass, nothing lost, lags that find pairs
    assert seen["fills"] > 64 and seen["returns"] > 64 and seen["missing"] > 0 and seen["ends"] > 0, seen
    assert seen["quotes_lost"] == 0 and seen["tape_lost"] == 0 and seen["bars_excluded"] == 0 and seen["lag_pairs"] > 0 and seen["flow_n"] > 0, seen
    # the identities with quote_stats at one-step bars, on the device's own words
    for which in ("current", "previous"):
        base, _, hist, _ = (_np(x) for x in env.quote_returns((1,), 1, HIST_HALF, episode=which))
        stats = _np(env.quote_stats(episode=which)[0])
        assert np.array_equal(base[:, SF.RET["returns"]], stats[:, Q.STAT["pairs"]]) and np.array_equal(base[:, SF.RET["sum_r2"]], stats[:, Q.STAT["dm2_sq"]])
        assert np.array_equal(base[:, SF.RET["sum_abs"]], stats[:, Q.STAT["abs_dm2"]]) and np.array_equal(hist.sum(axis=1), base[:, SF.RET["returns"]])
    # a sub-range is the same rows; pool stays on the device and is the plain sum
    whole = env.tape_flow_returns(FLOW_LAGS, 3, episode="previous")
    part = env.tape_flow_returns(FLOW_LAGS, 3, episode="previous", first_market=5, n_markets=6)
    assert all(torch.equal(p, w[5:11]) for p, w in zip(part, whole))
    pooled = SF.pool(whole[0])
    assert pooled.is_cuda and torch.equal(pooled, whole[0].sum(dim=0)) and np.array_equal(SF.pool(_np(whole[0])), _np(pooled))
    _clean(env)
    env.close()


# ---- 2. rings smaller than the episode: lost heads, the info words, bars_excluded ------------------------------------------------------------
def test_rings_smaller_than_the_episode_report_what_they_lost():
    env = _env(quote_cap=32, tape_cap=16)
    _play(env, STEPS)
    seen = _check(env, "small rings")
    assert seen["quotes_lost"] > 0 and seen["tape_lost"] > 0 and seen["bars_excluded"] > 0 and seen["all_lost"] > 0 and seen["flow_n"] > 0, seen
    _clean(env)
    env.close()


# ---- 3. per-market ticks: the histogram divides by the market's own ---------------------------------------------------------------------------
def test_the_histogram_is_in_the_market_s_own_ticks():
    rows = [{"tick_size": 1 if m % 2 == 0 else 5} for m in range(N)]
    env = _env(rows=rows)
    assert env.per_market and sorted(set(_ticks(env).tolist())) == [1, 5]
    _play(env, MAX_STEP + 30)
    seen = _check(env, "ticks", bars=(1,), hist_half=3)
    assert seen["returns"] > 64 and seen["ends"] > 0, seen
    _clean(env)
    env.close()


# ---- 4. the border: 4096 bar points ------------------------------------------------------------------------------------------------------------
def _raw(env, name, first, n, which, lags, *mid_and_outs):
    from gym_continuousdoubleauction_amd._lib import lib
    return getattr(lib(), name)(env._h, first, n, which, (C.c_int32 * max(1, len(lags)))(*lags), len(lags), *mid_and_outs, env._stream())


def test_an_episode_of_8192_steps_needs_two_step_bars():
    env = _env(n=6, a=4, max_step=8192, quote_cap=64, tape_cap=256)
    _play(env, 40)
    for call in (env.quote_returns, env.tape_flow_returns):
        with pytest.raises(ValueError, match="bar points"):
            call(bar_steps=1)
    out = [torch.zeros(6 * 64, dtype=torch.int64, device="cuda:0") for _ in range(3)]
    ptr = [o.data_ptr() for o in out]
    assert _raw(env, "cda_quote_returns", 0, 6, 0, (1,), 1, 2, ptr[0], ptr[1], ptr[2], None) == INVALID
    assert _raw(env, "cda_tape_flow_returns", 0, 6, 0, (1,), 1, ptr[0], ptr[1], None) == INVALID
    assert _raw(env, "cda_quote_returns", 0, 6, 0, (1,), 2, 2, ptr[0], ptr[1], ptr[2], None) == 0          # 4096 points: accepted (info may be NULL)
    assert _raw(env, "cda_tape_flow_returns", 0, 6, 0, (1,), 2, ptr[0], ptr[1], None) == 0
    torch.cuda.synchronize()
    seen = _check(env, "border", lags=(1, 3), flow_lags=(0, 2), bars=(2, 5))
    assert seen["flow_n"] > 0 and seen["lag_pairs"] > 0, seen
    _clean(env)
    env.close()


def test_the_entry_points_refuse_bad_arguments_on_a_live_env():
    env = _env(n=4, a=4, max_step=32, quote_cap=16, tape_cap=16)
    _play(env, 8)
    out = [torch.zeros(4 * 64 + 1, dtype=torch.int64, device="cuda:0") for _ in range(3)]
    p = [o.data_ptr() for o in out]
    info = torch.zeros(17, dtype=torch.int32, device="cuda:0").data_ptr()
    good = {"cda_quote_returns": (1, 2, p[0], p[1], p[2], info), "cda_tape_signs": (p[0], p[1], info), "cda_tape_flow_returns": (1, p[0], p[1], info)}
    for name, rest in good.items():
        assert _raw(env, name, 0, 4, 0, (1, 2), *rest) == 0 and _raw(env, name, 1, 3, 1, (1, 2), *rest) == 0, name
        for first, n, which, lags in ((0, 5, 0, (1,)), (-1, 2, 0, (1,)), (0, 0, 0, (1,)), (4, 1, 0, (1,)), (0, 4, 2, (1,)), (0, 4, -1, (1,)), (0, 4, 0, ()), (0, 4, 0, (1,) * 9),
                                      (0, 4, 0, (-1,)), (0, 4, 0, ((1 << 20) + 1,))):
            assert _raw(env, name, first, n, which, lags, *rest) == INVALID, (name, first, n, which, lags)
        assert _raw(env, name, 0, 4, 0, (0,), *rest) == (0 if name == "cda_tape_flow_returns" else INVALID), name
        outs = len(rest) - (2 if name == "cda_quote_returns" else 1 if name == "cda_tape_flow_returns" else 0)
        for k in range(len(rest) - outs, len(rest)):                # every output: NULL (info alone may be), misaligned
            is_info = k == len(rest) - 1
            assert _raw(env, name, 0, 4, 0, (1,), *rest[:k], None, *rest[k + 1:]) == (0 if is_info else INVALID), (name, k)
            assert _raw(env, name, 0, 4, 0, (1,), *rest[:k], rest[k] + (2 if is_info else 4), *rest[k + 1:]) == INVALID, (name, k)
    assert _raw(env, "cda_quote_returns", 0, 4, 0, (1,), 0, 2, p[0], p[1], p[2], info) == INVALID and _raw(env, "cda_tape_flow_returns", 0, 4, 0, (1,), 0, p[0], p[1], info) == INVALID
    for hh in (0, 65):
        assert _raw(env, "cda_quote_returns", 0, 4, 0, (1,), 1, hh, p[0], p[1], p[2], info) == INVALID
    torch.cuda.synchronize()
    env.disable_quotes()
    assert _raw(env, "cda_quote_returns", 0, 4, 0, (1,), *good["cda_quote_returns"]) == UNSUPPORTED
    assert _raw(env, "cda_tape_flow_returns", 0, 4, 0, (1,), *good["cda_tape_flow_returns"]) == UNSUPPORTED and _raw(env, "cda_tape_signs", 0, 4, 0, (1,), *good["cda_tape_signs"]) == 0
    with pytest.raises(RuntimeError, match="enable_quotes"):
        env.quote_returns()
    env.disable_tape()
    assert _raw(env, "cda_tape_signs", 0, 4, 0, (1,), *good["cda_tape_signs"]) == UNSUPPORTED
    torch.cuda.synchronize()
    _clean(env)
    env.close()


# ---- 5. random configurations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(6))
def test_the_reductions_on_a_random_service_configuration(index):
    import fuzz_cases as F
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from services_fuzz_util import TAPE_CAPACITY
    case = F.service_cases(F.SERVICE_SEED, index + 1)[index]
    cfg, n, a, rows = case["cfg"], case["n_markets"], case["cfg"]["num_of_agents"], case["rows"]
    env = CDAVecEnv(cfg, n_markets=n, device="cuda:0", with_info=False, market_configs=[rows[m % len(rows)] for m in range(n)] if rows else None)
    env.enable_tape(TAPE_CAPACITY)
    env.enable_quotes(F.service_extras(case)["quote_capacity"])
    rng = np.random.default_rng(case["seed"])
    env.reset(seed=rng.integers(0, 2 ** 63, n).astype(np.uint64))
    for _ in range(F.SERVICE_STEPS + F.SERVICE_STEPS_AFTER):
        acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
        env.step(*acts, present)
    flags = _np(env.flags())
    seen = _check(env, f"case {index} {cfg} rows={rows}", lags=(1, 3, 64, 65), flow_lags=(0, 1, 4), bars=(1, case["bar_steps"]), hist_half=1 + index * 12)
    assert seen["lag_pairs"] > 0 or seen["fills"] < 2, seen
    _clean(env, flags)
    env.close()


# ---- 6. evaluate ---------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_reports_the_stylised_facts_of_the_tapes_it_kept(tmp_path):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd import quotes as Q
    from gym_continuousdoubleauction_amd import stylised as SF
    from gym_continuousdoubleauction_amd import tape as T
    from gym_continuousdoubleauction_amd.evaluate import STYLISED_HIST_HALF, evaluate
    n, a, episodes, max_step, lags, bar = 32, 4, 2, 72, (1, 2, 5), 2      # (one rollout per episode: the saved tape's episode ids are exact)
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}, n_markets=n, with_info=False)
    pol = mlp.FusedPolicy("cuda:0", seed=5)
    for bad in ({"stylised_facts": ()}, {"stylised_facts": (0, 1)}, {"stylised_facts": (1,), "bar_steps": 0}):
        with pytest.raises(ValueError):
            evaluate(env, pol, opponents=["random"], episodes=episodes, seed=3, **bad)
    qpath, tpath, keep = str(tmp_path / "quotes.npz"), str(tmp_path / "tape.npz"), {}
    res = evaluate(env, pol, opponents=["random", "maker"], trained_slots=1, episodes=episodes, seed=3, tape=tpath, quotes=qpath, stylised_facts=lags, bar_steps=bar, keep=keep)
    assert not env.quotes_enabled and not env.tape_enabled
    z, tp = Q.load(qpath), T.load_tape(tpath)
    assert z["counts"].tolist() == [max_step] * n and not tp["dropped"].any()
    flow_lags = [0] + list(lags)
    want = [np.zeros(s, np.int64) for s in ((8,), (len(lags), 4), (2 * STYLISED_HIST_HALF + 1,), (8,), (len(lags), 4), (len(flow_lags), 6), (4,))]
    for m in range(n):
        t = tp["records"][(tp["market"] == m) & (tp["episode"] == episodes - 1)]      # every market's last finished episode
        q = z["records"][m, :z["counts"][m]]
        parts = SF.returns_from_quotes(q, lags, bar, STYLISED_HIST_HALF, 1) + SF.signs_from_records(t, lags) + SF.flow_returns_from_records(t, q, flow_lags, bar, 0)
        for acc, part in zip(want, parts):
            acc += part
    block = res["stylised_facts"]
    got = [np.array(block["rows"][k], np.int64) for k in ("returns", "returns_lagged", "returns_hist", "signs", "signs_lagged", "flows_lagged", "flows")]
    for g, w, name in zip(got, want, ("returns", "returns_lagged", "returns_hist", "signs", "signs_lagged", "flows_lagged", "flows")):
        assert np.array_equal(g, w), (name, g, w)
    assert want[0][1] > 0 and want[3][0] > 0 and want[5][0, 0] > 0
    about = block["about"]
    assert about["lags"] == list(lags) and about["flow_lags"] == flow_lags and about["bar_steps"] == bar and about["markets"] == n
    assert about["quotes_lost"] == 0 and about["tape_records_lost"] == 0 and about["tape_records"] == want[3][0] and about["quotes"] == n * max_step
    same = SF.summary(returns=want[:3], signs=want[3:5], flows=want[5:7], lags=lags, flow_lags=flow_lags, bar_steps=bar)
    assert block["signs"] == same["signs"] and block["flows"] == same["flows"] and block["returns"]["lags"] == same["returns"]["lags"]
    assert block["returns"]["variance_ratio"]["k"] == bar and set(block["flows"]["lags"]) == {"k0", "k1", "k2", "k5"}
    assert keep["stylised_tables"]["counted"].all() and np.array_equal(keep["stylised_tables"]["signs"][0].sum(axis=0), want[3])
    _clean(env)
    env.close()
