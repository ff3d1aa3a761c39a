"""GPU: the P&L report (include/cda.h cda_tape_pnl; CDAVecEnv.tape_pnl).  The device must equal the numpy specification (gym_continuousdoubleauction_amd/pnl.py,
which tests/test_pnl_host.py pins to a scalar restatement) WORD FOR WORD - the sixteen words per agent and the three series - with the specification fed from host
dumps of the same rings: quote_series and tape_last.  The cases are tests/pnl_cases.py DEVICE_CASES; the host test replays them on the CPU oracle and shows what
they hold, and the tests here assert the same from the dumps.  Integers only: every comparison is exact."""
import numpy as np
import pytest
import torch

import pnl_cases as PC

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
POISON64, POISON32 = -0x5a5a5a5a5a5a5a5b, -0x5a5a5a5b


def _np(t):
    return t.cpu().numpy()


def _env(n, a, max_step, tape_cap, quote_cap, **kw):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    cfg = dict({"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}, **kw)
    env = CDAVecEnv(cfg, n_markets=n, device="cuda:0", with_info=False)
    env.enable_tape(tape_cap)
    env.enable_quotes(quote_cap)
    return env


def _dumps(env, which):
    """the host dumps the specification is fed from: per market (quote rows, quotes' info row, tape rows, tape records lost)"""
    qrec, qcnt, qinfo = (_np(x) for x in env.quote_series(episode=which))
    trec, tcnt = (_np(x) for x in env.tape_last(env.tape_capacity, episode=which))
    total = _np(env.tape_counts()["n_episode" if which == "current" else "n_previous"])
    return [(qrec[m, :qcnt[m]], qinfo[m], trec[m, :tcnt[m]], int(total[m]) - int(tcnt[m])) for m in range(env.n_markets)]


def _seen():
    return dict.fromkeys(("stale", "unmarked", "open_fills", "self", "tape_lost", "quote_lost", "long", "fills", "bars"), 0)


def _check(env, tag, bars, seen=None):
    """stats and the three series of both remembered episodes against the specification on the dumps, and the identities on the device's own words"""
    from gym_continuousdoubleauction_amd import pnl as PN
    from gym_continuousdoubleauction_amd.stylised import n_points
    F, n, a = PN.PNL, env.n_markets, env.num_agents
    seen = _seen() if seen is None else seen
    top = int(env.market_rows()["max_step"].max()) if env.per_market else int(env.max_step)
    for which in ("current", "previous"):
        dumps = _dumps(env, which)
        for bar in bars:
            P = n_points(top, bar)
            stats, equity, position, marks, info = (_np(x) for x in env.tape_pnl(bar, which, series=True))
            alone, info2 = (_np(x) for x in env.tape_pnl(bar, which))
            assert stats.dtype == np.int64 and stats.shape == (n, a, 16) and equity.dtype == np.int64 and equity.shape == (n, a, P)
            assert position.dtype == np.int32 and position.shape == (n, a, P) and marks.dtype == np.int32 and marks.shape == (n, P) and info.shape == (n, 4)
            assert np.array_equal(alone, stats) and np.array_equal(info2, info), (tag, which, bar)
            for m, (q, qinfo, t, tlost) in enumerate(dumps):
                ctx = (tag, which, bar, m)
                want = PN.pnl_from_records(t, q, a, bar, n_points=P)
                for got, w, name in zip((stats[m], equity[m], position[m], marks[m]), want, ("stats", "equity", "position", "marks")):
                    assert got.dtype == w.dtype and np.array_equal(got, w), (ctx, name, got, w)
                assert info[m].tolist() == [len(t), tlost, int(qinfo[1]), 0], (ctx, info[m], len(t), tlost, qinfo)
                s = want[0]
                seen["stale"] += int(s[0, F["stale"]] > 0); seen["unmarked"] += int(s[0, F["unmarked"]] > 0); seen["open_fills"] += int(s[:, F["open_fills"]].sum() > 0)
                seen["self"] += int(len(t) and (t[:, 3] == t[:, 6]).any()); seen["tape_lost"] += int(tlost > 0); seen["quote_lost"] += int(qinfo[1] > 0)
                seen["long"] += int(s[0, F["points"]] > 128); seen["fills"] = max(seen["fills"], len(t)); seen["bars"] += int(s[0, F["bars"]])
            # the identities, on the device's own output
            assert np.array_equal(stats[..., F["inventory"]] + stats[..., F["trading"]], stats[..., F["equity_last"]] - stats[..., F["equity_first"]]), (tag, which, bar)
            assert np.array_equal(stats[..., F["bars"]], np.maximum(stats[..., F["points"]] - 1, 0)) and (stats[..., F["max_drawdown"]] >= 0).all()
            whole = np.array([d[3] == 0 for d in dumps])            # no lost tape head: the agents' equities sum to 0 at every point, and so do the two parts
            assert not equity[whole].sum(axis=1).any() and not stats[whole][..., F["inventory"]].sum(axis=1).any() and not stats[whole][..., F["trading"]].sum(axis=1).any()
            assert not position[whole].sum(axis=1).any()
    return seen


def _clean(env, flags_before=None):
    flags = _np(env.flags())
    assert (_np(env.check_invariants()) == 0).all()
    assert (flags == 0).all() if flags_before is None else np.array_equal(flags, flags_before)


def _play(env, c, seen=None):
    """the case's steps with a check at every stop"""
    env.reset(seed=PC.seeds(c))
    rng = np.random.default_rng(c["seed"])
    done = 0
    for stop in c["stops"]:
        for _ in range(stop - done):
            env.step(*PC.actions(rng, c["n"], c["a"]))
        done = stop
        seen = _check(env, (c["name"], stop), c["bars"], seen)
    return seen


# ---- 1. device == specification ----------------------------------------------------------------------------------------------------------------
def test_the_base_case_equals_the_specification_mid_episode_and_behind_the_auto_reset():
    from gym_continuousdoubleauction_amd import pnl as PN
    c = PC.case("base")
    assert (c["n"], c["a"], c["max_step"], c["stops"][0], c["bars"]) == (24, 4, 150, 100, (1, 7))
    env = _env(c["n"], c["a"], c["max_step"], c["tape_cap"], c["quote_cap"])
    seen = _play(env, c)
    # not vacuous, from the dumps: more than one pass of fills and more than two of points, stale and unmarked points, open fills, self-trades, nothing lost
    assert seen["fills"] > 64 and seen["long"] > 0 and seen["stale"] > 0 and seen["unmarked"] > 0 and seen["open_fills"] > 0 and seen["self"] > 0 and seen["bars"] > 0, seen
    assert seen["tape_lost"] == 0 and seen["quote_lost"] == 0, seen
    # a sub-range is the same rows; the folds stay on the device
    whole = env.tape_pnl(7, "previous", series=True)
    part = env.tape_pnl(7, "previous", series=True, first_market=5, n_markets=6)
    assert all(torch.equal(p, w[5:11]) for p, w in zip(part, whole))
    folded = PN.fold(whole[0])
    assert folded.is_cuda and np.array_equal(_np(folded), PN.fold(_np(whole[0])))
    slot = torch.arange(c["n"] * c["a"], device="cuda:0").reshape(c["n"], c["a"]) % 3
    by_mod = PN.pnl_by_module(whole[0], slot, 3)
    assert by_mod.is_cuda and all(np.array_equal(_np(by_mod[k]), PN.fold(_np(whole[0])[_np(slot) == k])) for k in range(3))
    _clean(env)
    env.close()


@pytest.mark.parametrize("name", ["agents2", "agents5", "agents16", "pass64", "pass65", "pass128"])
def test_agent_counts_and_scan_pass_borders(name):
    c = PC.case(name)
    env = _env(c["n"], c["a"], c["max_step"], c["tape_cap"], c["quote_cap"])
    seen = _play(env, c)
    assert seen["bars"] > 0 and seen["fills"] > 0 and seen["unmarked"] > 0 and seen["open_fills"] > 0 and seen["tape_lost"] == 0 and seen["quote_lost"] == 0, seen
    if name.startswith("pass"):                                      # the previous episode is whole: exactly max_step points at one-step bars
        stats = _np(env.tape_pnl(1, "previous")[0])
        assert (stats[..., 0] + stats[..., 2] == c["max_step"]).all()
    _clean(env)
    env.close()


# ---- 2. rings smaller than the episode ------------------------------------------------------------------------------------------------------------
def test_rings_smaller_than_the_episode_report_what_they_lost():
    c = PC.case("small_rings")
    assert c["tape_cap"] == 64 and c["quote_cap"] == 64
    env = _env(c["n"], c["a"], c["max_step"], c["tape_cap"], c["quote_cap"])
    seen = _play(env, c)
    assert seen["tape_lost"] > 0 and seen["quote_lost"] > 0 and seen["bars"] > 0 and seen["open_fills"] > 0, seen
    _clean(env)
    env.close()


# ---- 3. every word is written; refusals write none -------------------------------------------------------------------------------------------------
def _raw(env, first, n, which, bar, stats, equity, position, marks, n_points, info):
    from gym_continuousdoubleauction_amd._lib import lib
    ptr = [None if x is None else x if isinstance(x, int) else x.data_ptr() for x in (stats, equity, position, marks, info)]
    return lib().cda_tape_pnl(env._h, first, n, which, bar, ptr[0], ptr[1], ptr[2], ptr[3], n_points, ptr[4], env._stream())


def _poisoned(n, a, P):
    dev = "cuda:0"
    return [torch.full((n, a, 16), POISON64, dtype=torch.int64, device=dev), torch.full((n, a, P), POISON64, dtype=torch.int64, device=dev),
            torch.full((n, a, P), POISON32, dtype=torch.int32, device=dev), torch.full((n, P), POISON32, dtype=torch.int32, device=dev),
            torch.full((n, 4), POISON32, dtype=torch.int32, device=dev)]


def _untouched(bufs):
    torch.cuda.synchronize()
    return all(bool((b == (POISON64 if b.dtype == torch.int64 else POISON32)).all()) for b in bufs)


def test_every_output_word_is_written_without_a_memset():
    n, a, max_step = 10, 4, 90                                       # (10 markets: the last workgroup has waves without a market)
    env = _env(n, a, max_step, 1024, 256)
    env.reset(seed=np.arange(40, 40 + n, dtype=np.uint64))
    rng = np.random.default_rng(9)
    for _ in range(max_step + 20):                                   # a whole previous episode, a current one of 20 steps: most of its grid is not held
        env.step(*PC.actions(rng, n, a))
    for which in (0, 1):
        for bar, P in ((1, 90), (1, 97), (7, 13), (7, 40)):          # grids of exactly the episode's points, and wider ones
            bufs = _poisoned(n, a, P)
            assert _raw(env, 0, n, which, bar, *bufs[:4], P, bufs[4]) == 0
            torch.cuda.synchronize()
            for b in bufs:
                assert not bool((b == (POISON64 if b.dtype == torch.int64 else POISON32)).any()), (which, bar, P, b.shape)
            if P in (90, 13):
                want = env.tape_pnl(bar, "current" if which == 0 else "previous", series=True)
                assert all(torch.equal(g, w) for g, w in zip(bufs, want)), (which, bar)
            some = _poisoned(n, a, P)                                # one series alone, no info: the others are not touched
            assert _raw(env, 0, n, which, bar, some[0], None, None, some[3], P, None) == 0
            assert _untouched([some[1], some[2], some[4]]) and torch.equal(some[0], bufs[0]) and torch.equal(some[3], bufs[3])
    # a range that leaves markets out writes their rows neither
    bufs = _poisoned(n, a, 90)
    assert _raw(env, 3, 5, 1, 1, bufs[0][3:8], bufs[1][3:8], bufs[2][3:8], bufs[3][3:8], 90, bufs[4][3:8]) == 0
    torch.cuda.synchronize()
    want = env.tape_pnl(1, "previous", series=True, first_market=3, n_markets=5)
    assert all(torch.equal(b[3:8], w) for b, w in zip(bufs, want)) and _untouched([b[:3] for b in bufs] + [b[8:] for b in bufs])
    _clean(env)
    env.close()


def test_the_entry_point_refuses_bad_arguments_on_a_live_env_and_writes_nothing():
    n, a, max_step = 4, 4, 32
    env = _env(n, a, max_step, 64, 64)
    env.reset(seed=np.arange(7, 7 + n, dtype=np.uint64))
    rng = np.random.default_rng(3)
    for _ in range(12):
        env.step(*PC.actions(rng, n, a))
    P = 32
    bufs = _poisoned(n, a, P + 1)                                    # (one word more: room for a misaligned pointer)
    s, e, p, k, info = bufs
    assert _raw(env, 0, n, 0, 1, *_poisoned(n, a, P)[:4], P, None) == 0 and _raw(env, 1, 3, 1, 7, *_poisoned(n, a, P)[:4], 5, None) == 0
    for first, cnt, which, bar in ((0, 5, 0, 1), (-1, 2, 0, 1), (0, 0, 0, 1), (4, 1, 0, 1), (0, 4, 2, 1), (0, 4, -1, 1), (0, 4, 0, 0), (0, 4, 0, -2)):
        assert _raw(env, first, cnt, which, bar, s, e, p, k, P, info) == INVALID, (first, cnt, which, bar)
    assert _raw(env, 0, n, 0, 1, None, e, p, k, P, info) == INVALID                                     # stats may not be NULL
    assert _raw(env, 0, n, 0, 1, s.data_ptr() + 4, e, p, k, P, info) == INVALID and _raw(env, 0, n, 0, 1, s, e.data_ptr() + 4, p, k, P, info) == INVALID
    for at in range(3):                                              # the int32 outputs: 4-byte aligned
        ptrs = [p.data_ptr(), k.data_ptr(), info.data_ptr()]
        ptrs[at] += 2
        assert _raw(env, 0, n, 0, 1, s, e, ptrs[0], ptrs[1], P, ptrs[2]) == INVALID, at
    # too few points for a series - any one of them - and fine without one
    for series in ((e, None, None), (None, p, None), (None, None, k), (e, p, k)):
        assert _raw(env, 0, n, 0, 1, s, *series, P - 1, info) == INVALID and _raw(env, 0, n, 0, 7, s, *series, 4, info) == INVALID, series
    assert _untouched(bufs)
    assert _raw(env, 0, n, 0, 1, s, None, None, None, 0, None) == 0 and _raw(env, 0, n, 0, 7, s, None, None, None, -5, None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        env.tape_pnl(bar_steps=0)
    with pytest.raises(ValueError):
        env.tape_pnl(episode="next")
    # either tape off: unsupported
    bufs = _poisoned(n, a, P)
    env.disable_quotes()
    assert _raw(env, 0, n, 0, 1, *bufs[:4], P, bufs[4]) == UNSUPPORTED
    with pytest.raises(RuntimeError, match="enable_quotes"):
        env.tape_pnl()
    env.enable_quotes(64)
    assert _raw(env, 0, n, 0, 1, *_poisoned(n, a, P)[:4], P, None) == 0
    torch.cuda.synchronize()
    env.disable_tape()
    assert _raw(env, 0, n, 0, 1, *bufs[:4], P, bufs[4]) == UNSUPPORTED
    with pytest.raises(RuntimeError, match="enable_tape"):
        env.tape_pnl()
    assert _raw(env, 0, 5, 0, 1, *bufs[:4], P, bufs[4]) == INVALID                                      # (an invalid argument is still that)
    assert _untouched(bufs)
    _clean(env)
    env.close()


# ---- 4. the border: 4096 points -----------------------------------------------------------------------------------------------------------------
def test_an_episode_of_8192_steps_needs_two_step_bars():
    n, a = 1, 4
    env = _env(n, a, 8192, 256, 64)
    env.reset(seed=np.array([77], np.uint64))
    rng = np.random.default_rng(8)
    for _ in range(40):
        env.step(*PC.actions(rng, n, a))
    with pytest.raises(ValueError, match="bar points"):
        env.tape_pnl(bar_steps=1)
    bufs = _poisoned(n, a, 8192)
    assert _raw(env, 0, n, 0, 1, *bufs[:4], 8192, bufs[4]) == INVALID and _raw(env, 0, n, 0, 1, bufs[0], None, None, None, 0, None) == INVALID
    assert _untouched(bufs)
    seen = _check(env, "border", (2, 5))                             # 4096 points: one market-wave per workgroup, the whole LDS budget
    assert seen["bars"] > 0 and seen["quote_lost"] == 0, seen
    _clean(env)
    env.close()


# ---- 5. random configurations --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(6))
def test_the_report_on_a_random_service_configuration(index):
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
    top = int(env.market_rows()["max_step"].max()) if env.per_market else int(env.max_step)
    bars = sorted({b for b in (1, case["bar_steps"]) if -(-top // b) <= 4096} or {-(-top // 4096)})
    seen = _check(env, f"case {index} {cfg} rows={rows}", bars)
    assert seen["bars"] > 0 or seen["fills"] < 2, seen
    _clean(env, flags)
    env.close()


# ---- 6. evaluate -----------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_reports_every_module_s_pnl(tmp_path):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd import pnl as PN
    from gym_continuousdoubleauction_amd import quotes as Q
    from gym_continuousdoubleauction_amd import tape as T
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    n, a, episodes, max_step, bar = 32, 4, 2, 48, 3
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}, n_markets=n, with_info=False)
    pol = mlp.FusedPolicy("cuda:0", seed=5)
    with pytest.raises(ValueError, match="tape"):
        evaluate(env, pol, opponents=["random"], episodes=episodes, seed=3, pnl_report=True)
    with pytest.raises(ValueError, match="bar_steps"):
        evaluate(env, pol, opponents=["random"], episodes=episodes, seed=3, pnl_report=True, tape=str(tmp_path / "x.npz"), bar_steps=0)
    qpath, tpath, keep = str(tmp_path / "quotes.npz"), str(tmp_path / "tape.npz"), {}
    res = evaluate(env, pol, opponents=["random", "maker"], trained_slots=1, episodes=episodes, seed=3, tape=tpath, quotes=qpath, pnl_report=True, bar_steps=bar, keep=keep)
    assert not env.quotes_enabled and not env.tape_enabled
    z, tp = Q.load(qpath), T.load_tape(tpath)
    assert z["counts"].tolist() == [max_step] * n and not tp["dropped"].any()
    tables = keep["pnl_tables"]
    assert tables["counted"].all() and tables["stats"].shape == (n, a, 16)
    # The kept tables are the specification's, from the saved tape and quotes.  Both episodes ran in one rollout, so the file's episode ids are exact only where
    # the step index drops between them; the device's own record count says which of a market's rows are the last finished episode's: the current one is empty.
    for m in range(n):
        mine = tp["records"][tp["market"] == m]
        t = mine[len(mine) - int(tables["info"][m, 0]):]
        assert len(t) <= len(mine) and (np.diff(t[:, 7] >> 2) >= 0).all(), m
        want = PN.pnl_from_records(t, z["records"][m, :z["counts"][m]], a, bar)[0]
        assert np.array_equal(tables["stats"][m], want), (m, tables["stats"][m], want)
    names = ["policy", "opponent_0", "opponent_1"]
    modules = keep["modules"]
    by_mod = PN.pnl_by_module(torch.from_numpy(tables["stats"]), torch.from_numpy(modules.astype(np.int64)), len(names)).numpy()
    traded = 0
    for i, name in enumerate(names):
        block = res["modules"][name]["pnl"]
        row = np.array(block["row"], np.int64)
        assert np.array_equal(row, by_mod[i]) and np.array_equal(row, PN.fold(tables["stats"][modules == i])), (name, row, by_mod[i])
        assert {k: v for k, v in block.items() if k != "row"} == PN.pnl_summary(row, bar_steps=bar), name
        assert row[PN.PNL["points"]] > 0 and row[PN.PNL["bars"]] > 0
        traded += int(row[PN.PNL["sum_d2"]] > 0)
    assert traded >= 2 and by_mod[:, PN.PNL["inventory"]].sum() == 0 and by_mod[:, PN.PNL["trading"]].sum() == 0      # the modules' P&L parts cancel: nothing lost
    about = res["pnl"]
    assert about["bar_steps"] == bar and about["markets"] == n and about["episode"] == "previous" and about["pnl_words"] == list(PN.PNL_FIELDS)
    assert about["tape_records_lost"] == 0 and about["quotes_lost"] == 0 and about["partial_markets"] == 0
    assert about["tape_records"] == int(tables["info"][:, 0].sum()) > 0
    _clean(env)
    env.close()
