"""CPU: the P&L report's host side (gym_continuousdoubleauction_amd/pnl.py).  The worked example of the report's definition, word by word; the specification -
vectorised numpy - against a scalar restatement written here from the definitions (a loop per fill and per point, sharing no code with pnl.py) over a few hundred
random small episodes (tests/pnl_cases.py); the identities the words obey; the fold rule, pnl_by_module on CPU tensors, pnl_summary; cda_tape_pnl_check_host at
each bound and one beyond it through the product library (no env, no device); and the cases the GPU test plays, replayed on the CPU oracle: they must hold what
that comparison is about.  Integers only."""
import os
import re

import numpy as np
import pytest

import pnl_cases as PC
from gym_continuousdoubleauction_amd import pnl as PN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
F = PN.PNL


# ---- the worked example ------------------------------------------------------------------------------------------------------------------------
def _example():
    quotes = np.array([(0, 0, 0, 0, 0, 0, 0, 0), (1, 3, 98, 102, 1, 1, 1, 1), (2, 1, 98, 0, 1, 0, 1, 0), (3, 3, 100, 104, 1, 1, 1, 1), (4, 3, 99, 101, 1, 1, 1, 1)], np.int32)
    # (time, price, quantity, counter_id, counter_order_id, counter_left, init_id, step << 2 | init side << 1 | counter side)
    tape = np.array([(0, 102, 3, 1, 0, 0, 0, (1 << 2) | (0 << 1) | 1),      # step 1: agent 0 initiates, buys 3 @ 102 from agent 1
                     (1, 104, 1, 0, 1, 0, 1, (3 << 2) | (0 << 1) | 1),      # step 3: agent 1 initiates, buys 1 @ 104 from agent 0
                     (2, 99, 2, 1, 2, 0, 0, (4 << 2) | (1 << 1) | 0)], np.int32)      # step 4: agent 0 initiates, sells 2 @ 99 to agent 1
    return tape, quotes


def test_the_worked_example_word_by_word():
    tape, quotes = _example()
    stats, equity, position, marks = PN.pnl_from_records(tape, quotes, 2, 1)
    assert PN.PNL_FIELDS == ("points", "stale", "unmarked", "bars", "equity_first", "equity_last", "inventory", "trading", "sum_d2", "up", "down", "under_water",
                             "max_drawdown", "equity_max", "equity_min", "open_fills")
    assert stats.dtype == np.int64 and stats.tolist() == [[4, 1, 1, 3, 0, -4, 0, -4, 304, 1, 2, 2, 12, 0, -12, 1],
                                                          [4, 1, 1, 3, 0, 4, 0, 4, 304, 2, 1, 2, 12, 12, 0, 1]]
    assert marks.dtype == np.int32 and marks.tolist() == [0, 200, 200, 204, 200]
    assert position.dtype == np.int32 and position.tolist() == [[0, 0, 3, 3, 2], [0, 0, -3, -3, -2]]
    assert equity.dtype == np.int64 and equity.tolist() == [[0, 0, -12, 0, -4], [0, 0, 12, 0, 4]]
    # on a longer grid the tail is zeros; a shorter one is refused
    wide = PN.pnl_from_records(tape, quotes, 2, 1, n_points=8)
    assert np.array_equal(wide[0], stats) and wide[1].shape == (2, 8) and wide[3].tolist() == [0, 200, 200, 204, 200, 0, 0, 0] and not wide[1][:, 5:].any()
    with pytest.raises(ValueError, match="n_points"):
        PN.pnl_from_records(tape, quotes, 2, 1, n_points=4)
    with pytest.raises(ValueError, match="agent id"):
        PN.pnl_from_records(tape, quotes, 1, 1)
    with pytest.raises(ValueError, match="consecutive"):
        PN.pnl_from_records(tape, quotes[[0, 2, 3]], 2, 1)
    with pytest.raises(ValueError, match="bar_steps"):
        PN.pnl_from_records(tape, quotes, 2, 0)


def test_summary_of_the_example():
    tape, quotes = _example()
    stats = PN.pnl_from_records(tape, quotes, 2, 1)[0]
    s = PN.pnl_summary(stats[0])
    assert s["pnl"] == -2.0 and s["inventory_pnl"] == 0.0 and s["trading_pnl"] == -2.0 and s["max_drawdown"] == 6.0 and s["equity_max"] == 0.0 and s["equity_min"] == -6.0
    assert s["bars"] == 3 and s["points"] == 4 and s["open_fills"] == 1 and s["stale_points"] == 1 and s["unmarked_points"] == 1 and s["bar_steps"] == 1
    d = np.array([-6.0, 6.0, -2.0])                                  # the bar P&L in price units
    assert s["bar_pnl_mean"] == pytest.approx(d.mean()) and s["bar_pnl_std"] == pytest.approx(d.std())
    assert s["sharpe_per_bar"] == pytest.approx(d.mean() / d.std()) and s["sharpe_episode"] == pytest.approx(d.mean() / d.std() * 3 ** 0.5)
    assert s["hit_ratio"] == pytest.approx(1 / 3) and s["under_water_share"] == 0.5 and s["calmar"] == pytest.approx(-4 / 12)
    t = PN.pnl_summary(stats[1], bar_steps=7)
    assert t["pnl"] == 2.0 and t["hit_ratio"] == pytest.approx(2 / 3) and t["calmar"] == pytest.approx(4 / 12) and t["bar_steps"] == 7
    empty = PN.pnl_summary(np.zeros(16, np.int64))
    for key in ("bar_pnl_mean", "bar_pnl_std", "sharpe_per_bar", "sharpe_episode", "hit_ratio", "under_water_share", "calmar"):
        assert empty[key] is None, key
    assert empty["pnl"] == 0.0
    flat = PN.pnl_summary(np.array([3, 0, 0, 2, 5, 5, 0, 0, 0, 0, 0, 0, 0, 5, 5, 0], np.int64))      # no variance: no Sharpe ratio
    assert flat["bar_pnl_std"] == 0.0 and flat["sharpe_per_bar"] is None and flat["hit_ratio"] is None and flat["calmar"] is None
    with pytest.raises(ValueError):
        PN.pnl_summary(stats)


# ---- the scalar restatement --------------------------------------------------------------------------------------------------------------------
def loop_pnl(tape, quotes, agents, bar):
    """from the definitions, one fill and one point at a time -> (stats rows, {agent: {point: E}}, {agent: {point: pos}}, {point: mark})"""
    held = {int(r[0]): (int(r[2]) + int(r[3]) if (int(r[1]) & 3) == 3 else None) for r in quotes}      # step -> m2, None where not two-sided
    points = sorted(s // bar for s in held if s % bar == 0)
    mark, m = {}, None
    for p in points:
        if held[p * bar] is not None:
            m = held[p * bar]
        if m is not None:
            mark[p] = m
    marked = [p for p in points if p in mark]
    rows, eq_of, pos_of = [], {}, {}
    for who in range(agents):
        mine = []                                                    # (step, signed quantity, price)
        for r in tape:
            price, qty, cid, iid, word = int(r[1]), int(r[2]), int(r[3]), int(r[6]), int(r[7])
            if cid == iid or who not in (cid, iid):
                continue
            side = (word >> 1) & 1 if iid == who else word & 1
            mine.append((word >> 2, qty if side == 0 else -qty, price))
        pos_of[who] = {p: sum(sq for s, sq, _ in mine if s < p * bar) for p in points}
        E = {}
        for p in marked:
            cash = sum(-sq * price for s, sq, price in mine if s < p * bar)
            E[p] = 2 * cash + pos_of[who][p] * mark[p]
        eq_of[who] = E
        row = dict.fromkeys(PN.PNL_FIELDS, 0)
        row["points"], row["unmarked"] = len(marked), len(points) - len(marked)
        row["stale"] = sum(1 for p in marked if held[p * bar] is None)
        row["open_fills"] = sum(1 for s, _, _ in mine if s >= marked[-1] * bar) if marked else len(mine)
        if marked:
            row["equity_first"], row["equity_last"] = E[marked[0]], E[marked[-1]]
            row["equity_max"], row["equity_min"] = max(E.values()), min(E.values())
            top = E[marked[0]]
            for p in marked:
                top = max(top, E[p])
                row["under_water"] += E[p] < top
                row["max_drawdown"] = max(row["max_drawdown"], top - E[p])
            for p, nxt in zip(marked[:-1], marked[1:]):
                assert nxt == p + 1                                  # held points are consecutive
                d = E[nxt] - E[p]
                row["bars"] += 1; row["sum_d2"] += d * d; row["up"] += d > 0; row["down"] += d < 0
                row["inventory"] += pos_of[who][p] * (mark[nxt] - mark[p])
                row["trading"] += sum(sq * (mark[nxt] - 2 * price) for s, sq, price in mine if p * bar <= s < nxt * bar)
        rows.append([row[f] for f in PN.PNL_FIELDS])
    return np.array(rows, np.int64).reshape(agents, 16), eq_of, pos_of, mark


CASES = PC.episodes(20261, 300)


def test_the_generator_covers_the_ground():
    assert {c["agents"] for c in CASES} == set(range(1, 17)) and {c["bar"] for c in CASES} == set(PC.BARS)
    assert min(len(c["quotes"]) for c in CASES) == 0 and max(len(c["quotes"]) for c in CASES) > 128 and min(len(c["tape"]) for c in CASES) == 0
    assert max(len(c["tape"]) for c in CASES) > 128 and any(c["tape_lost"] for c in CASES) and any(c["quote_lost"] for c in CASES)
    assert any(len(c["tape"]) and (c["tape"][:, 3] == c["tape"][:, 6]).any() for c in CASES)
    flags = [c["quotes"][:, 1] & 3 for c in CASES if len(c["quotes"]) > 10]
    assert any((f[:3] != 3).all() for f in flags) and any((f[-3:] != 3).all() for f in flags) and any((f[0] == 3) and (f[-1] == 3) and (f != 3).any() for f in flags)


@pytest.mark.parametrize("chunk", range(6))
def test_the_specification_equals_the_scalar_restatement(chunk):
    seen = dict.fromkeys(("stale", "unmarked", "open_fills", "bars", "under_water", "no_points"), 0)
    for i, c in enumerate(CASES[chunk * 50:(chunk + 1) * 50]):
        tape, quotes, a, bar = c["tape"], c["quotes"], c["agents"], c["bar"]
        stats, equity, position, marks = PN.pnl_from_records(tape, quotes, a, bar)
        want, eq_of, pos_of, mark = loop_pnl(tape, quotes, a, bar)
        ctx = (chunk, i, a, bar)
        assert stats.dtype == np.int64 and stats.shape == (a, 16) and np.array_equal(stats, want), (ctx, stats, want)
        n_pts = (int(quotes[-1, 0]) // bar + 1) if len(quotes) else 0
        assert equity.shape == position.shape == (a, n_pts) and marks.shape == (n_pts,)
        assert marks.tolist() == [mark.get(p, 0) for p in range(n_pts)], ctx
        for who in range(a):
            assert equity[who].tolist() == [eq_of[who].get(p, 0) for p in range(n_pts)], (ctx, who)
            assert position[who].tolist() == [pos_of[who].get(p, 0) for p in range(n_pts)], (ctx, who)
        # the identities
        assert np.array_equal(stats[:, F["inventory"]] + stats[:, F["trading"]], stats[:, F["equity_last"]] - stats[:, F["equity_first"]]), ctx
        assert np.array_equal(stats[:, F["bars"]], np.maximum(stats[:, F["points"]] - 1, 0)), ctx
        assert (stats[:, F["max_drawdown"]] >= 0).all() and (stats[:, F["equity_max"]] >= stats[:, F["equity_min"]]).all(), ctx
        if not c["tape_lost"]:
            assert not equity.sum(axis=0).any() and stats[:, F["inventory"]].sum() == 0 and stats[:, F["trading"]].sum() == 0, ctx
        for key in ("stale", "unmarked", "open_fills", "bars", "under_water"):
            seen[key] += int(stats[:, F[key]].sum() > 0)
        seen["no_points"] += int(stats[0, F["points"]] == 0)
    assert all(v > 0 for v in seen.values()), seen


def test_a_bar_s_signed_quantity_is_an_int32_word_and_products_wrap():
    big = 2 ** 31 - 1
    quotes = np.array([(s, 3, 10, 12 + 2 * s, 1, 1, 1, 1) for s in range(4)], np.int32)
    tape = np.zeros((2, 8), np.int32)
    tape[:, 1], tape[:, 2], tape[:, 3], tape[:, 6], tape[:, 7] = 11, big, 1, 0, (1 << 2) | 1      # agent 0 buys INT32_MAX twice in step 1, from agent 1
    stats, equity, position, marks = PN.pnl_from_records(tape, quotes, 2, 1)
    assert position[0].tolist() == [0, 0, -2, -2] and marks.tolist() == [22, 24, 26, 28]          # Q_1 = 2^32 - 2 wraps to -2
    assert equity[0].tolist() == [0, 0, -4 * big * 11 - 2 * 26, -4 * big * 11 - 2 * 28]
    assert stats[0, F["inventory"]] + stats[0, F["trading"]] == stats[0, F["equity_last"]] - stats[0, F["equity_first"]]


# ---- the fold ---------------------------------------------------------------------------------------------------------------------------------
def test_the_fold_rule():
    import torch
    assert set(PN.PNL_ADDITIVE) | {"max_drawdown", "equity_max", "equity_min"} == set(PN.PNL_FIELDS) and len(PN.PNL_ADDITIVE) == 13 and PN.pool is PN.fold
    rows = np.concatenate([PN.pnl_from_records(c["tape"], c["quotes"], c["agents"], c["bar"])[0] for c in CASES[:40]])
    none = rows[:, F["points"]] == 0
    assert none.any() and (~none).any()
    rows[none, F["equity_min"]] = 0                                  # (as the device leaves them) - and they must not enter the min / max
    got = PN.fold(rows)
    some = rows[~none]
    for f in PN.PNL_ADDITIVE:
        assert got[F[f]] == rows[:, F[f]].sum(), f
    assert got[F["max_drawdown"]] == some[:, F["max_drawdown"]].max() and got[F["equity_max"]] == some[:, F["equity_max"]].max()
    assert got[F["equity_min"]] == some[:, F["equity_min"]].min()
    all_above = some[some[:, F["equity_min"]] > 0][:3]               # rows without points hold zeros: they must not pull a positive minimum down
    if len(all_above):
        assert PN.fold(np.concatenate([all_above, rows[none][:2]]))[F["equity_min"]] == all_above[:, F["equity_min"]].min() > 0
    lifted = np.array([[2, 0, 0, 1, 5, 9, 0, 4, 16, 1, 0, 0, 0, 9, 5, 0], [0] * 16, [2, 0, 0, 1, -7, -3, 0, 4, 16, 1, 0, 0, 0, -3, -7, 0]], np.int64)
    assert PN.fold(lifted[:2])[F["equity_min"]] == 5 and PN.fold(lifted[1:])[F["equity_max"]] == -3 and PN.fold(lifted[1:2]).tolist() == [0] * 16
    # a fold of folds is the fold; lists of tables and tensors alike
    assert np.array_equal(PN.fold([PN.fold(rows[:17]), PN.fold(rows[17:])]), got) and np.array_equal(PN.fold([rows[:5], rows[5:]]), got)
    assert np.array_equal(PN.fold(rows.reshape(-1, 1, 16)), got) and np.array_equal(PN.fold(torch.from_numpy(rows)).numpy(), got)
    assert np.array_equal(PN.fold([torch.from_numpy(rows[:9]), torch.from_numpy(rows[9:])]).numpy(), got)
    assert PN.fold(np.zeros((0, 16), np.int64)).tolist() == [0] * 16


def test_pnl_by_module_folds_through_the_slot_map():
    import torch
    rng = np.random.default_rng(5)
    n, a, m = 9, 4, 3
    cases = [c for c in CASES if c["agents"] == a][:n]
    stats = np.stack([PN.pnl_from_records(c["tape"], c["quotes"], a, c["bar"])[0] for c in cases])
    slot = rng.integers(0, m, (n, a))
    slot[0] = 3                                                      # a module of one market's slots only
    got = PN.pnl_by_module(torch.from_numpy(stats), torch.from_numpy(slot), m + 2).numpy()
    for k in range(m + 1):
        assert np.array_equal(got[k], PN.fold(stats[slot == k])), k
    assert got[m + 1].tolist() == [0] * 16                           # a module without slots
    with pytest.raises(ValueError, match="module id"):
        PN.pnl_by_module(torch.from_numpy(stats), torch.from_numpy(slot), 3)
    with pytest.raises(ValueError):
        PN.pnl_by_module(torch.from_numpy(stats[:, :, :8]), torch.from_numpy(slot), 4)


# ---- the library's host check ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip_lib():
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib()


def test_the_host_check_at_each_bound_and_one_beyond(hip_lib):
    check = hip_lib.cda_tape_pnl_check_host                          # (bar_steps, n_points, want_series, max_step)
    assert check(1, 0, 0, 64) == OK and check(1, 64, 1, 64) == OK and check(1, 63, 1, 64) == INVALID and check(1, 65, 1, 64) == OK
    assert check(0, 64, 0, 64) == INVALID and check(-3, 64, 0, 64) == INVALID and check(1, 0, 0, 0) == INVALID
    assert check(1, 0, 0, 4096) == OK and check(1, 0, 0, 4097) == INVALID                          # the border: 4096 / 4097 points
    assert check(2, 0, 0, 8192) == OK and check(2, 0, 0, 8193) == INVALID and check(3, 0, 0, 4096 * 3) == OK and check(3, 0, 0, 4096 * 3 + 1) == INVALID
    assert check(1, 4096, 1, 4096) == OK and check(1, 4095, 1, 4096) == INVALID and check(2, 4096, 1, 8191) == OK and check(2, 4095, 1, 8191) == INVALID
    assert check(7, 10, 1, 64) == OK and check(7, 9, 1, 64) == INVALID and check(7, -1, 0, 64) == OK and check(7, -1, 1, 64) == INVALID
    assert check(2 ** 31 - 1, 1, 1, 2 ** 31 - 1) == OK and check(2 ** 31 - 1, 0, 1, 2 ** 31 - 1) == INVALID
    assert hip_lib.cda_tape_pnl(None, 0, 1, 0, 1, None, None, None, None, 0, None, None) == INVALID      # without an env nothing is launched


class _StubLib:
    def __init__(self):
        self.tape, self.quotes, self.calls = 64, 64, []

    def cda_tape_capacity(self, h):
        return self.tape

    def cda_quotes_capacity(self, h):
        return self.quotes

    def __getattr__(self, name):
        def call(*a):
            self.calls.append(name)
            return 0
        return call


def test_the_wrapper_checks_its_arguments_before_any_launch(monkeypatch):
    from gym_continuousdoubleauction_amd import vec_env as V
    stub = _StubLib()
    monkeypatch.setattr(V, "lib", lambda: stub)
    env = V.CDAVecEnv.__new__(V.CDAVecEnv)
    env._h, env.n_markets, env.num_agents, env.per_market, env.max_step = None, 8, 4, False, 8192
    env.sync = env.join = lambda: None
    for kw in ({"episode": "next"}, {"first_market": 8}, {"n_markets": 0}, {"first_market": 5, "n_markets": 4}, {"bar_steps": 0}, {"bar_steps": 1}):
        with pytest.raises(ValueError):
            env.tape_pnl(**kw)
    with pytest.raises(ValueError, match="bar points"):
        env.tape_pnl(bar_steps=1, series=True)                       # 8192 points
    stub.quotes = 0
    with pytest.raises(RuntimeError, match="enable_quotes"):
        env.tape_pnl(bar_steps=2)
    stub.quotes, stub.tape = 64, 0
    with pytest.raises(RuntimeError, match="enable_tape"):
        env.tape_pnl(bar_steps=2)
    assert stub.calls == []


def test_field_tuple_words_and_entry_points_are_the_header_s():
    from gym_continuousdoubleauction_amd import _capi, _lib
    hdr = open(os.path.join(ROOT, "include", "cda.h")).read()
    assert re.search(r"#define CDA_PNL_WORDS\s+16\b", hdr) and PN.PNL_WORDS == len(PN.PNL_FIELDS) == _capi.PNL_WORDS == 16 and PN.MAX_BARS == 4096
    for name in ("cda_tape_pnl", "cda_tape_pnl_check_host"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SYMBOLS, name
    inc =open(os.path.join(ROOT, "gym_continuousdoubleauction_amd", "csrc", "cda_hip.hip")).read()
    assert inc.index('#include "cda_stylised.inc"') < inc.index('#include "cda_tape_pnl.inc"')
    enum = re.search(r"enum \{ (PN_POINTS.*?) \};", open(os.path.join(ROOT, "gym_continuousdoubleauction_amd", "csrc", "cda_tape_pnl.inc")).read(), re.S).group(1)
    assert [w.split("=")[0].strip().lower()[3:] for w in enum.replace("\n", " ").split(",")] == list(PN.PNL_FIELDS)


# ---- the cases the GPU test plays hold what it is about -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replays():
    import __graft_entry__ as g
    g.build_oracle()
    return [(c, PC.replay(c)) for c in PC.DEVICE_CASES]


def test_the_device_cases_cover_what_the_comparison_is_about(replays):
    """From the CPU oracle and the quote recorder's host replay alone.  The oracle keeps no tape: a step's non-self fills are half its trade counters' sum, which a
    self-trade does not move; those are counted by a shadow oracle that replays the base case's steps order by order (pnl_cases.self_trades)."""
    seen = dict.fromkeys(("stale", "unmarked", "open_fills", "tape_lost", "quote_lost", "long", "fills", "markets"), 0)
    by_case = {}
    for c, stops in replays:
        mine = dict.fromkeys(seen, 0)
        assert len(stops) == len(c["stops"])
        for stop in stops:
            for which in ("current", "previous"):
                for row in stop[which]:
                    q, per_step = row["quotes"], row["fills"]
                    for bar in c["bars"]:
                        st = PN.pnl_from_records(np.zeros((0, 8), np.int32), q, c["a"], bar)[0][0]
                        mine["stale"] += int(st[F["stale"]] > 0); mine["unmarked"] += int(st[F["unmarked"]] > 0); mine["long"] += int(st[F["points"]] > 128)
                        if st[F["points"]] and len(q):
                            last = (int(q[-1, 0]) // bar) * bar      # the step of the last marked point
                            mine["open_fills"] += int(sum(per_step[last:]) > 0)
                    mine["tape_lost"] += int(row["tape_lost"] > 0); mine["quote_lost"] += int(row["quote_lost"] > 0); mine["fills"] += sum(per_step); mine["markets"] += 1
        by_case[c["name"]] = mine
        for k, v in mine.items():
            seen[k] += v
    assert all(v > 0 for v in seen.values()), seen
    assert by_case["small_rings"]["tape_lost"] > 0 and by_case["small_rings"]["quote_lost"] > 0 and by_case["base"]["long"] > 0
    assert by_case["base"]["tape_lost"] == 0 and by_case["base"]["quote_lost"] == 0                # the base case's rings hold both episodes whole
    assert all(m["fills"] > 64 and m["unmarked"] > 0 and m["open_fills"] > 0 for m in by_case.values()), by_case
    assert PC.self_trades(PC.case("base")) > 0
    assert {c["a"] for c, _ in replays} >= {2, 4, 5, 16} and {c["max_step"] for c, _ in replays} >= {64, 65, 128, 150}
