"""CPU: the stylised-facts report's host side (gym_continuousdoubleauction_amd/stylised.py).  Each of the three specifications - vectorised numpy - against a
plain-loop restatement written from the definitions, over random series with one-sided and empty steps, a lost head, bar sizes 1, 3 and 7 and lags that run past
the end; the identities with quote_stats at bar_steps 1; pool's additivity; summary on constructed series; the refusals of the three entry points through the
product library (cda_stylised_check_host is the check they make: no env, no device) and of the CDAVecEnv wrappers with the library stubbed.  Integers only."""
import ctypes as C
import os
import re
from collections import defaultdict

import numpy as np
import pytest

from gym_continuousdoubleauction_amd import quotes as Q
from gym_continuousdoubleauction_amd import stylised as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["cda_quote_returns", "cda_tape_signs", "cda_tape_flow_returns", "cda_stylised_check_host"]
OK, INVALID = 0, -1
BARS = (1, 3, 7)
LAGS = (1, 2, 8, 70)                                             # 70 runs past the end of every series below at bar sizes 3 and 7
FLOW_LAGS = (0, 1, 5, 70)


# ---- random series ------------------------------------------------------------------------------------------------------------------------
def quote_series(rng, steps, step0=0, tick=1, p_two=0.8):
    """int32 [steps, 8] quote rows of the consecutive steps step0 ..: a random walk of the mid in ticks, some steps one-sided or empty"""
    rows = np.zeros((steps, 8), np.int32)
    mid = 50 + np.cumsum(rng.integers(-3, 4, steps))
    for i in range(steps):
        flags = 3 if rng.random() < p_two else int(rng.integers(0, 3))
        bid, ask = (int(mid[i]) - int(rng.integers(0, 3))) * tick, (int(mid[i]) + 1 + int(rng.integers(0, 3))) * tick
        rows[i] = (step0 + i, flags, bid if flags & 1 else 0, ask if flags & 2 else 0, 5, 6, 1, 1)
    return rows


def tape_series(rng, fills, last_step, agents=4, step0=0):
    """int32 [fills, 8] tape rows in step order: sweeps (several same-sign fills in one step), self-trades, both sides"""
    rows = np.zeros((fills, 8), np.int32)
    steps = np.sort(rng.integers(step0, last_step + 1, fills))
    side = 0
    for i in range(fills):
        if i == 0 or steps[i] != steps[i - 1] or rng.random() < 0.3:
            side = int(rng.integers(0, 2))
        cid, iid = int(rng.integers(0, agents)), int(rng.integers(0, agents))
        rows[i] = (i, 40 + int(rng.integers(0, 20)), 1 + int(rng.integers(0, 30)), cid, i, -1, iid, (int(steps[i]) << 2) | (side << 1) | (1 - side))
    return rows


# ---- the plain-loop restatements ------------------------------------------------------------------------------------------------------------
def _m2_by_step(quote_rows):
    """step -> m2 of every HELD step, None where the record is not two-sided"""
    return {int(r[0]): (int(r[2]) + int(r[3]) if (int(r[1]) & 3) == 3 else None) for r in quote_rows}


def _ret(m2, s, bar):
    """the return at point s, or None"""
    a, b = m2.get(s), m2.get(s + bar)
    return None if a is None or b is None else b - a


def loop_returns(quote_rows, lags, bar, hh, tick):
    m2 = _m2_by_step(quote_rows)
    points = [s for s in sorted(m2) if s % bar == 0]
    base, lagged, hist = [0] * 8, [[0] * 4 for _ in lags], [0] * (2 * hh + 1)
    base[0] = len(points)
    for s in points:
        r = _ret(m2, s, bar)
        if r is None:
            base[2] += 1 if s + bar in m2 else 0
            continue
        base[1] += 1; base[3] += r; base[4] += abs(r); base[5] += r * r; base[6] += r > 0; base[7] += r < 0
        ticks = abs(r) // tick * (1 if r > 0 else -1)
        hist[min(max(ticks, -hh), hh) + hh] += 1
        for h, l in enumerate(lags):
            r2 = _ret(m2, s + l * bar, bar)
            if r2 is not None:
                lagged[h][0] += 1; lagged[h][1] += r * r2; lagged[h][2] += abs(r) * abs(r2); lagged[h][3] += r * abs(r2)
    return np.array(base, np.int64), np.array(lagged, np.int64), np.array(hist, np.int64)


def _fill(row):
    """(sign, quantity, step, self) of a tape row"""
    return (1 if (int(row[7]) >> 1) & 1 == 0 else -1), int(row[2]), int(row[7]) >> 2, int(row[3]) == int(row[6])


def loop_signs(tape_rows, lags):
    f = [_fill(r) for r in tape_rows]
    base, lagged = [0] * 8, [[0] * 4 for _ in lags]
    for i, (s, q, t, own) in enumerate(f):
        base[0] += 1; base[1] += s > 0; base[2] += s < 0; base[3] += q if s > 0 else 0; base[4] += q if s < 0 else 0; base[5] += own
        base[6] += i == 0 or f[i - 1][0] != s
        base[7] += i == 0 or f[i - 1][2] != t
        for h, l in enumerate(lags):
            if i + l < len(f):
                s2, q2, t2, _ = f[i + l]
                lagged[h][0] += 1; lagged[h][1] += s * s2; lagged[h][2] += s * q * s2 * q2; lagged[h][3] += t == t2
    return np.array(base, np.int64), np.array(lagged, np.int64)


def loop_flows(tape_rows, quote_rows, lags, bar, lost):
    m2, f = _m2_by_step(quote_rows), [_fill(r) for r in tape_rows]
    last_bar = max(m2) // bar if m2 else -1                        # the last bar that begins at or before the last held quote step
    first = 0
    if lost > 0:
        first = f[0][2] // bar + 1 if f else last_bar + 1
    volume, base = defaultdict(int), [0, 0, first, 0]
    for s, q, t, _ in f:
        volume[t // bar] += s * q
        if t // bar >= first:
            base[0] += 1; base[3] += q
    base[1] = len({t // bar for _, _, t, _ in f if t // bar >= first})
    lagged = [[0] * 6 for _ in lags]
    for b in range(first, last_bar + 1):
        qb = volume[b]
        for h, l in enumerate(lags):
            r = _ret(m2, (b + l) * bar, bar)
            if r is not None:
                lagged[h][0] += 1; lagged[h][1] += qb; lagged[h][2] += r; lagged[h][3] += qb * r; lagged[h][4] += qb * qb; lagged[h][5] += r * r
    return np.array(lagged, np.int64), np.array(base, np.int64)


# ---- 1. the specifications against the restatements -----------------------------------------------------------------------------------------
CASES = [(0, 90, 0, 1), (1, 90, 0, 5), (2, 64, 13, 1), (3, 65, 21, 2), (4, 1, 0, 1), (5, 2, 6, 1), (6, 0, 0, 1), (7, 130, 0, 1)]      # seed, steps, lost head, tick


@pytest.mark.parametrize("bar", BARS)
@pytest.mark.parametrize("seed,steps,step0,tick", CASES)
def test_returns_from_quotes_equals_the_loop_restatement(seed, steps, step0, tick, bar):
    rng = np.random.default_rng(100 + seed)
    rows = quote_series(rng, steps, step0, tick, p_two=0.8 if seed != 3 else 0.4)
    for hh in (2, 16):
        got, want = SF.returns_from_quotes(rows, LAGS, bar, hh, tick), loop_returns(rows, LAGS, bar, hh, tick)
        for g, w, name in zip(got, want, ("base", "lagged", "hist")):
            assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (name, g, w)
        assert got[2].sum() == got[0][SF.RET["returns"]] and got[0][SF.RET["bars"]] == len([s for s in rows[:, 0] if s % bar == 0])
    if steps > 60 and bar > 1:
        assert not got[1][-1].any()                                # the lag of 70 bars runs past the end
    if steps >= 90 and bar == 1:
        ends = SF.returns_from_quotes(rows, LAGS, bar, 2, tick)[2]
        assert got[1][:, 0].min() > 0 and got[0][SF.RET["missing"]] > 0 and ends[0] > 0 and ends[-1] > 0 and got[2][0] + got[2][-1] == 0      # two bins clip, sixteen do not


@pytest.mark.parametrize("seed,fills,last_step", [(0, 0, 10), (1, 1, 10), (2, 64, 30), (3, 65, 12), (4, 200, 90), (5, 131, 3)])
def test_signs_from_records_equals_the_loop_restatement(seed, fills, last_step):
    rows = tape_series(np.random.default_rng(200 + seed), fills, last_step)
    got, want = SF.signs_from_records(rows, LAGS), loop_signs(rows, LAGS)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (g, w)
    b = dict(zip(SF.SIGN_FIELDS, got[0]))
    assert b["buys"] + b["sells"] == b["fills"] == fills and b["runs"] <= fills and b["steps_with_fills"] <= min(fills, last_step + 1)
    if fills > 100:
        assert b["self_fills"] > 0 and 1 < b["runs"] < fills and got[1][0, SF.SLAG["same_step"]] > 0 and got[1][-1, 0] == fills - 70


@pytest.mark.parametrize("bar", BARS)
@pytest.mark.parametrize("seed,steps,step0,fills,lost", [(0, 90, 0, 150, 0), (1, 90, 0, 150, 9), (2, 64, 13, 40, 0), (3, 64, 13, 40, 3), (4, 40, 0, 0, 0),
                                                        (5, 40, 5, 0, 7), (6, 0, 0, 12, 2), (7, 0, 0, 0, 4), (8, 3, 8, 0, 1)])
def test_flow_returns_from_records_equals_the_loop_restatement(seed, steps, step0, fills, lost, bar):
    rng = np.random.default_rng(300 + seed)
    quotes = quote_series(rng, steps, step0, 1)
    first_step = 30 if lost else 0                                 # a tape whose head is lost starts later
    tape = tape_series(rng, fills, max(first_step, step0 + steps - 1, 20), step0=first_step)
    got, want = SF.flow_returns_from_records(tape, quotes, FLOW_LAGS, bar, lost), loop_flows(tape, quotes, FLOW_LAGS, bar, lost)
    for g, w, name in zip(got, want, ("lagged", "base")):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (name, seed, bar, g, w)
    if seed == 0:
        assert got[0][0, 0] > 0 and got[0][0, SF.FLAG["qq"]] > 0 and got[1][SF.FLW["bars_excluded"]] == 0 and got[1][SF.FLW["fills"]] == fills
    if seed == 1:
        assert got[1][SF.FLW["bars_excluded"]] == 30 // bar + 1 and 0 < got[1][SF.FLW["fills"]] < fills


def test_a_bar_s_signed_volume_is_an_int32_word():
    big = 2 ** 31 - 1
    tape = np.zeros((2, 8), np.int32)
    tape[:, 2], tape[:, 7] = big, (1 << 2) | 1                      # two buys of INT32_MAX in step 1
    quotes = np.array([(s, 3, 10, 12 + 2 * s, 1, 1, 1, 1) for s in range(4)], np.int32)
    lagged, base = SF.flow_returns_from_records(tape, quotes, (0,), 1)
    assert base.tolist() == [2, 1, 0, 2 * big]
    assert lagged[0].tolist() == [3, -2, 6, -4, 4, 12]             # Q_1 = 2^32 - 2 wraps to -2; every r is 2


# ---- 2. the identities with quote_stats at bar_steps 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,steps,step0", [(0, 90, 0), (2, 64, 13), (5, 2, 6), (6, 0, 0)])
def test_at_one_step_bars_the_base_words_are_quote_stats_own(seed, steps, step0):
    rows = quote_series(np.random.default_rng(100 + seed), steps, step0)
    base, _, hist = SF.returns_from_quotes(rows, (1,), 1, 4)
    stats = dict(zip(Q.STAT_FIELDS, Q.stats_from_quotes(rows)))
    b = dict(zip(SF.RETURN_FIELDS, base))
    assert b["returns"] == stats["pairs"] and b["sum_r2"] == stats["dm2_sq"] and b["sum_abs"] == stats["abs_dm2"] and hist.sum() == b["returns"]
    assert b["bars"] == stats["steps"] and b["up"] + b["down"] == stats["m2_changes"]


# ---- 3. pool and summary ---------------------------------------------------------------------------------------------------------------------
def test_pool_is_additive_over_a_split_of_the_markets():
    import torch
    rng = np.random.default_rng(7)
    tables = [np.stack(x) for x in zip(*[SF.returns_from_quotes(quote_series(rng, 50), (1, 3), 1, 3) for _ in range(6)])]
    for t in tables:
        assert t.shape[0] == 6 and np.array_equal(SF.pool(t), SF.pool(t[:2]) + SF.pool(t[2:])) and np.array_equal(SF.pool(t), t.sum(axis=0))
        assert np.array_equal(SF.pool(torch.from_numpy(t)).numpy(), SF.pool(t))
    whole = SF.summary(returns=tables, lags=(1, 3))
    assert whole == SF.summary(returns=[SF.pool(t) for t in tables], lags=(1, 3)) and whole["returns"]["returns"] == int(tables[0][:, 1].sum())


def _quotes_of_mids(mids):
    return np.array([(s, 3, m - 1, m + 1, 1, 1, 1, 1) for s, m in enumerate(mids)], np.int32)


def test_summary_of_an_alternating_series_has_a_negative_lag_one_autocorrelation():
    rows = _quotes_of_mids([100 + (s % 2) for s in range(41)])      # returns +2, -2, +2, ... in half units
    s = SF.summary(returns=SF.returns_from_quotes(rows, (1, 2), 1, 4), returns_k=SF.returns_from_quotes(rows, (1, 2), 2, 4), k=2, lags=(1, 2))["returns"]
    assert s["returns"] == 40 and s["mean"] == 0.0 and s["variance"] == 4.0 and s["mean_abs"] == 2.0
    assert s["lags"]["k1"]["acf"] == -1.0 and s["lags"]["k2"]["acf"] == 1.0 and s["lags"]["k1"]["n"] == 39
    assert s["lags"]["k1"]["acf_abs"] is None and s["lags"]["k1"]["leverage"] is None      # constant magnitudes: no variance to divide by
    assert s["variance_ratio"] == {"k": 2, "value": 0.0}            # two-step returns are all 0: pure bounce
    assert s["clipped_share"] == 0.0 and s["excess_kurtosis"] == pytest.approx(-2.0)       # two equal spikes
    walk = _quotes_of_mids(100 + np.cumsum(np.random.default_rng(3).integers(-1, 2, 400)))
    w = SF.summary(returns=SF.returns_from_quotes(walk, (1,), 1, 4), lags=(1,))["returns"]
    assert abs(w["lags"]["k1"]["acf"]) < 0.2 and w["clipped_share"] == 0.0
    empty = SF.summary(returns=SF.returns_from_quotes(walk[:1], (1,), 1, 1), lags=(1,))["returns"]
    assert empty["mean"] is None and empty["variance"] is None and empty["lags"]["k1"]["acf"] is None and empty["excess_kurtosis"] is None


def test_summary_of_a_constant_sign_tape_has_a_sign_autocorrelation_of_one():
    tape = np.zeros((30, 8), np.int32)
    tape[:, 2], tape[:, 3], tape[:, 6] = 2, 0, 1
    tape[:, 7] = ((np.arange(30) // 3) << 2) | 1                    # buys, three per step
    s = SF.summary(signs=SF.signs_from_records(tape, (1, 3)), lags=(1, 3))["signs"]
    assert s["fills"] == 30 and s["buy_share"] == 1.0 and s["mean_run"] == 30.0 and s["fills_per_step"] == 3.0 and s["self_share"] == 0.0
    assert s["lags"]["k1"]["acf"] == 1.0 and s["lags"]["k3"]["acf"] == 1.0
    assert s["lags"]["k1"]["same_step_share"] == pytest.approx(20 / 29) and s["lags"]["k3"]["same_step_share"] == 0.0
    alt = tape.copy()
    alt[:, 7] = (np.arange(30) << 2) | np.where(np.arange(30) % 2 == 0, 1, 2)      # buy, sell, buy, ... one per step
    a = SF.summary(signs=SF.signs_from_records(alt, (1,)), lags=(1,))["signs"]
    assert a["lags"]["k1"]["acf"] == -1.0 and a["lags"]["k1"]["acf_across_steps"] == -1.0 and a["mean_run"] == 1.0


def test_summary_of_a_flow_that_moves_the_price_has_a_positive_lambda():
    rng = np.random.default_rng(11)
    q = rng.integers(-5, 6, 60)
    mids = 200 + np.concatenate([[0], np.cumsum(q)])                # the mid moves by the bar's signed volume: r_b = 2 Q_b
    tape = np.zeros((60, 8), np.int32)
    tape[:, 2], tape[:, 7] = np.abs(q), (np.arange(60) << 2) | np.where(q >= 0, 1, 2)
    tape = tape[q != 0]
    s = SF.summary(flows=SF.flow_returns_from_records(tape, _quotes_of_mids(mids), (0, 1), 1), flow_lags=(0, 1))["flows"]
    assert s["lags"]["k0"]["lambda"] == pytest.approx(2.0) and s["lags"]["k0"]["r2"] == pytest.approx(1.0) and s["lags"]["k0"]["n"] == 60
    assert abs(s["lags"]["k1"]["corr"]) < 0.4 and s["bars_excluded"] == 0 and s["fills"] == len(tape)


# ---- 4. the refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip_lib():
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib()


def _check(L, kind, lags, bar=1, hh=16, max_step=64):
    arr = (C.c_int32 * max(1, len(lags)))(*lags)
    return L.cda_stylised_check_host(kind, arr, len(lags), bar, hh, max_step)


def test_every_invalid_argument_is_refused_by_the_product_library(hip_lib):
    L, R, S, F = hip_lib, 0, 1, 2
    for kind in (R, S, F):
        assert _check(L, kind, (1, 2, 8, 70)) == OK and _check(L, kind, (1,) * 8) == OK and _check(L, kind, (1 << 20,)) == OK
        assert _check(L, kind, ()) == INVALID and _check(L, kind, (1,) * 9) == INVALID                      # L outside 1 .. 8
        assert _check(L, kind, (1, -1)) == INVALID and _check(L, kind, ((1 << 20) + 1,)) == INVALID           # a lag out of range
        assert L.cda_stylised_check_host(kind, None, 1, 1, 16, 64) == INVALID
        assert _check(L, kind, (0, 1)) == (OK if kind == F else INVALID)                                      # lag 0: the joined table alone
    assert _check(L, 3, (1,)) == INVALID and _check(L, -1, (1,)) == INVALID
    for kind in (R, F):
        assert _check(L, kind, (1,), bar=0) == INVALID and _check(L, kind, (1,), bar=-3) == INVALID           # bar_steps < 1
        assert _check(L, kind, (1,), bar=1, max_step=4096) == OK and _check(L, kind, (1,), bar=1, max_step=4097) == INVALID      # the border: 4096 / 4097 points
        assert _check(L, kind, (1,), bar=2, max_step=8192) == OK and _check(L, kind, (1,), bar=2, max_step=8193) == INVALID
        assert _check(L, kind, (1,), bar=3, max_step=4096 * 3) == OK and _check(L, kind, (1,), bar=3, max_step=4096 * 3 + 1) == INVALID
        assert _check(L, kind, (1,), bar=2 ** 31 - 1, max_step=2 ** 31 - 1) == OK
    assert _check(L, S, (1,), bar=0, hh=0, max_step=10 ** 6) == OK                                            # signs take neither bars nor bins
    for hh in (0, -1, 65):
        assert _check(L, R, (1,), hh=hh) == INVALID and _check(L, F, (1,), hh=hh) == OK                       # hist_half outside 1 .. 64
    assert _check(L, R, (1,), hh=1) == OK and _check(L, R, (1,), hh=64) == OK
    # the entry points themselves: without an env nothing is launched
    lags = (C.c_int32 * 2)(1, 2)
    assert L.cda_quote_returns(None, 0, 1, 0, lags, 2, 1, 16, None, None, None, None, None) == INVALID
    assert L.cda_tape_signs(None, 0, 1, 0, lags, 2, None, None, None, None) == INVALID
    assert L.cda_tape_flow_returns(None, 0, 1, 0, lags, 2, 1, None, None, None, None) == INVALID


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


def test_wrappers_check_their_arguments_before_any_launch(monkeypatch):
    from gym_continuousdoubleauction_amd import vec_env as V
    stub = _StubLib()
    monkeypatch.setattr(V, "lib", lambda: stub)
    env = V.CDAVecEnv.__new__(V.CDAVecEnv)
    env._h, env.n_markets, env.num_agents, env.per_market, env.max_step = None, 8, 4, False, 8192
    env.sync = env.join = lambda: None
    calls = (env.quote_returns, env.tape_signs, env.tape_flow_returns)
    for kw in ({"episode": "next"}, {"first_market": 8}, {"n_markets": 0}, {"first_market": 5, "n_markets": 4}, {"lags": ()}, {"lags": tuple(range(1, 10))},
               {"lags": (1, -2)}, {"lags": (2 ** 20 + 1,)}):
        for call in calls:
            with pytest.raises(ValueError):
                call(**kw)
    for call in calls[:2]:
        with pytest.raises(ValueError, match="lags"):
            call(lags=(0, 1))
    for call in (env.quote_returns, env.tape_flow_returns):
        with pytest.raises(ValueError, match="bar_steps"):
            call(bar_steps=0)
        with pytest.raises(ValueError, match="bar points"):
            call(bar_steps=1)                                      # 8192 points
    for hh in (0, 65):
        with pytest.raises(ValueError, match="hist_half"):
            env.quote_returns(bar_steps=2, hist_half=hh)
    assert stub.calls == []
    stub.quotes = 0
    for call in (env.quote_returns, env.tape_flow_returns):
        with pytest.raises(RuntimeError, match="enable_quotes"):
            call(bar_steps=2)
    stub.quotes, stub.tape = 64, 0
    for call in (env.tape_signs, env.tape_flow_returns):
        with pytest.raises(RuntimeError, match="enable_tape"):
            call()
    assert stub.calls == []


def test_field_tuples_bounds_and_entry_points_are_the_header_s():
    hdr = open(os.path.join(ROOT, "include", "cda.h")).read()
    for name, value in (("CDA_STYL_MAX_BARS", SF.MAX_BARS), ("CDA_STYL_MAX_LAGS", SF.MAX_LAGS), ("CDA_STYL_MAX_HIST_HALF", SF.MAX_HIST_HALF)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), hdr), name
    assert re.search(r"#define CDA_STYL_MAX_LAG\s+\(1 << 20\)", hdr) and SF.MAX_LAG == 1 << 20
    assert (len(SF.RETURN_FIELDS), len(SF.RETURN_LAG_FIELDS), len(SF.SIGN_FIELDS), len(SF.SIGN_LAG_FIELDS), len(SF.FLOW_FIELDS), len(SF.FLOW_LAG_FIELDS)) == (8, 4, 8, 4, 4, 6)
    from gym_continuousdoubleauction_amd import _lib
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS
    inc = open(os.path.join(ROOT, "gym_continuousdoubleauction_amd", "csrc", "cda_hip.hip")).read()
    assert inc.index('#include "cda_quotes.inc"') < inc.index('#include "cda_stylised.inc"')
