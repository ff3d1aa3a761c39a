"""CPU: the quote tape's host side (gym_continuousdoubleauction_amd/quotes.py) - the episode rule, a record from a book's ladders, the statistics and the spread
report, each against answers worked by hand - the argument checking of the CDAVecEnv wrappers with the library stubbed, the .npz container and the C-ABI's
declarations.  Integers only.  No GPU."""
import os
import re

import numpy as np
import pytest

from gym_continuousdoubleauction_amd import book as BK
from gym_continuousdoubleauction_amd import quotes as Q
from gym_continuousdoubleauction_amd import tape as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["cda_quotes_enable", "cda_quotes_disable", "cda_quotes_capacity", "cda_quote_meta", "cda_quote_series", "cda_quote_stats", "cda_tape_spreads"]


def _run(meta, steps):
    for t in steps:
        meta = Q.record(meta, t)
    return meta


# ---- the episode rule ---------------------------------------------------------------------------------------------------------------------
def test_roll_a_fresh_start_and_normal_steps_change_nothing():
    m = Q.new_meta()
    assert Q.roll(m, 0) == m                                    # nothing recorded, the clock at 0: the expected step
    m = _run(m, [0, 1, 2])
    assert (m["n_total"], m["n_episode"], m["first"], m["flags"], m["n_prev"], m["gap"]) == (3, 3, 0, 0, 0, 0)
    assert Q.roll(m, 3) == m                                    # t_step == n_episode
    assert Q.span(m, 8) == {"start": 0, "count": 3, "lost": 0, "step0": 0, "partial": 0}
    assert Q.span(m, 8, "previous")["count"] == 0
    with pytest.raises(ValueError):
        Q.span(m, 8, "next")


def test_roll_a_reset_seen_late_and_a_double_reset():
    m = _run(Q.new_meta(), range(5))                            # an episode of five steps; the in-kernel auto reset put the clock back to 0
    r = Q.roll(m, 0)
    assert (r["n_total"], r["n_episode"], r["n_prev"], r["first"], r["prev_first"], r["flags"], r["gap"]) == (5, 0, 5, 0, 0, 0, 0)
    assert Q.span(r, 8, "previous") == {"start": 0, "count": 5, "lost": 0, "step0": 0, "partial": 0}
    assert Q.span(r, 8, "current")["count"] == 0
    assert Q.roll(r, 0) == r                                    # a second reset with no step between: the same row (the rule is idempotent)
    assert m["n_prev"] == 0                                     # (roll returns a new row)
    r = _run(r, [0, 1])
    assert (r["n_total"], r["n_episode"], r["n_prev"]) == (7, 2, 5)
    assert Q.span(r, 8, "previous")["start"] == 0 and Q.span(r, 8, "current") == {"start": 5, "count": 2, "lost": 0, "step0": 0, "partial": 0}
    r = Q.roll(r, 0)                                            # a reset in mid-episode: the two steps become the previous episode
    assert (r["n_prev"], r["n_episode"]) == (2, 0) and Q.span(r, 8, "previous")["start"] == 5


def test_roll_a_restore_forward_and_backward_keeps_the_previous_episode():
    base = _run(Q.roll(_run(Q.new_meta(), range(6)), 0), range(10))      # a finished episode of 6, then 10 steps of the next
    assert (base["n_prev"], base["n_episode"], base["n_total"]) == (6, 10, 16)
    for t in (30, 4):                                           # forward, backward
        r = Q.roll(base, t)
        assert (r["n_episode"], r["first"], r["gap"], r["flags"], r["n_prev"], r["prev_first"]) == (0, t, 10, Q.PARTIAL, 6, 0), t
        assert Q.span(r, 64, "previous") == {"start": 0, "count": 6, "lost": 0, "step0": 0, "partial": 0}
        assert Q.span(r, 64, "current") == {"start": 16, "count": 0, "lost": 0, "step0": t, "partial": 1}
        r = _run(r, [t, t + 1])                                 # the next records land at the restored step
        assert (r["n_episode"], r["first"], r["n_total"]) == (2, t, 18) and Q.roll(r, t + 2) == r
        assert Q.span(r, 64, "current") == {"start": 16, "count": 2, "lost": 0, "step0": t, "partial": 1}
        r = Q.roll(r, 0)                                        # the reset behind it: the partial tail becomes the previous episode, flag and all
        assert (r["n_prev"], r["prev_first"], r["flags"], r["gap"], r["first"]) == (2, t, Q.PREV_PARTIAL, 0, 0)
        assert Q.span(r, 64, "previous") == {"start": 16, "count": 2, "lost": 0, "step0": t, "partial": 1}
    r = Q.roll(Q.roll(base, 30), 0)                             # a restore to step 0 of an episode: complete from its first step, hence not partial
    assert (r["first"], r["flags"], r["gap"], r["n_prev"]) == (0, 0, 10, 6)
    r = Q.roll(Q.roll(base, 30), 12)                            # two restores in a row: the gap does not grow (nothing was recorded between them)
    assert (r["first"], r["gap"]) == (12, 10)


def test_span_of_a_ring_that_wrapped():
    m = _run(Q.roll(_run(Q.new_meta(), range(4)), 0), range(6))          # 4 + 6 records through a ring of 4: it holds records 6 .. 9
    assert Q.span(m, 4, "current") == {"start": 6, "count": 4, "lost": 2, "step0": 2, "partial": 0}
    assert Q.span(m, 4, "previous") == {"start": 4, "count": 0, "lost": 4, "step0": 4, "partial": 0}
    assert Q.span(m, 7, "previous") == {"start": 3, "count": 1, "lost": 3, "step0": 3, "partial": 0}
    assert Q.span(m, 16, "previous") == {"start": 0, "count": 4, "lost": 0, "step0": 0, "partial": 0}
    words = np.array([10, 0, 6, 4, 0, 0, 0, 0], np.int32)
    assert Q.meta_from_words(words) == m
    assert Q.meta_from_words(np.array([-1, 1, 0, 0, 0, 0, 0, 0], np.int32))["n_total"] == 2 ** 33 - 1      # the 64-bit pair


# ---- a record from a book ------------------------------------------------------------------------------------------------------------------
def test_quote_from_levels_on_hand_built_books():
    none = np.zeros((0, 5), np.int32)
    assert Q.quote_from_orders(7, none, none).tolist() == [7, 0, 0, 0, 0, 0, 0, 0]
    # (price, qty, owner, order_id, timestamp), queue order: three orders on the best bid, two levels behind; one ask
    bids = np.array([[50, 3, 0, 1, 1], [50, 4, 1, 2, 2], [50, 10, 0, 5, 9], [49, 100, 2, 3, 3], [40, 1, 1, 4, 4]], np.int32)
    asks = np.array([[53, 6, 2, 6, 5]], np.int32)
    assert Q.quote_from_orders(0, bids, none).tolist() == [0, Q.BID, 50, 0, 17, 0, 3, 0]
    assert Q.quote_from_orders(3, none, asks).tolist() == [3, Q.ASK, 0, 53, 0, 6, 0, 1]
    got = Q.quote_from_orders(12, bids, asks)
    assert got.dtype == np.int32 and got.tolist() == [12, Q.BID | Q.ASK, 50, 53, 17, 6, 3, 1]
    assert got.tolist() == Q.quote_from_levels(12, BK.levels_from_orders(bids, 4), BK.levels_from_orders(asks, 4)).tolist()      # deeper ladders: the same
    rec = Q.as_quotes(got[None])
    assert (rec["step"][0], rec["bid_price"][0], rec["ask_price"][0], rec["bid_volume"][0], rec["ask_orders"][0]) == (12, 50, 53, 17, 1)
    # a level sum beyond int32 is clamped and flagged, never wrapped
    big = Q.quote_from_levels(1, [[50, 2 ** 31 + 5, 3]], [[53, 2 ** 31 - 1, 2]])
    assert big.tolist() == [1, Q.BID | Q.ASK | Q.SATURATED, 50, 53, 2 ** 31 - 1, 2 ** 31 - 1, 3, 2]
    with pytest.raises(ValueError):
        Q.as_rows(np.zeros((3, 7), np.int32))


# ---- statistics ------------------------------------------------------------------------------------------------------------------------------
# ten steps with a one-sided gap in the middle: (flags, bid, ask, bid volume, ask volume)
SERIES = [(3, 10, 12, 5, 7), (3, 10, 12, 5, 7), (3, 11, 13, 3, 2), (3, 11, 12, 4, 1), (1, 11, 0, 9, 0), (0, 0, 0, 0, 0), (2, 0, 13, 0, 8), (3, 9, 13, 1, 1),
          (3, 10, 12, 2, 2), (3, 12, 14, 6, 6)]


def _series_rows(step0=0):
    return np.array([[step0 + i, f, b, a, bv, av, 1 if f & 1 else 0, 1 if f & 2 else 0] for i, (f, b, a, bv, av) in enumerate(SERIES)], np.int32)


def test_stats_from_quotes_on_a_series_worked_by_hand():
    got = dict(zip(Q.STAT_FIELDS, Q.stats_from_quotes(_series_rows()).tolist()))
    # spreads of the seven two-sided steps: 2 2 2 1 | 4 2 2; m2: 22 22 24 23 | 22 22 26; neighbours both two-sided: (0,1) (1,2) (2,3) (7,8) (8,9), m2 moves 0 +2 -1 0 +4
    assert got == {"steps": 10, "two_sided": 7, "bid_only": 1, "ask_only": 1, "empty": 1, "spread_sum": 15, "spread_sq": 37, "spread_min": 1, "spread_max": 4,
                   "m2_sum": 161, "bid_volume": 26, "ask_volume": 26, "pairs": 5, "m2_changes": 3, "abs_dm2": 7, "dm2_sq": 21}
    assert Q.stats_from_quotes(np.zeros((0, 8), np.int32)).tolist() == [0] * 16
    one_sided = _series_rows()[4:7]
    assert Q.stats_from_quotes(one_sided).tolist() == [3, 0, 1, 1, 1] + [0] * 11
    s = Q.stats_summary(Q.stats_from_quotes(_series_rows()))
    assert s["mean_spread"] == 15 / 7 and s["mean_mid"] == 161 / 14 and s["mid_change_share"] == 3 / 5 and s["realised_variance_per_step"] == 21 / 20
    assert Q.stats_summary(np.zeros(16, np.int64))["mean_spread"] is None


# ---- spread report ---------------------------------------------------------------------------------------------------------------------------
def _fill(step, price, qty, maker, maker_side, taker):
    return [0, price, qty, maker, 0, -1, taker, int(TP.pack_sides_step(maker_side, maker_side ^ 1, step))]


def test_spreads_from_records_on_a_hand_built_tape_and_series():
    # the ring lost the quotes of steps 0 and 1; step 4 is one-sided; the last held step is 7
    quotes = np.array([[2, 3, 10, 12, 1, 1, 1, 1], [3, 3, 10, 14, 1, 1, 1, 1], [4, 1, 10, 0, 1, 0, 1, 0], [5, 3, 11, 13, 1, 1, 1, 1], [6, 3, 12, 14, 1, 1, 1, 1],
                       [7, 3, 12, 13, 1, 1, 1, 1]], np.int32)
    tape = np.array([_fill(1, 12, 5, 0, 1, 1),          # its quote was overwritten                                     -> unquoted at both horizons
                     _fill(2, 12, 4, 0, 1, 1),          # agent 1 lifts agent 0's ask: 2p - m2 = 24 - 22 = 2; later 24 - 24 = 0 at step 3 and at step 5
                     _fill(2, 11, 9, 2, 0, 2),          # a self-trade                                                  -> skipped
                     _fill(3, 14, 1, 1, 1, 0),          # agent 0 lifts agent 1's ask: k = 1 meets the one-sided step 4 -> unquoted; k = 3: 28 - 24 = 4, later 28 - 26 = 2
                     _fill(4, 10, 2, 1, 0, 2),          # on the one-sided step                                         -> unquoted at both horizons
                     _fill(5, 11, 3, 2, 0, 0)],         # agent 0 hits agent 2's bid: 22 - 24 = -2, later 22 - 26 = -4, sold: x -1; k = 3: step 8 is past the end -> open
                    np.int32)
    got = Q.spreads_from_records(tape, quotes, (1, 3), 3)
    want = np.array([
        [[[-8, 0, 4, 1, 0, 1], [6, 12, 3, 1, 0, 1]], [[-8, 0, 4, 1, 0, 1], [4, 2, 1, 1, 1, 0]]],
        [[[0, 0, 0, 0, 0, 2], [8, 0, 4, 1, 0, 1]], [[-4, -2, 1, 1, 0, 1], [8, 0, 4, 1, 0, 1]]],
        [[[-6, -12, 3, 1, 0, 0], [0, 0, 0, 0, 0, 1]], [[0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1]]]], np.int64)
    assert got.dtype == np.int64 and got.shape == (3, 2, 2, 6)
    assert np.array_equal(got, want), np.argwhere(got != want)
    # every non-self fill is in exactly one of the three bins, in both roles
    assert (got[..., 3] + got[..., 4] + got[..., 5]).sum() == 2 * 5 * 2
    # without any quote every fill is open; without any fill the table is zero
    none = Q.spreads_from_records(tape, np.zeros((0, 8), np.int32), (1, 3), 3)
    assert none[..., 4].sum() == 20 and none[..., [0, 1, 2, 3, 5]].sum() == 0
    assert not Q.spreads_from_records(np.zeros((0, 8), np.int32), quotes, (1,), 3).any()
    s = Q.spread_summary(got[1], horizons=(1, 3))
    assert s["k1"]["taker"] == {"effective_half_spread": 1.0, "realised_half_spread": 0.0, "impact": 1.0, "qty": 4, "fills": 1, "open_fills": 0, "unquoted_fills": 1,
                                "coverage": 0.5}
    assert s["k1"]["maker"]["effective_half_spread"] is None and s["k3"]["maker"]["realised_half_spread"] == -1.0
    for bad in ((), tuple(range(9)), (-1,)):
        with pytest.raises(ValueError):
            Q.spreads_from_records(tape, quotes, bad, 3)
    with pytest.raises(ValueError):
        Q.spreads_from_records(tape, quotes, (1,), 2)              # agent 2 is on the tape
    with pytest.raises(ValueError):
        Q.spreads_from_records(tape, quotes[[0, 2, 3]], (1,), 3)   # not consecutive steps


def test_spreads_by_module_sums_the_slots_of_a_module():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    sp = torch.from_numpy(rng.integers(-50, 50, (4, 3, 2, 2, 6)).astype(np.int64))
    mod = torch.tensor([[0, 1, 1], [2, 0, 1], [1, 1, 1], [0, 0, 2]], dtype=torch.int32)
    got = Q.spreads_by_module(sp, mod, 3).numpy()
    want = np.zeros((3, 2, 2, 6), np.int64)
    for i in range(4):
        for a in range(3):
            want[int(mod[i, a])] += sp[i, a].numpy()
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        Q.spreads_by_module(sp, mod, 2)
    with pytest.raises(ValueError):
        Q.spreads_by_module(sp[..., :5], mod, 3)


# ---- the wrappers' argument checking, the library stubbed ------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self, tape=0, quotes=0):
        self.tape, self.quotes, self.calls = tape, quotes, []

    def cda_tape_capacity(self, h):
        return self.tape

    def cda_quotes_capacity(self, h):
        return self.quotes

    def cda_quotes_enable(self, h, capacity):
        self.calls.append(("enable", capacity)); self.quotes = capacity
        return 0

    def cda_quotes_disable(self, h):
        self.calls.append(("disable",)); self.quotes = 0
        return 0


def _stub_env(monkeypatch, **kw):
    from gym_continuousdoubleauction_amd import vec_env as V
    stub = _StubLib(**kw)
    monkeypatch.setattr(V, "lib", lambda: stub)
    env = V.CDAVecEnv.__new__(V.CDAVecEnv)
    env._h, env.n_markets, env.num_agents, env.quote_epoch, env.per_market, env.max_step = None, 8, 4, 0, False, 16
    env.sync = env.join = lambda: None
    return env, stub


def test_wrappers_check_their_arguments_before_any_launch(monkeypatch):
    env, stub = _stub_env(monkeypatch)
    for bad in (0, -4, (1 << 20) + 1):
        with pytest.raises(ValueError, match="capacity"):
            env.enable_quotes(bad)
    assert stub.calls == [] and env.quote_epoch == 0 and not env.quotes_enabled
    for call in (env.quote_series, env.quote_stats, env.quote_meta, env.tape_spreads):
        with pytest.raises(RuntimeError, match="enable_"):
            call()
    env.enable_quotes(40)                                       # any capacity >= 1, not only powers of two
    assert stub.calls == [("enable", 40)] and env.quote_epoch == 1 and env.quotes_enabled and env.quote_capacity == 40
    with pytest.raises(RuntimeError, match="enable_tape"):
        env.tape_spreads()                                      # quotes alone do not make a spread report
    stub.tape = 64
    for kw in ({"episode": "next"}, {"first_market": 8}, {"first_market": -1}, {"n_markets": 0}, {"first_market": 5, "n_markets": 4}):
        for call in (env.quote_series, env.quote_stats, env.tape_spreads):
            with pytest.raises(ValueError):
                call(**kw)
    with pytest.raises(ValueError):
        env.quote_meta(first_market=7, n_markets=2)
    for k in (0, -1):
        with pytest.raises(ValueError, match="k must"):
            env.quote_series(k)
    for hz in ((), tuple(range(1, 10)), (1, -5)):
        with pytest.raises(ValueError, match="horizons"):
            env.tape_spreads(hz)
    env.disable_quotes()
    assert env.quote_epoch == 2 and not env.quotes_enabled and stub.calls[-1] == ("disable",)


# ---- container and declarations --------------------------------------------------------------------------------------------------------------
def test_npz_round_trip(tmp_path):
    rec = np.zeros((2, 12, 8), np.int32)
    rec[0, :10] = _series_rows()
    rec[1, :3] = _series_rows(5)[:3]
    path = str(tmp_path / "q.npz")
    Q.save(path, rec, counts=np.array([10, 3]), info=np.array([[10, 0, 0, 0], [3, 2, 5, 1]], np.int32), module=np.array([4, 7], np.int32))
    back = Q.load(path)
    assert np.array_equal(back["records"], rec) and back["records"].dtype == np.int32 and back["counts"].tolist() == [10, 3]
    assert tuple(back["fields"]) == Q.FIELDS and back["module"].tolist() == [4, 7] and back["info"][1].tolist() == [3, 2, 5, 1]
    assert np.array_equal(Q.stats_from_quotes(back["records"][0, :back["counts"][0]]), Q.stats_from_quotes(_series_rows()))
    Q.save(path, Q.as_quotes(_series_rows()))                   # a structured array of one market
    assert np.array_equal(Q.load(path)["records"], _series_rows())
    with pytest.raises(ValueError):
        Q.save(path, np.zeros((3, 7), np.int32))


def test_record_dtype_and_entry_points_are_the_header_s():
    hdr = open(os.path.join(ROOT, "include", "cda.h")).read()
    body = re.search(r"typedef struct cda_quote_record \{(.*?)\} cda_quote_record;", hdr, re.S).group(1)
    assert tuple(re.findall(r"int32_t (\w+);", body)) == Q.FIELDS and Q.QUOTE_DTYPE.itemsize == 32
    for name, value in (("CDA_QUOTE_WORDS", Q.QUOTE_WORDS), ("CDA_QUOTE_STAT_WORDS", Q.STAT_WORDS), ("CDA_QUOTE_BID", Q.BID), ("CDA_QUOTE_ASK", Q.ASK),
                        ("CDA_QUOTE_SATURATED", Q.SATURATED)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), hdr), name
    assert re.search(r"#define CDA_QUOTE_CAP_MAX\s+\(1 << 20\)", hdr) and Q.CAP_MAX == 1 << 20
    from gym_continuousdoubleauction_amd import _capi, _lib
    assert _capi.QUOTE_WORDS == Q.QUOTE_WORDS and _capi.QUOTE_STAT_WORDS == Q.STAT_WORDS and Q.MAX_HORIZONS == _capi.TAPE_MAX_HORIZONS
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|int64_t) %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS
