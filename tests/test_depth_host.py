"""CPU: the depth tape's host side (gym_continuousdoubleauction_amd/depth.py) - the record from the book's ladders, the three specifications on hand-worked
records, the pooling, the replay of the recorder's episode rule (tests/depth_replay.py) - and the argument check of the product library
(cda_depth_check_host: no env, no device).  Integers only: every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from depth_replay import DepthReplay
from gym_continuousdoubleauction_amd import book as B
from gym_continuousdoubleauction_amd import depth as D
from gym_continuousdoubleauction_amd import quotes as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["cda_depth_enable", "cda_depth_disable", "cda_depth_capacity", "cda_depth_levels", "cda_depth_meta", "cda_depth_series", "cda_depth_profile",
                "cda_depth_imbalance", "cda_depth_ofi", "cda_depth_check_host"]
OK, INVALID = 0, -1
BIG = 2 ** 31 - 1


def rec(step, bids, asks, levels, extra=0):
    """a record from (price, volume) lists, best first, at most `levels` per side"""
    out = np.zeros((1 + levels, 4), np.int64)
    out[0] = step, (D.BID if bids else 0) | (D.ASK if asks else 0) | extra, len(bids), len(asks)
    for l, (p, v) in enumerate(bids):
        out[1 + l, :2] = p, v
    for l, (p, v) in enumerate(asks):
        out[1 + l, 2:] = p, v
    return out.reshape(-1).astype(np.int32)


def orders(levels):
    """get_book()-style rows [n, 5] from (price, [quantities]) levels, best first"""
    rows = [(p, q, 0, 0, 0) for p, qs in levels for q in qs]
    return np.array(rows, np.int32).reshape(-1, 5)


# ---- 1. a record ---------------------------------------------------------------------------------------------------------------------------------
def test_record_from_levels_flags_counts_and_zero_rows():
    L = 3
    bids = orders([(50, [3, 4]), (49, [1]), (47, [2, 2, 2])])            # exactly `levels` levels: no more bit
    asks = orders([(52, [5]), (53, [1]), (55, [1]), (60, [9])])          # levels + 1: the more bit
    r = D.record_from_orders(7, bids, asks, L)
    assert r.tolist() == [7, D.BID | D.ASK | D.ASK_MORE, 3, 3, 50, 7, 52, 5, 49, 1, 53, 1, 47, 6, 55, 1]
    d = D.as_depth(r, L)[0]
    assert d["step"] == 7 and d["bid_levels"] == 3 and d["level"]["ask_price"].tolist() == [52, 53, 55] and d["level"]["bid_volume"].tolist() == [7, 1, 6]
    one = D.record_from_orders(0, bids[:2], orders([]), L)                # one level on one side, none on the other: zero rows behind the counts
    assert one.tolist() == [0, D.BID, 1, 0, 50, 7, 0, 0] + [0] * 8
    assert D.record_from_orders(3, orders([]), orders([]), L).tolist() == [3] + [0] * 15
    more_bid = D.record_from_orders(0, orders([(9, [1]), (8, [1]), (7, [1]), (6, [1]), (5, [1])]), asks[:1], L)
    assert more_bid[1] == D.BID | D.ASK | D.BID_MORE and more_bid[2:4].tolist() == [3, 1]
    with pytest.raises(ValueError, match="levels \\+ 1"):
        D.record_from_levels(0, B.levels_from_orders(bids, L), B.levels_from_orders(asks, L), L)      # without the extra row the more bit is undecidable
    for bad in (0, 17):
        with pytest.raises(ValueError, match="levels"):
            D.record_dtype(bad)
    assert D.record_dtype(16).itemsize == 17 * 16 and D.record_words(10) == 44


def test_a_saturated_volume_is_clamped_and_flagged():
    lv = np.zeros((3, 3), np.int64)
    lv[0] = 50, 2 ** 31 + 5, 3
    lv[1] = 49, BIG, 1                                                    # INT32_MAX itself is not saturated
    ask = np.zeros((3, 3), np.int64)
    ask[0] = 51, 7, 1
    r = D.record_from_levels(2, lv, ask, 2)
    assert r.tolist() == [2, D.BID | D.ASK | D.SATURATED, 2, 1, 50, BIG, 51, 7, 49, BIG, 0, 0]
    lv[0, 1] = BIG
    assert D.record_from_levels(2, lv, ask, 2)[1] == D.BID | D.ASK


@pytest.mark.parametrize("seed", range(6))
def test_level_0_agrees_with_the_quote_record(seed):
    rng = np.random.default_rng(seed)
    side = lambda lo, n: orders([(int(p), rng.integers(1, 9, rng.integers(1, 4)).tolist()) for p in lo + np.sort(rng.choice(30, n, replace=False))])   # noqa: E731
    bids, asks = side(10, int(rng.integers(0, 6)))[::-1], side(60, int(rng.integers(0, 6)))
    bids = bids[np.argsort(-bids[:, 0], kind="stable")] if len(bids) else bids
    r, q = D.record_from_orders(5, bids, asks, 4), Q.quote_from_orders(5, bids, asks)
    assert (r[0], r[1] & 7, r[4], r[6], r[5], r[7]) == (q[0], q[1], q[2], q[3], q[4], q[5])
    assert r[2] == min(4, len(set(bids[:, 0].tolist()))) and r[3] == min(4, len(set(asks[:, 0].tolist())))


# ---- 2. the profile ----------------------------------------------------------------------------------------------------------------------------------
def test_profile_on_hand_worked_records_with_a_clipped_distance():
    L = 3
    rows = np.array([rec(0, [(100, 5), (98, 2), (90, 7)], [(102, 1), (104, 3)], L, D.BID_MORE),
                     rec(1, [(100, 4)], [], L),
                     rec(2, [], [(110, 6), (112, 1), (150, 2)], L, D.ASK_MORE | D.SATURATED)])
    base, lev, shape = D.profile_from_records(rows, L, max_dist=4, tick=2)
    assert base.tolist() == [3, 1, 1, 1, 1, 4, 5, 0]
    assert lev[0].tolist() == [[2, 9, 0], [1, 2, 1], [1, 7, 5]] and lev[1].tolist() == [[2, 7, 0], [2, 4, 2], [1, 2, 20]]
    assert shape[0].tolist() == [9, 2, 0, 0, 7]                          # distance 5 ticks lands in the clip bin 4
    assert shape[1].tolist() == [7, 4, 0, 0, 2]                          # ... and 20 ticks too
    assert D.profile_from_records(rows, L, max_dist=5, tick=2)[2][0].tolist() == [9, 2, 0, 0, 0, 7]      # exactly max_dist: the last bin, unclipped
    empty = D.profile_from_records(np.zeros((0, 16), np.int32), L, 4)
    assert not empty[0].any() and not empty[1].any() and not empty[2].any()
    for bad in (0, 257):
        with pytest.raises(ValueError, match="max_dist"):
            D.profile_from_records(rows, L, bad)
    with pytest.raises(ValueError, match="consecutive"):
        D.profile_from_records(rows[[0, 2]], L, 4)


# ---- 3. the imbalance ----------------------------------------------------------------------------------------------------------------------------------
def test_imbalance_bins_at_the_edges():
    assert D.imbalance_bin(5, 5, 8) == 8                                 # B == A: bin `half`
    assert D.imbalance_bin(10 ** 9, 1, 8) == 15 and D.imbalance_bin(1, 10 ** 9, 8) == 0
    assert D.imbalance_bin(7, 1, 4) == 7 and D.imbalance_bin(3, 1, 4) == 6 and D.imbalance_bin(1, 3, 4) == 2 and D.imbalance_bin(1, 0, 1) == 1


def test_imbalance_on_hand_worked_records_with_a_lag_past_the_end():
    L, half = 2, 4
    rows = np.array([rec(0, [(100, 5), (99, 5)], [(102, 5), (103, 5)], L),      # B = A -> bin 4;       m2 = 202
                     rec(1, [(100, 90), (99, 9)], [(104, 1)], L),              # B >> A -> bin 7;      m2 = 204
                     rec(2, [(101, 1)], [(103, 50), (104, 49)], L),            # B << A -> bin 0;      m2 = 204
                     rec(3, [(101, 1)], [], L),                                # one-sided
                     rec(4, [(99, 3)], [(103, 1)], L)])                        # 3 : 1 -> bin 6;       m2 = 202
    resp, base = D.imbalance_from_records(rows, L, (1, 2, 9), k=2, half=half)
    assert base.tolist() == [5, 4, (10 - 10) + (99 - 1) + (1 - 99) + (3 - 1), 20 + 100 + 100 + 4]
    want = np.zeros((3, 8, 5), np.int64)
    want[0, 4] = 1, 2, 4, 1, 0                                           # lag 1: step 0 -> 1 (+2), 1 -> 2 (0); 2 -> 3 and 3 -> 4 undefined
    want[0, 7] = 1, 0, 0, 0, 0
    want[1, 4] = 1, 2, 4, 1, 0                                           # lag 2: 0 -> 2 (+2), 2 -> 4 (-2); 1 -> 3 undefined
    want[1, 0] = 1, -2, 4, 0, 1
    assert np.array_equal(resp, want) and not resp[2].any()              # a lag past the end yields zeros
    k1 = D.imbalance_from_records(rows, L, (1,), k=1, half=half)
    assert k1[1].tolist() == [5, 4, 0 + 89 - 49 + 2, 10 + 91 + 51 + 4] and k1[0][0, 0].tolist() == [0] * 5      # level 0 alone: step 2 is 1 : 50 -> bin 0, no defined r at lag 1
    for kw in ({"k": 0}, {"k": 3}, {"half": 0}, {"half": 65}):
        with pytest.raises(ValueError, match="k must be"):
            D.imbalance_from_records(rows, L, (1,), **dict({"k": 1, "half": 4}, **kw))
    with pytest.raises(ValueError, match="lags"):
        D.imbalance_from_records(rows, L, (0,), 1, 4)


# ---- 4. the order-flow imbalance -------------------------------------------------------------------------------------------------------------------------
def test_ofi_terms_of_appearing_and_vanishing_levels_on_each_side():
    L = 2
    a = rec(0, [(100, 5)], [(102, 7)], L)
    assert D.ofi_terms(a, rec(1, [(100, 5), (99, 4)], [(102, 7)], L), L).tolist() == [0, 4]              # a bid level appears: + its volume
    assert D.ofi_terms(rec(0, [(100, 5), (99, 4)], [(102, 7)], L), a, L).tolist() == [0, -4]             # ... vanishes: - its volume
    assert D.ofi_terms(a, rec(1, [(100, 5)], [(102, 7), (103, 6)], L), L).tolist() == [0, -6]            # an ask level appears: - its volume
    assert D.ofi_terms(rec(0, [(100, 5)], [(102, 7), (103, 6)], L), a, L).tolist() == [0, 6]             # ... vanishes: + its volume
    assert D.ofi_terms(a, rec(1, [(101, 2)], [(102, 3)], L), L).tolist() == [2 + (7 - 3), 0]              # bid up: + new volume; ask stays: q' - q
    assert D.ofi_terms(a, rec(1, [(99, 2)], [(101, 3)], L), L).tolist() == [-5 - 3, 0]                   # bid down: - old volume; ask down: - new volume
    assert D.ofi_terms(a, rec(1, [(100, 8)], [(104, 3)], L), L).tolist() == [3 + 7, 0]                   # bid stays: q - q'; ask up: + old volume
    assert D.ofi_terms(a, rec(1, [], [], L), L).tolist() == [-5 + 7, 0] and D.ofi_terms(rec(0, [], [], L), a, L).tolist() == [5 - 7, 0]


def test_ofi_on_hand_worked_records_bars_lags_and_a_lost_head():
    L = 2
    rows = np.array([rec(4, [(100, 5)], [(102, 7)], L),
                     rec(5, [(101, 2)], [(102, 3)], L),                  # e = (2 + 4, 0)
                     rec(6, [(101, 2), (100, 4)], [(102, 3)], L),        # e = (0, 4)
                     rec(7, [(101, 2), (100, 4)], [(103, 1)], L, D.SATURATED),      # e = (3, 0)
                     rec(8, [(101, 6), (100, 4)], [(103, 1)], L),        # e = (4, 0)
                     rec(9, [(102, 1)], [(104, 2)], L)])                 # e = (1 + 1, -4)
    lag, base = D.ofi_from_records(rows, L, (0, 1, 7), bar_steps=2, depths=(1, 2), head_lost=True)
    # steps 4 .. 9, bars of 2: the head is lost, so bars 0 .. 2 (up to the bar of step 4) are excluded; bars 3 = {6, 7} and 4 = {8, 9} are kept and complete
    assert base.tolist() == [4, 2, 3, 1]
    # points: 2 (step 4, m2 202), 3 (step 6, 203), 4 (step 8, 204); r_2 = 1, r_3 = 1, r_4 undefined (step 10 is not held)
    # OFI_1: bar 3 = 0 + 3 = 3, bar 4 = 4 + 2 = 6; OFI_2: bar 3 = 4 + 3 = 7, bar 4 = 4 - 2 = 2
    assert lag[0, 0].tolist() == [1, 3, 1, 3, 9, 1] and lag[1, 0].tolist() == [1, 7, 1, 7, 49, 1]       # lag 0: bar 3 alone (r_4 is undefined)
    assert not lag[:, 1].any() and not lag[:, 2].any()                   # lag 1: r_4, r_5 undefined; a lag past the end: zeros
    lag, base = D.ofi_from_records(rows, L, (0, 1), bar_steps=1, depths=(2,), head_lost=True)
    assert base.tolist() == [5, 5, 5, 1]                                 # bars 0 .. 4 excluded; the pairs of steps 5 .. 9
    e2 = [6, 4, 3, 4, -2]                                                # OFI_2 of steps 5 .. 9; r of points 5 .. 8 = 0, 1, 0, 2 (m2 203, 203, 204, 204, 206)
    r = [0, 1, 0, 2]
    assert lag[0, 0].tolist() == [4, sum(e2[:4]), sum(r), sum(q * x for q, x in zip(e2, r)), sum(q * q for q in e2[:4]), sum(x * x for x in r)]
    assert lag[0, 1].tolist() == [3, sum(e2[:3]), sum(r[1:]), sum(q * x for q, x in zip(e2, r[1:])), sum(q * q for q in e2[:3]), sum(x * x for x in r[1:])]
    whole = np.array([rec(s, [(100 + s, 1)], [(110 + s, 1)], L) for s in range(4)])
    lag, base = D.ofi_from_records(whole, L, (0,), 2, (1,))
    assert base.tolist() == [3, 2, 0, 0] and lag[0, 0].tolist() == [1, 1 + 1, 4, 8, 4, 16]               # a complete episode: bar 0 is kept, its first step has no pair
    assert D.ofi_from_records(whole[:0], L, (0,), 2, (1,))[1].tolist() == [0, 0, 0, 0]
    for bad in ((), (0,), (3,), (1, 1, 1, 1, 1)):
        with pytest.raises(ValueError, match="depths"):
            D.ofi_from_records(whole, L, (0,), 1, bad)


def test_a_bar_s_ofi_is_an_int32_word():
    L = 1
    rows = np.array([rec(0, [(100, 1)], [(102, 1)], L), rec(1, [(101, BIG)], [(102, 1)], L), rec(2, [(102, BIG)], [(103, 1)], L), rec(3, [(102, 1)], [(103, 1)], L)])
    lag, base = D.ofi_from_records(rows, L, (0,), 4, (1,))               # one bar: BIG + (BIG + 1) + (1 - BIG) = 2^31 + 1 wraps to -(2^31 - 1)
    assert base.tolist() == [3, 1, 0, 0] and not lag.any()               # (no return: the second point is not held)
    rows = np.concatenate([rows, [rec(4, [(102, 1)], [(103, 1)], L)]])
    lag, _ = D.ofi_from_records(rows, L, (0,), 4, (1,))
    q = -(2 ** 31 - 1)
    assert lag[0, 0].tolist() == [1, q, 3, 3 * q, q * q, 9]


# ---- 5. folding and reading --------------------------------------------------------------------------------------------------------------------------------
def _random_rows(rng, steps, L, step0=0):
    rows = []
    for s in range(steps):
        nb, na = int(rng.integers(0, L + 1)), int(rng.integers(0, L + 1))
        bp = 100 - np.sort(rng.choice(20, nb, replace=False))
        ap = 101 + np.sort(rng.choice(20, na, replace=False))
        rows.append(rec(step0 + s, [(int(p), int(rng.integers(1, 50))) for p in bp], [(int(p), int(rng.integers(1, 50))) for p in ap], L,
                        (D.BID_MORE if nb == L and rng.random() < 0.5 else 0)))
    return np.array(rows, np.int32).reshape(-1, D.record_words(L))


def test_pool_is_additive_over_a_split_of_the_episode_s_markets():
    import torch
    rng, L = np.random.default_rng(4), 4
    markets = [_random_rows(rng, 40, L) for _ in range(5)]
    prof = [D.profile_from_records(m, L, 8) for m in markets]
    imb = [D.imbalance_from_records(m, L, (1, 3), 3, 4) for m in markets]
    ofi = [D.ofi_from_records(m, L, (0, 2), 3, (1, 4)) for m in markets]
    for tables in (prof, imb, ofi):
        for j in range(len(tables[0])):
            stack = np.stack([t[j] for t in tables])
            assert np.array_equal(D.pool(stack), D.pool(stack[:2]) + D.pool(stack[2:]))
            assert np.array_equal(D.pool(torch.from_numpy(stack)).numpy(), D.pool(stack))
    s = D.summary(profile=[D.pool(np.stack([t[j] for t in prof])) for j in range(3)], imbalance=[D.pool(np.stack([t[j] for t in imb])) for j in range(2)],
                  ofi=[D.pool(np.stack([t[j] for t in ofi])) for j in range(2)], lags=(1, 3), ofi_lags=(0, 2), depths=(1, 4))
    assert s["profile"]["steps"] == 200 and len(s["profile"]["bid"]["mean_depth"]) == L and abs(sum(s["profile"]["ask"]["shape"]) - 1.0) < 1e-12
    assert s["profile"]["bid"]["mean_distance"][0] == 0.0 and 0.0 < s["profile"]["bid"]["truncation_share"] < 1.0
    assert set(s["imbalance"]["response"]) == {"k1", "k3"} and len(s["imbalance"]["response"]["k1"]) == 8
    assert set(s["ofi"]["regression"]) == {"K1", "K4"} and set(s["ofi"]["regression"]["K1"]) == {"k0", "k2"} and s["ofi"]["bars_excluded"] == 0


def test_summary_reads_the_regression_of_a_complete_episode():
    L = 1
    mids, rows = 100, []
    rng = np.random.default_rng(3)
    for s in range(80):                                              # the best bid's volume change of this step is the mid's move of the next
        q = int(rng.integers(1, 9))
        rows.append(rec(s, [(mids - 1, q)], [(mids + 1, 5)], L))
        mids += 0 if s == 0 else (1 if q > rows[-2][5] else -1 if q < rows[-2][5] else 0)
    s = D.summary(ofi=D.ofi_from_records(np.array(rows), L, (0, 1), 1, (1,)), ofi_lags=(0, 1), depths=(1,))["ofi"]
    k0, k1 = s["regression"]["K1"]["k0"], s["regression"]["K1"]["k1"]      # bar 0 is kept (its first step has no pair: OFI 0); the last point has no return
    assert s["pairs"] == 79 and k0["n"] == 79 and k1["n"] == 78 and s["bars_kept"] == 80 and k0["slope"] is not None and 0.0 <= k0["r_squared"] <= 1.0


def test_save_and_load_round_trip(tmp_path):
    L = 3
    rows = _random_rows(np.random.default_rng(8), 12, L).reshape(2, 6, -1)
    D.save(str(tmp_path / "d.npz"), rows, L, counts=[6, 5], info=np.zeros((2, 4), np.int32))
    z = D.load(str(tmp_path / "d.npz"))
    assert np.array_equal(z["records"], rows) and int(z["levels"]) == L and z["counts"].tolist() == [6, 5] and z["info"].shape == (2, 4)
    assert D.as_depth(z["records"][1], int(z["levels"]))["step"].tolist() == list(range(6, 12))
    with pytest.raises(ValueError, match="shape"):
        D.save(str(tmp_path / "e.npz"), rows, L + 1)


# ---- 6. the replay of the recorder's episode rule ----------------------------------------------------------------------------------------------------------------
def test_the_replay_follows_resets_restores_and_a_short_ring():
    L = 2
    rp = DepthReplay(1, capacity=4, levels=L)
    row = lambda s: rec(s, [(100, s + 1)], [(102, 1)], L)                # noqa: E731
    for s in range(6):
        rp.visit(0, s, row(s)); rp.clock(0, s + 1)
    rows, count, lost, step0, partial = rp.held(0)
    assert (count, lost, step0, partial) == (4, 2, 2, 0) and rows[:, 0].tolist() == [2, 3, 4, 5]
    rp.clock(0, 0)                                                       # a reset: the readers roll at once
    assert rp.held(0)[1] == 0 and rp.held(0, "previous")[1:] == (4, 2, 2, 0)
    rp.visit(0, 0, row(0)); rp.clock(0, 1)
    assert rp.held(0, "previous")[1:] == (3, 3, 3, 0) and rp.held(0)[1:] == (1, 0, 0, 0)
    rp.clock(0, 5)                                                       # a restore moved the clock: partial, the fragment becomes a gap
    assert rp.held(0)[1:] == (0, 0, 5, 1) and rp.rolled(0)["gap"] == 1
    rp.visit(0, 5, row(5)); rp.clock(0, 6)
    prof, imb, ofi, info = rp.reductions(0, "current", 4, 1, (1,), 1, 4, (0,), 1, (1,))
    assert info == [1, 0, 5, 1] and prof[0][0] == 1 and imb[1][0] == 1 and ofi[1].tolist() == [0, 0, 6, 0]      # partial: every bar up to step 5's is excluded
    assert D.roll is Q.roll and D.record is Q.record and D.span is Q.span       # taken from quotes.py, not copied


# ---- 7. the library's host check and the header ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip_lib():
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib()


def _arr(v):
    return (C.c_int32 * max(1, len(v)))(*v)


def _check(L, kind, levels=10, lags=(1,), a=1, b=1, depths=(1,)):
    return L.cda_depth_check_host(kind, levels, _arr(lags), len(lags), a, b, _arr(depths), len(depths))


def test_the_host_check_at_each_bound_and_one_beyond(hip_lib):
    L, P, I, O = hip_lib, D.PROFILE, D.IMBALANCE, D.OFI
    for kind in (P, I, O):
        assert _check(L, kind, levels=1) == OK and _check(L, kind, levels=16, b=64) == OK
        assert _check(L, kind, levels=0) == INVALID and _check(L, kind, levels=17) == INVALID
    assert _check(L, 3) == INVALID and _check(L, -1) == INVALID
    # the profile: max_dist in 1 .. 256; nothing else is read
    assert _check(L, P, a=1) == OK and _check(L, P, a=256) == OK and _check(L, P, a=0) == INVALID and _check(L, P, a=257) == INVALID
    assert L.cda_depth_check_host(P, 10, None, 0, 32, 0, None, 0) == OK
    # the imbalance: 1 .. 8 lags in 1 .. 2^20, k in 1 .. levels, half in 1 .. 64
    assert _check(L, I, lags=(1,) * 8, a=10, b=64) == OK and _check(L, I, lags=(1 << 20,)) == OK
    assert _check(L, I, lags=()) == INVALID and _check(L, I, lags=(1,) * 9) == INVALID and _check(L, I, lags=(0,)) == INVALID
    assert _check(L, I, lags=((1 << 20) + 1,)) == INVALID and L.cda_depth_check_host(I, 10, None, 1, 1, 1, None, 0) == INVALID
    assert _check(L, I, a=0) == INVALID and _check(L, I, a=11) == INVALID and _check(L, I, levels=3, a=3) == OK and _check(L, I, levels=3, a=4) == INVALID
    assert _check(L, I, b=0) == INVALID and _check(L, I, b=65) == INVALID and _check(L, I, b=1) == OK
    # the OFI: lags >= 0, bar_steps >= 1, at most 4096 bar points, 1 .. 4 depths in 1 .. levels
    assert _check(L, O, lags=(0, 1), a=1, b=4096) == OK and _check(L, O, a=1, b=4097) == INVALID
    assert _check(L, O, a=2, b=8192) == OK and _check(L, O, a=2, b=8193) == INVALID and _check(L, O, a=0, b=64) == INVALID and _check(L, O, a=1, b=0) == INVALID
    assert _check(L, O, lags=(-1,), b=64) == INVALID and _check(L, O, lags=(1,) * 9, b=64) == INVALID and _check(L, O, lags=((1 << 20) + 1,), b=64) == INVALID
    assert _check(L, O, b=64, depths=(1, 2, 5, 10)) == OK and _check(L, O, b=64, depths=(1,) * 5) == INVALID and _check(L, O, b=64, depths=()) == INVALID
    assert _check(L, O, b=64, depths=(0,)) == INVALID and _check(L, O, b=64, depths=(11,)) == INVALID and _check(L, O, levels=16, b=64, depths=(16,)) == OK
    assert L.cda_depth_check_host(O, 10, _arr((0,)), 1, 1, 64, None, 1) == INVALID
    # the entry points themselves: without an env nothing is launched
    one, lags = C.c_void_p(64), _arr((1, 2))
    assert L.cda_depth_enable(None, 16, 4) == INVALID and L.cda_depth_disable(None) == INVALID and L.cda_depth_capacity(None) == 0 and L.cda_depth_levels(None) == 0
    assert L.cda_depth_meta(None, 0, 1, one, None) == INVALID and L.cda_depth_series(None, 0, 1, 0, 4, one, None, None, None) == INVALID
    assert L.cda_depth_profile(None, 0, 1, 0, 8, one, one, one, None, None) == INVALID
    assert L.cda_depth_imbalance(None, 0, 1, 0, lags, 2, 1, 4, one, one, None, None) == INVALID
    assert L.cda_depth_ofi(None, 0, 1, 0, lags, 2, 1, _arr((1,)), 1, one, one, None, None) == INVALID


def test_constants_field_tuples_and_entry_points_are_the_header_s():
    hdr = open(os.path.join(ROOT, "include", "cda.h")).read()
    for name, value in (("CDA_DEPTH_MAX_LEVELS", D.MAX_LEVELS), ("CDA_DEPTH_MAX_DIST", D.MAX_DIST), ("CDA_DEPTH_MAX_DEPTHS", D.MAX_DEPTHS), ("CDA_DEPTH_BID", D.BID),
                        ("CDA_DEPTH_ASK", D.ASK), ("CDA_DEPTH_SATURATED", D.SATURATED), ("CDA_DEPTH_BID_MORE", D.BID_MORE), ("CDA_DEPTH_ASK_MORE", D.ASK_MORE),
                        ("CDA_DEPTH_PROFILE", D.PROFILE), ("CDA_DEPTH_IMBALANCE", D.IMBALANCE), ("CDA_DEPTH_OFI", D.OFI)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), hdr), name
    assert (len(D.PROFILE_FIELDS), len(D.LEVEL_FIELDS), len(D.IMBALANCE_FIELDS), len(D.RESPONSE_FIELDS), len(D.OFI_FIELDS), len(D.OFI_LAG_FIELDS)) == (8, 3, 4, 5, 4, 6)
    from gym_continuousdoubleauction_amd import _lib
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|int32_t|int64_t) %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS
    inc = open(os.path.join(ROOT, "gym_continuousdoubleauction_amd", "csrc", "cda_hip.hip")).read()
    assert inc.index('#include "cda_quotes.inc"') < inc.index('#include "cda_depth.inc"')


def test_the_entry_points_are_exported(hip_lib):
    for name in ENTRY_POINTS:
        assert hasattr(hip_lib, name), name
