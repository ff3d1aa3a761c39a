"""CPU: the stateful opponents' laws (include/cda_stateful_agents.h) against their specification (gym_continuousdoubleauction_amd/stateful.py): hand-written
sequences of views with the action, the state words and the branch at every step; cda_stateful_advance_host against the specification on random (profile, view,
state) triples that sit on every edge; the update rule; the profile's bounds; the GPU test's own closed-loop case played on the CPU oracle with the specification
choosing the actions (the coverage conditions are asserted here); the kernel's resources.  No GPU."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import stateful_util as U
from gym_continuousdoubleauction_amd import scripted as S
from gym_continuousdoubleauction_amd import stateful as F
from gym_continuousdoubleauction_amd.stateful import Profile

ERR_INVALID = -1
K16 = 1 << 16
SEED, COUNTER, MARKET, AGENT = 7, 2, 11, 3
ORDER = (0.25, 0.125)
TREND = Profile(law=F.LAW_TREND, size_mean=0.25, size_sigma=0.125, max_position=2, fast_shift=0, slow_shift=1, band_ticks=1, direction=1, warmup=1)
VALUE = Profile(law=F.LAW_VALUE, size_mean=0.25, size_sigma=0.125, max_position=1, band_ticks=1, p_move_q32=1 << 32)
EXEC = Profile(law=F.LAW_EXECUTION, size_mean=0.25, size_sigma=0.125, target=10, start_step=2, duration=4, patience=1)
EXEC_SELL = dataclasses.replace(EXEC, target=-10, start_step=0)


def view(**kw):
    v = np.zeros((), S.VIEW_DTYPE)
    for k, x in kw.items():
        v[k] = x
    return v


def header(profile_index, t):
    return ((profile_index + 1) << 32) | t


def _draws(up, n=4):
    """draw numbers whose value draw (SEED, COUNTER, MARKET, draw, AGENT) has bit 32 clear (V moves up) / set (down)"""
    return [d for d in range(200) if ((F.value_draw(SEED, COUNTER, MARKET, d, AGENT) >> 32) & 1 == 0) == up][:n]


UP, DOWN = _draws(True), _draws(False)
PASS_ = (0, 0.0, 0.0, 0, 1)
# per law: the profile, its index in the attached list (the tag is 1 + that), and the steps (view, draw, the intended action, the intended words 1 .. 3, the branch)
SEQUENCES = {
    # tick 1, band 1 tick of the mid = 2 units of x = 2 << 16; the slow EMA halves the distance, the fast one (shift 0) is x << 16 itself
    "trend": (TREND, 2, [
        (view(t_step=0, tick=1, best_ask=101), 0, PASS_, (0, 0, 0), "trend_warmup"),                                   # unquoted: nothing is seen
        (view(t_step=1, tick=1, best_bid=100, best_ask=102), 0, PASS_, (202 * K16, 202 * K16, 1), "trend_warmup"),       # the first observation sets both; count 1 = warmup
        (view(t_step=2, tick=1, best_bid=102, best_ask=104), 0, PASS_, (206 * K16, 204 * K16, 2), "trend_flat"),         # exactly at the band
        (view(t_step=3, tick=1, best_bid=104, best_ask=105, net_position=1), 0, (1, *ORDER, 0, 1), (209 * K16, 206 * K16 + K16 // 2, 3), "trend_buy"),
        (view(t_step=3, tick=1, best_bid=1, best_ask=2, net_position=2), 0, PASS_, (209 * K16, 206 * K16 + K16 // 2, 3), "trend_buy_capped"),      # the same step again: no update
        (view(t_step=5, tick=1, best_bid=100, best_ask=101, net_position=-2), 0, PASS_, (201 * K16, 203 * K16 + 3 * K16 // 4, 4), "trend_sell_capped"),   # a gap: one update
        (view(t_step=6, tick=1, best_bid=100, net_position=-1), 0, (5, *ORDER, 0, 1), (201 * K16, 203 * K16 + 3 * K16 // 4, 4), "trend_sell"),      # unquoted: the EMAs stand
    ]),
    # tick 5: V moves by 10, the band is 10
    "value": (VALUE, 0, [
        (view(t_step=0, tick=5), 0, PASS_, (0, 0, 0), "value_uninitialised"),
        (view(t_step=1, tick=5, best_bid=100, best_ask=110), 0, PASS_, (210, 1, 0), "value_hold"),                       # V = x, no draw at the initialising step
        (view(t_step=2, tick=5, best_bid=100, best_ask=105), UP[0], PASS_, (220, 1, 0), "value_hold"),                   # 2 ask = V - band exactly
        (view(t_step=3, tick=5, best_bid=100, best_ask=105), UP[1], (1, *ORDER, 0, 1), (230, 1, 0), "value_buy"),
        (view(t_step=3, tick=5, best_bid=100, best_ask=105, net_position=1), DOWN[0], PASS_, (230, 1, 0), "value_buy_capped"),      # the same step again: no draw
        (view(t_step=4, tick=5, best_bid=120, best_ask=125, net_position=-1), DOWN[1], PASS_, (220, 1, 0), "value_sell_capped"),
        (view(t_step=5, tick=5, best_bid=120), DOWN[2], (5, *ORDER, 0, 1), (210, 1, 0), "value_sell"),                   # unquoted, initialised: V still walks, the bid is dear
    ]),
    # due(t) = 10 * clamp(t - 2, 0, 4) / 4 = 0, 2, 5, 7, 10 at t = 2 .. 6
    "execution": (EXEC, 1, [
        (view(t_step=0), 0, PASS_, (0, 0, 0), "exec_waiting"),
        (view(t_step=2), 0, PASS_, (0, 0, 0), "exec_ahead"),
        (view(t_step=3), 0, (2, *ORDER, 0, 1), (1, 0, 0), "exec_passive_limit"),
        (view(t_step=4), 0, (1, *ORDER, 0, 1), (2, 0, 0), "exec_market"),                                               # behind for longer than patience
        (view(t_step=5, net_position=7), 0, PASS_, (0, 0, 0), "exec_ahead"),
        (view(t_step=6, net_position=7, own_orders=(2, 0)), 0, (3, *ORDER, 0, 1), (1, 0, 0), "exec_passive_modify"),
        (view(t_step=7, net_position=10), 0, PASS_, (0, 0, 0), "exec_done"),
        (view(t_step=8, net_position=12), 0, PASS_, (0, 0, 0), "exec_done"),                                            # overshot: it never reverses
    ]),
    # a sell order: due(1) = -10 / 4 truncates to -2 (a floor would say -3 and call the slot behind)
    "execution_sell": (EXEC_SELL, 4, [
        (view(t_step=0), 0, PASS_, (0, 0, 0), "exec_ahead"),
        (view(t_step=1, net_position=-2), 0, PASS_, (0, 0, 0), "exec_ahead"),
        (view(t_step=2, net_position=-2, own_orders=(3, 0)), 0, (6, *ORDER, 0, 1), (1, 0, 0), "exec_passive_limit"),    # (its bids do not count: the acquiring side is the ask)
        (view(t_step=3, net_position=-2), 0, (5, *ORDER, 0, 1), (2, 0, 0), "exec_market"),
    ]),
}


def test_hand_written_sequences():
    seen = set()
    for name, (prof, pidx, steps) in SEQUENCES.items():
        state = [0, 0, 0, 0]
        views, draws, states_in = [], [], []
        for k, (v, draw, want, words, branch) in enumerate(steps):
            act, new, why = F.advance(prof, v, state, (SEED, COUNTER, MARKET, draw, AGENT), pidx)
            got = (act[0], float(act[1]), float(act[2]), act[3], act[4])
            assert why == branch and got == tuple(want), (name, k, why, got)
            assert new == [header(pidx, int(v["t_step"])), *words], (name, k, new)
            views.append(v); draws.append(draw); states_in.append(state)
            state = new
            seen.add(why)
        # ... and the C functions say the same, step by step from the same states
        profiles = [prof] * (pidx + 1)
        rc, got, st = U.advance_host(profiles, pidx, np.array(views), np.array(states_in), SEED, COUNTER, MARKET, np.array(draws), AGENT)
        assert rc == 0
        for k, (v, _d, want, words, _b) in enumerate(steps):
            assert (int(got[0][k]), float(got[1][k]), float(got[2][k]), int(got[3][k]), int(got[4][k])) == tuple(want), (name, k)
            assert st[k].tolist() == [header(pidx, int(v["t_step"])), *words], (name, k)
    assert seen == set(F.BRANCHES), sorted(set(F.BRANCHES) - seen)


EDGES = [  # profile, state in (tag 1, last_t 4), view at t_step 5, draw, the intended words 1 .. 3
    # a negative EMA distance floors: -3 >> 1 = -2 (truncation would say -1); +3 >> 1 = 1
    (dataclasses.replace(TREND, fast_shift=1, slow_shift=2), [200 * K16 + 3, 200 * K16 - 3, 9], view(t_step=5, tick=1, best_bid=100, best_ask=100), 0,
     (200 * K16 + 1, 200 * K16 - 3 + 0, 10)),
    (dataclasses.replace(TREND, fast_shift=1, slow_shift=2), [200 * K16 - 3, 200 * K16 + 5, 9], view(t_step=5, tick=1, best_bid=100, best_ask=100), 0,
     (200 * K16 - 2, 200 * K16 + 3, 10)),
    # V never goes below 2 ticks of x
    (VALUE, [10, 1, 0], view(t_step=5, tick=5), DOWN[0], (10, 1, 0)),
    (VALUE, [15, 1, 0], view(t_step=5, tick=5), DOWN[0], (10, 1, 0)),
    (VALUE, [15, 1, 0], view(t_step=5, tick=5), UP[0], (25, 1, 0)),
    (dataclasses.replace(VALUE, p_move_q32=0), [15, 1, 0], view(t_step=5, tick=5), UP[0], (15, 1, 0)),
]


def test_hand_written_edges():
    for k, (prof, words_in, v, draw, words) in enumerate(EDGES):
        state = [header(0, 4), *words_in]
        _act, new, _why = F.advance(prof, v, state, (SEED, COUNTER, MARKET, draw, AGENT), 0)
        assert new == [header(0, 5), *words], (k, new)
        rc, _got, st = U.advance_host([prof], 0, np.array([v]), np.array([state]), SEED, COUNTER, MARKET, draw, AGENT)
        assert rc == 0 and st[0].tolist() == new, (k, st[0].tolist())


# ---------------------------------------------------------------------------------------------------------------- random triples on the laws' edges
LAW_PROFILES = {
    "trend": [TREND, dataclasses.replace(TREND, fast_shift=2, slow_shift=5, band_ticks=0, direction=-1, warmup=0, max_position=0),
              dataclasses.replace(TREND, fast_shift=3, slow_shift=12, band_ticks=3, warmup=7, max_position=9),
              dataclasses.replace(TREND, fast_shift=0, slow_shift=4, band_ticks=F.MAX_BAND, direction=-1, warmup=2, max_position=5)],
    "value": [dataclasses.replace(VALUE, p_move_q32=p, max_position=c, band_ticks=b) for p in (0, 1, 1 << 31, (1 << 32) - 1, 1 << 32) for c, b in ((0, 0), (3, 1), (7, 4))],
    "execution": [EXEC, EXEC_SELL, dataclasses.replace(EXEC, target=-7, start_step=5, duration=3, patience=0), dataclasses.replace(EXEC, target=1000, start_step=0, duration=7, patience=4),
                  dataclasses.replace(EXEC, target=-(2 ** 31), start_step=1, duration=2 ** 31 - 1, patience=2), dataclasses.replace(EXEC, target=3, start_step=10, duration=1, patience=1)],
}


def random_triples(rng, law, n, profiles, pix):
    """(views, states) on the laws' edges: the signal at the band and one beyond it, the position at the cap and one beyond it, the count at warmup and one above
    it, steps behind at patience and one above it, t at start_step and at start_step + duration, empty sides, ticks 1 / 5 / 7, odd EMA distances of both signs,
    V at its floor - and headers that are fresh (t_step 0, no tag, another profile's tag), repeated (last_t == t_step) or one or several steps old"""
    get = lambda k: np.array([getattr(p, k) for p in profiles], np.int64)[pix]      # noqa: E731
    v = np.zeros(n, S.VIEW_DTYPE)
    tick = rng.choice([1, 5, 7], n)
    v["tick"] = tick
    t = np.where(rng.integers(0, 10, n) == 0, 0, rng.integers(1, 300, n))
    if law == "execution":
        start, dur = get("start_step"), get("duration")
        how = rng.integers(0, 8, n)
        t = np.select([how == 0, how == 1, how == 2, how == 3, how == 4], [start, start + np.minimum(dur, 1000), np.maximum(start - 1, 0), start + 1, start + np.minimum(dur, 1000) - 1], t)
    v["t_step"] = t
    bid = tick * rng.integers(1, 60, n)
    ask = bid + tick * rng.integers(1, 9, n)
    empty = rng.integers(0, 8, n)
    bid = np.where((empty == 0) | (empty == 2), 0, bid)
    ask = np.where((empty == 1) | (empty == 2), 0, ask)
    v["best_bid"], v["best_ask"] = bid, ask
    v["own_orders"] = rng.integers(0, 3, (n, 2))
    cap = get("max_position")
    pick = rng.integers(0, 8, n)
    pos = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4], [cap, cap + 1, -cap, -cap - 1, cap - 1], rng.integers(-40, 41, n))
    # the header: mostly this profile's tag and the step before; sometimes the same step, an older one, no tag, another tag
    hk = rng.integers(0, 10, n)
    tag = np.select([hk == 0, hk == 1], [0, (pix + 1) % len(profiles) + 1], pix + 1)
    last = np.select([hk == 2, hk == 3, hk == 4], [t, t, np.maximum(t - 5, 0)], np.maximum(t - 1, 0))
    st = np.zeros((n, 4), np.int64)
    st[:, 0] = (tag.astype(np.int64) << 32) | (last.astype(np.int64) & 0xffffffff)
    same = (tag == pix + 1) & (last == t) & (t != 0)                     # no update: the decision reads the state as it came in
    x = (bid + ask).astype(np.int64)
    if law == "trend":
        warm, band, dirn = get("warmup"), get("band_ticks"), get("direction")
        thr = (2 * band * tick) << 16
        slow = (x << 16) + rng.integers(-9, 10, n) + np.where(rng.integers(0, 3, n) == 0, rng.integers(-(1 << 24), 1 << 24, n), 0)
        sig = np.select([rng.integers(0, 2, n) == 0], [thr + rng.integers(-1, 2, n)], -thr + rng.integers(-1, 2, n))      # at the band, one inside, one beyond - both signs
        fast = np.where(rng.integers(0, 4, n) == 0, (x << 16) + rng.integers(-9, 10, n), slow + dirn * sig)
        cnt = np.select([rng.integers(0, 3, n) == 0], [rng.integers(0, 20, n)], warm + rng.integers(-1, 2, n))
        st[:, 1], st[:, 2], st[:, 3] = fast, slow, np.maximum(cnt, 0)
        st[(st[:, 3] == 0) & (rng.integers(0, 2, n) == 0), 1:3] = 0
    elif law == "value":
        band = 2 * get("band_ticks") * tick
        how = rng.integers(0, 6, n)
        near = rng.integers(-1, 2, n) + 2 * tick * rng.integers(-1, 2, n)      # the touch test at, one inside and one beyond - before and after a move of 2 ticks
        V = np.select([how == 0, how == 1, how == 2, how == 3], [2 * ask + band + near, 2 * bid - band + near, 2 * tick, 2 * tick + rng.integers(0, 2 * 7 + 1, n)], x + rng.integers(-30, 31, n))
        init = rng.integers(0, 6, n) != 0
        st[:, 1], st[:, 2] = np.where(init, np.maximum(V, 2 * tick), 0), init
    else:
        pat, target = get("patience"), get("target")
        st[:, 1] = np.maximum(pat + rng.integers(-2, 2, n), 0)             # + 1 by the update: patience - 1 .. patience + 2
        st[same, 1] = np.maximum(pat[same] + rng.integers(-1, 2, int(same.sum())), 0)
        el = np.clip(t - start, 0, dur)
        due = np.array([int(a) * int(b) for a, b in zip(target, el)], object)
        due = np.array([abs(int(d)) // int(q) * (1 if d >= 0 else -1) for d, q in zip(due, dur)], np.int64)
        how = rng.integers(0, 6, n)
        pos = np.select([how == 0, how == 1, how == 2], [due + rng.integers(-1, 2, n), target + rng.integers(-1, 2, n), 0], pos)
        pos = np.clip(pos, -(2 ** 31), 2 ** 31 - 1)
    v["net_position"] = pos
    return v, st


@pytest.mark.parametrize("law", sorted(LAW_PROFILES))
def test_advance_host_equals_the_specification(law):
    n = 20000
    rng = np.random.default_rng(F.LAWS[law])
    profiles = LAW_PROFILES[law]
    assert all(p.problems() == [] for p in profiles)
    pix = rng.integers(0, len(profiles), n)
    views, states = random_triples(rng, law, n, profiles, pix)
    market, draw, agent = rng.integers(0, 1 << 40, n), rng.integers(0, 1 << 31, n), rng.integers(0, 16, n)
    seed, counter = 0xfedcba9876543210, 12345
    tally = {}
    want, want_state = F.play(profiles, pix, views, states, seed, counter, market, draw, agent, branches=tally)
    rc, got, got_state = U.advance_host(profiles, pix, views, states, seed, counter, market, draw, agent)
    assert rc == 0 and U.same_actions(got, want), [np.flatnonzero(g != w)[:4] for g, w in zip(got, want)]
    assert np.array_equal(got_state, want_state), np.argwhere(got_state != want_state)[:4]
    assert (got_state != states).any(axis=1).mean() > 0.5 and (got_state == states).all(axis=1).any()      # most items advance, some are the same step again
    prefix = {"trend": "trend", "value": "value", "execution": "exec"}[law]
    need = {b for b in F.BRANCHES if b.startswith(prefix)}
    assert set(tally) == need, (sorted(need - set(tally)), sorted(set(tally) - need))      # every branch of the law fired, and no other name
    if law == "trend":                                                   # an EMA distance whose floor is not its truncation was among them
        upd = (got_state[:, 0] != states[:, 0]) & (states[:, 3] > 0) & (views["best_bid"] != 0) & (views["best_ask"] != 0) & ((states[:, 0] >> 32) == pix + 1) & (views["t_step"] != 0)
        y = (views["best_bid"].astype(np.int64) + views["best_ask"]) << 16
        sh = np.array([p.slow_shift for p in profiles])[pix]
        d = y - states[:, 2]
        assert (upd & (d < 0) & (d % (1 << sh) != 0)).sum() > 100
    if law == "value":
        assert (got_state[:, 1][states[:, 2] != 0] == 2 * views["tick"][states[:, 2] != 0]).sum() > 100      # V at its floor


# ---------------------------------------------------------------------------------------------------------------- the update rule
def _both(prof, pidx, v, state, draw=0, n_profiles=6):
    """specification and host function on one item; they must agree; returns (action tuple, new state list)"""
    act, new, _why = F.advance(prof, v, state, (SEED, COUNTER, MARKET, draw, AGENT), pidx)
    rc, got, st = U.advance_host([prof] * n_profiles, pidx, np.array([v]), np.array([state]), SEED, COUNTER, MARKET, draw, AGENT)
    assert rc == 0 and st[0].tolist() == new and int(got[0][0]) == act[0] and np.float32(got[1][0]) == act[1]
    return act, new


@pytest.mark.parametrize("law", ["trend", "value", "execution"])
def test_the_update_rule(law):
    prof, pidx, steps = SEQUENCES[law]
    quoted = view(t_step=9, tick=5, best_bid=100, best_ask=110, net_position=0)
    moved = view(t_step=9, tick=5, best_bid=300, best_ask=310, net_position=0)
    state = [header(pidx, 7), 215 * K16 if law == "trend" else (210 if law == "value" else 3), 205 * K16 if law == "trend" else (1 if law == "value" else 0), 5 if law == "trend" else 0]
    a1, s1 = _both(prof, pidx, quoted, state, draw=UP[0])
    assert s1 != state and s1[0] == header(pidx, 9)                      # a gap in t_step (7 -> 9): one update
    once = list(state)
    once[0] = header(pidx, 8)
    assert _both(prof, pidx, quoted, once, draw=UP[0])[1] == s1          # ... the same one as from the step before: no catching up
    # twice at one t_step: nothing changes, whatever the book and the draw say now
    a2, s2 = _both(prof, pidx, moved if law != "execution" else quoted, s1, draw=DOWN[0])
    assert s2 == s1
    assert _both(prof, pidx, quoted, s1, draw=DOWN[1])[0] == a1
    # t_step == 0 re-initialises whatever the state held
    zero = view(t_step=0, tick=5, best_bid=100, best_ask=110)
    _a, s0 = _both(prof, pidx, zero, s1, draw=UP[0])
    assert s0 == _both(prof, pidx, zero, [0, 0, 0, 0], draw=UP[0])[1] and s0[0] == header(pidx, 0)
    assert s0[1:] == {"trend": [210 * K16, 210 * K16, 1], "value": [210, 1, 0], "execution": [0, 0, 0]}[law]
    # a changed tag re-initialises mid-episode; so does no tag
    other = list(s1)
    other[0] = header(pidx + 1, 8)
    _a, sn = _both(prof, pidx, quoted, other, draw=UP[0])
    assert sn == _both(prof, pidx, quoted, [0, 0, 0, 0], draw=UP[0])[1] == _both(prof, pidx, quoted, [8, 77, 77, 77], draw=UP[0])[1] and sn[0] == header(pidx, 9)


def test_value_draws_are_their_own():
    """equal keys: the value law's draw differs from the taker's and from the label tap's mix draw, in the whole word and in the low 32 bits the laws test"""
    rng = np.random.default_rng(3)
    for _ in range(2000):
        key = (int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 31)), int(rng.integers(0, 16)))
        w, wt, wm = F.value_draw(*key), S.taker_draw(*key), S.mix_draw(*key)
        assert len({w, wt, wm}) == 3 and len({w & 0xffffffff, wt & 0xffffffff, wm & 0xffffffff}) == 3
    # ... and the C function draws what value_draw says: a walk of V over 64 steps, every step a move
    prof = dataclasses.replace(VALUE, p_move_q32=1 << 32)
    state, want, ups = [header(0, 0), 1000, 1, 0], 1000, 0
    for t in range(1, 65):
        _a, state = _both(prof, 0, view(t_step=t, tick=1), state, draw=t, n_profiles=1)
        up = (F.value_draw(SEED, COUNTER, MARKET, t, AGENT) >> 32) & 1 == 0
        want, ups = (want + 2 if up else max(want - 2, 2)), ups + up
        assert state[1] == want
    assert 16 <= ups <= 48                                               # both directions, about evenly (a fair coin leaves this band once in 10^4 walks)


# ---------------------------------------------------------------------------------------------------------------- the profile's bounds
BOUNDS = [  # field, values that are valid, values one step outside
    ("law", (1, 3), (0, 4)),
    ("size_mean", (-1.0, 1.0), (np.nextafter(np.float32(-1), np.float32(-2)), np.nextafter(np.float32(1), np.float32(2)), float("nan"))),
    ("size_sigma", (0.0, 1.0), (-np.nextafter(np.float32(0), np.float32(1)), np.nextafter(np.float32(1), np.float32(2)), float("nan"))),
    ("max_position", (0, 2 ** 31 - 1), (-1,)),
    ("fast_shift", (0, 4), (-1, 5)),                                     # (the base profile's slow_shift is 5)
    ("slow_shift", (3, 12), (2, 13)),                                    # (... and its fast_shift 2)
    ("band_ticks", (0, F.MAX_BAND), (-1, F.MAX_BAND + 1)),
    ("direction", (-1, 1), (0, 2, -2)),
    ("warmup", (0, 2 ** 31 - 1), (-1,)),
    ("p_move_q32", (0, 1 << 32), ((1 << 32) + 1,)),
    ("target", (-(2 ** 31), -1, 1, 2 ** 31 - 1), (0,)),
    ("start_step", (0, 2 ** 31 - 1), (-1,)),
    ("duration", (1, 2 ** 31 - 1), (0, -1)),
    ("patience", (0, 2 ** 31 - 1), (-1,)),
]


def test_profile_validation():
    from gym_continuousdoubleauction_amd._lib import lib
    base = Profile(law=F.LAW_VALUE, size_mean=0.5, size_sigma=0.5, max_position=10, fast_shift=2, slow_shift=5, band_ticks=3, direction=1, warmup=4, patience=2,
                   p_move_q32=5, target=7, start_step=3, duration=9)

    def c_valid(p):
        pa = F.profiles_array([p], validate=False)
        return lib().cda_stateful_profile_check_host(pa.ctypes.data, 1)

    assert base.problems() == [] and c_valid(base) == 0
    for field, good, bad in BOUNDS:
        for x in good:
            p = dataclasses.replace(base, **{field: x})
            assert p.problems() == [] and c_valid(p) == 0, (field, x)
        for x in bad:
            p = dataclasses.replace(base, **{field: x})
            assert p.problems() != [] and c_valid(p) == ERR_INVALID, (field, x)
            with pytest.raises(ValueError):
                F.profiles_array([p])
            # an invalid profile is refused by the host entry point, and nothing is written
            rc, got, st = U.advance_host([p], 0, np.zeros(3, S.VIEW_DTYPE), np.full((3, 4), 5), 0, 0, 0, 0, 0)
            assert rc == ERR_INVALID and (got[0] == -7).all() and (st == 5).all()
    assert set(F.NAMED) == {"trend", "value", "execution"}
    for name in F.NAMED:
        assert F.parse_profile(name).problems() == [] and F.parse_profile(name).law == F.LAWS[name] and F.is_stateful_spec(name)
        assert not S.is_scripted_spec(name)
        with pytest.raises(ValueError):
            S.parse_profile(name)                                        # the stateless family's boundary stands
    p = F.parse_profile("execution:target=-40,size_mean=0.5, patience=0x10")
    assert p.target == -40 and p.size_mean == 0.5 and p.patience == 16 and p.law == F.LAW_EXECUTION and p.duration == F.NAMED["execution"].duration
    assert F.is_stateful_spec("trend:warmup=3") and F.is_stateful_spec(p) and not F.is_stateful_spec("maker") and not F.is_stateful_spec(S.NAMED["maker"])
    for bad in ("maker", "momentum", "trend:slow_shift=13", "trend:law=2", "value:nosuch=1", "execution:target", "execution:target=0"):
        with pytest.raises(ValueError):
            F.parse_profile(bad)
    assert F.module_id(1, F.NAMED["value"]) == "stateful_1_value"
    assert F.PROFILE_DTYPE.itemsize == 64 and C.sizeof(C.c_char * F.PROFILE_DTYPE.itemsize) == 64 and F.STATE_WORDS == 4 and F.STATE_DTYPE.itemsize == 8


# ---------------------------------------------------------------------------------------------------------------- the closed loop, on the oracle alone
@pytest.mark.parametrize("n,a", sorted({(n, a) for n, a, _tile in U.SHAPES}))
def test_closed_loop_on_the_oracle_reaches_what_the_gpu_test_needs(n, a):
    """the GPU test's own case (stateful_util: profiles, slot table, seeds, shapes) on the CPU oracle, the specification choosing every slot's action"""
    r = U.oracle_episode(n, a)
    assert U.TRADING <= set(r["tally"]), sorted(U.TRADING - set(r["tally"]))      # every trading branch of every law
    assert set(r["tally"]) <= set(F.BRANCHES) and sum(r["tally"].values()) == U.STEPS * n * a
    assert (r["resets"] >= 2).all(), r["resets"]                        # each market resets itself at least twice
    assert r["unquoted"] > 0                                             # a slot meets an unquoted step
    assert len(set(r["actions"][0].reshape(-1).tolist())) >= 6           # passes, both market orders, limits and modifies among the actions
    hdr = r["states"][..., 0]
    assert np.array_equal(hdr >> 32, np.broadcast_to(U.mixed_slots(n, a), hdr.shape))          # every slot's tag is its profile's
    assert np.array_equal(hdr[:, 0, 0] & 0xffffffff, np.arange(U.STEPS) % U.MAX_STEP)         # ... and last_t follows the episode clock through the resets


# ---------------------------------------------------------------------------------------------------------------- the kernel's resources
def test_the_stateful_kernel_exists_once_and_keeps_everything_in_registers():
    from test_kernel_resources import _kernels
    ks, bodies = _kernels()
    inst = {n: v for n, v in ks.items() if "k_stateful_actions" in n}
    assert len(inst) == 1, sorted(inst)
    (n, v), = inst.items()
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 128, (n, v)
    body = bodies[n]
    assert not any("atomic" in l for l in body), n
    assert not any("scratch_" in l for l in body), n
    assert sum("global_store_dwordx4" in l for l in body) >= 2 and sum("global_load_dwordx4" in l for l in body) >= 2      # the state moves in 16-byte words
    # the name carries none of the stems other tests count kernels by
    assert not any(stem in n for stem in ("k_stepILb", "k_tstepILb", "k_policy_step", "k_tape_", "k_script_actions", "k_script_label", "k_net_step"))
    assert sum("k_script_actions" in k for k in ks) == 1 and sum("k_script_label" in k for k in ks) == 1
