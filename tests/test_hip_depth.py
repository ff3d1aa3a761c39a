"""GPU: the depth tape (include/cda.h cda_depth_*; CDAVecEnv.enable_depth / depth_series / depth_profile / depth_imbalance / depth_ofi).  The ground truth of a
recorded ladder is the CPU oracle replayed beside the env - its book ahead of each step through depth.record_from_orders, fed to tests/depth_replay.py, which
applies the episode rule; where a test steps eagerly without an oracle, env.book_levels(levels + 1) called ahead of each step is the witness.  The reductions are
held to their numpy specifications (depth.profile_from_records, imbalance_from_records, ofi_from_records - which tests/test_depth_host.py pins to hand-worked
answers) on what the ring holds.  Integers only: every comparison is exact.  The oracle's run of a case is computed once and shared."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle_lib as O
from depth_replay import DepthReplay
from test_hip_tape import _actions

pytestmark = pytest.mark.gpu

MAX_STEP = 48                                                    # a horizon short enough that episodes end inside a run
STEPS = MAX_STEP + 22
# n, a, tile, levels, ring
CASES = {"24x4-256-L10": (24, 4, 256, 10, 64), "8x16-512-L3": (8, 16, 512, 3, 64), "8x16-256-L16": (8, 16, 256, 16, 64), "8x4-256-L10-ring20": (8, 4, 256, 10, 20)}
SERIES_CASES = [c for c in CASES if "ring" not in c]
MAX_DIST, LAGS, HALF, OFI_LAGS, BAR = 4, (1, 3), 4, (0, 1, 4), 3


def _np(t):
    return t.cpu().numpy()


def _cfg(a, cap=0, max_step=MAX_STEP, **kw):
    return dict({"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "book_capacity": cap}, **kw)


def _params(L):
    """the reductions' parameters of a case: (k, depths)"""
    return min(L, 5), sorted({1, min(3, L), L})


def _done_set(e, market, a):
    s = e.get_state(market)
    s.done_mask = (1 << a) - 1
    e.set_state(market, s)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The oracle's run of a case, once: the actions, the observations behind every step and the replay of the recorder (a copy of it at every step count in
    `marks`).  At step 10 market 3's episode is declared over (no record, the step ends it): it runs out of step with the batch from there on."""
    from gym_continuousdoubleauction_amd import depth as D
    n, a, cap, L, ring = CASES[case]
    cfg = _cfg(a, cap)
    ora = O.OracleEnv(cfg, n)
    seeds = np.arange(800, 800 + n, dtype=np.uint64)
    out = {"obs0": ora.reset(seeds).copy(), "seeds": seeds, "acts": [], "obs": [], "marks": {}}
    rp, rng = DepthReplay(n, ring, L), np.random.default_rng(5)
    for t in range(STEPS):
        if t == 10:
            _done_set(ora, 3, a)
        for m in range(n):
            s = ora.get_state(m)
            if not (bin(s.done_mask).count("1") == a or s.t_step >= MAX_STEP):
                rp.visit(m, s.t_step, D.record_from_orders(s.t_step, *ora.get_book(m), L))
        acts = _actions(rng, n, a)
        oo, _, ot, otr, _ = ora.step(*acts)
        done = ((ot != 0) | (otr != 0)).astype(np.uint8)
        oo = oo.copy()
        if done.any():
            oo[done == 1] = ora.reset(None, done)[done == 1]
        for m in range(n):
            rp.clock(m, ora.get_state(m).t_step)
        out["acts"].append(acts); out["obs"].append(oo)
        if t + 1 in (30, MAX_STEP, STEPS):
            out["marks"][t + 1] = copy.deepcopy(rp)
    ora.close()
    return out


def check(env, rp, tag, first=0):
    """depth_meta, depth_series and the three reductions of both remembered episodes against the replay; -> records seen"""
    from gym_continuousdoubleauction_amd import depth as D
    L, n = rp.levels, env.n_markets
    k, depths = _params(L)
    seen = 0
    meta = _np(env.depth_meta())
    for m in range(n):
        assert D.meta_from_words(meta[m]) == rp.rolled(m), (tag, m)
    for which in ("current", "previous"):
        rec, cnt, info = (_np(x) for x in env.depth_series(episode=which))
        pb, pl, ps, pinfo = (_np(x) for x in env.depth_profile(MAX_DIST, episode=which))
        ir, ib, iinfo = (_np(x) for x in env.depth_imbalance(LAGS, k, HALF, episode=which))
        ol, ob, oinfo = (_np(x) for x in env.depth_ofi(OFI_LAGS, BAR, depths, episode=which))
        assert rec.dtype == np.int32 and rec.shape[0] == n and rec.shape[2] == 4 * (1 + L) and pl.shape == (n, 2, L, 3) and ps.shape == (n, 2, MAX_DIST + 1)
        assert ir.shape == (n, len(LAGS), 2 * HALF, 5) and ol.shape == (n, len(depths), len(OFI_LAGS), 6) and pb.dtype == ir.dtype == ol.dtype == np.int64
        for m in range(n):
            want, count, lost, step0, partial = rp.held(m, which)
            c = int(cnt[m])
            assert c == count, (tag, which, m, c, count)
            assert np.array_equal(rec[m, :c], want), (tag, which, m, np.argwhere(rec[m, :c] != want)[:4])
            assert not rec[m, c:].any(), (tag, which, m)
            row = [count, lost, step0, partial]
            prof, imb, ofi, _ = rp.reductions(m, which, MAX_DIST, 1, LAGS, k, HALF, OFI_LAGS, BAR, depths)
            for i in (info, pinfo, iinfo, oinfo):
                assert i[m].tolist() == row, (tag, which, m, i[m], row)
            for got, spec, what in ((pb, prof[0], "profile base"), (pl, prof[1], "profile levels"), (ps, prof[2], "shape"), (ir, imb[0], "response"),
                                    (ib, imb[1], "imbalance base"), (ol, ofi[0], "ofi lagged"), (ob, ofi[1], "ofi base")):
                assert np.array_equal(got[m], spec), (tag, which, m, what, got[m].reshape(-1)[:12], spec.reshape(-1)[:12])
            seen += c
    return seen


def _run_case(case, with_info, marks=None):
    from hip_env import HipEnv
    n, a, cap, L, ring = CASES[case]
    ref = reference(case)
    hip = HipEnv(_cfg(a, cap, auto_reset=True), n, with_info=with_info)
    env = hip.env
    env.enable_depth(ring, L)
    assert env.book_capacity == cap and env.depth_enabled and env.depth_capacity == ring and env.depth_levels == L
    assert np.array_equal(hip.reset(ref["seeds"]).view(np.uint32), ref["obs0"].view(np.uint32))
    seen = {}
    for t in range(STEPS):
        if t == 10:
            _done_set(hip, 3, a)
        ho = hip.step(*ref["acts"][t])[0]
        assert np.array_equal(ho.view(np.uint32), ref["obs"][t].view(np.uint32)), t
        if t + 1 in ref["marks"] and (marks is None or t + 1 in marks):
            seen[t + 1] = check(env, ref["marks"][t + 1], f"{case} after {t + 1} steps")
    assert (_np(env.check_invariants()) == 0).all()
    return hip, ref, seen


# ---- 1. the series and the reductions, across the in-kernel auto reset -----------------------------------------------------------------------------
@pytest.mark.parametrize("with_info", [True, False], ids=["info", "noinfo"])
@pytest.mark.parametrize("case", SERIES_CASES)
def test_series_and_reductions_of_both_episodes_equal_the_oracle_s_book_ahead_of_every_step(case, with_info):
    n = CASES[case][0]
    hip, ref, seen = _run_case(case, with_info)
    # after MAX_STEP steps, right behind the step that ended the episodes and before any recorder saw the reset: the readers' own roll decides
    assert seen[30] >= 30 * (n - 1) and seen[MAX_STEP] >= MAX_STEP * (n - 1) and seen[STEPS] >= CASES[case][4] * (n - 1)      # (the ring of 64 has lost the previous episode's first records by then)
    rp = ref["marks"][MAX_STEP]
    assert sum(rp.rolled(m)["n_episode"] == 0 and rp.rolled(m)["n_prev"] == MAX_STEP for m in range(n)) >= n - 1
    hip.close()


def _coverage(case):
    """what the oracle's run of a case shows, from the reference alone"""
    from gym_continuousdoubleauction_amd import depth as D
    n, a, cap, L, ring = CASES[case]
    rp = reference(case)["marks"][STEPS]
    k, depths = _params(L)
    got = dict(more=False, shallow=False, appears=False, vanishes=False, bins=0, ends=False)
    resp = np.zeros((2 * HALF,), np.int64)
    for m in range(n):
        r = np.array(rp.records[m], np.int64).reshape(-1, 1 + L, 4)
        head = r[:, 0]
        got["more"] |= bool((head[:, 1] & (D.BID_MORE | D.ASK_MORE)).any())
        got["shallow"] |= bool((((head[:, 1] & 3) == 3) & ((head[:, 2] < L) | (head[:, 3] < L))).any())
        pair = head[1:, 0] == head[:-1, 0] + 1                       # consecutive steps of one episode
        for sd in (2, 3):
            got["appears"] |= bool((pair & (head[1:, sd] > head[:-1, sd])).any())
            got["vanishes"] |= bool((pair & (head[1:, sd] < head[:-1, sd])).any())
        rows = rp.held(m, "previous")[0]
        resp += D.imbalance_from_records(rows, L, LAGS, k, HALF)[0][0, :, 0]
        shape = D.profile_from_records(rows, L, MAX_DIST)[2]
        got["ends"] |= bool(((shape[:, 0] > 0) & (shape[:, MAX_DIST] > 0)).any())
    got["bins"] = int((resp > 0).sum())
    return got


def test_the_reference_runs_cover_what_the_kernels_can_get_wrong():
    cov = [_coverage(c) for c in SERIES_CASES]
    assert any(c["more"] for c in cov), "no record carries a more flag"
    assert any(c["shallow"] for c in cov), "no two-sided record holds fewer than `levels` levels"
    assert any(c["appears"] for c in cov) and any(c["vanishes"] for c in cov), "no OFI term from an appearing / a vanishing level"
    assert any(c["bins"] >= 4 for c in cov), "fewer than four imbalance bins at the smallest lag"
    assert any(c["ends"] for c in cov), "no market fills both end bins of the shape"


# ---- 2. beside the quote tape ---------------------------------------------------------------------------------------------------------------------
def test_level_0_is_the_quote_record_and_the_quotes_do_not_change():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a, L = 8, 4, 5
    both, alone = (CDAVecEnv(_cfg(a, auto_reset=True), n, with_info=False) for _ in range(2))
    both.enable_quotes(64); both.enable_depth(64, L); alone.enable_quotes(64)
    for env in (both, alone):
        env.reset(seed=41)
    for t in range(MAX_STEP + 9):
        acts = both.random_actions(t, action_seed=6)
        both.step(*acts); alone.step(*acts)
    for which in ("current", "previous"):
        q, qc, qi = (_np(x) for x in both.quote_series(episode=which))
        for got, want in zip((q, qc, qi), alone.quote_series(episode=which)):
            assert np.array_equal(got, _np(want)), which
        d, dc, di = (_np(x) for x in both.depth_series(episode=which))
        assert np.array_equal(dc, qc) and np.array_equal(di, qi) and dc.min() > 0
        d = d.reshape(n, -1, 1 + L, 4)
        assert np.array_equal(d[:, :, 0, 0], q[:, :, 0]) and np.array_equal(d[:, :, 0, 1] & 7, q[:, :, 1])            # step; sides and the saturated bit
        assert np.array_equal(d[:, :, 1, [0, 2, 1, 3]], q[:, :, 2:6])                                                 # prices and volumes of level 0
        assert ((q[:, :, 1] & 3) == 3).any()
    both.close(); alone.close()


# ---- 3. a ring shorter than the episode --------------------------------------------------------------------------------------------------------------
def test_a_ring_shorter_than_the_episode_reports_span_loss_and_excluded_bars():
    case = "8x4-256-L10-ring20"
    n, a, cap, L, ring = CASES[case]
    hip, ref, seen = _run_case(case, False)
    env, rp = hip.env, ref["marks"][STEPS]
    # a later, shallower book reuses a slot: the whole record is written, zero rows included, so the equality above has seen no stale row
    shallower = 0
    for m in range(n):
        r = np.array(rp.records[m], np.int64).reshape(-1, 1 + L, 4)
        shallower += int(((r[ring:, 0, 2] < r[:-ring, 0, 2]) | (r[ring:, 0, 3] < r[:-ring, 0, 3])).sum())
    assert shallower > 0
    rec, cnt, info = (_np(x) for x in env.depth_series(episode="current"))
    live = [m for m in range(n) if m != 3]
    assert rec.shape[1] == ring and cnt[live].tolist() == [ring] * len(live) and info[live, 1].tolist() == [STEPS - MAX_STEP - ring] * len(live)
    _, cnt, info = (_np(x) for x in env.depth_series(episode="previous"))
    assert not cnt[live].any() and info[live, 1].tolist() == [MAX_STEP] * len(live) and not info[:, 3].any()      # the ring holds nothing of it any more
    ofi = _np(env.depth_ofi(OFI_LAGS, BAR, (1, L))[1])
    assert (ofi[live, 2] == (STEPS - MAX_STEP - ring) // BAR + 1).all() and (ofi[live, 1] > 0).all()                 # the bars up to the first held step's are excluded
    rec, cnt, _ = (_np(x) for x in env.depth_series(4, first_market=5, n_markets=2))                                # the last k of what is held; a sub-range
    assert rec.shape == (2, 4, 4 * (1 + L)) and cnt.tolist() == [4, 4] and np.array_equal(rec[1], rp.held(6)[0][-4:])
    hip.close()


# ---- 4. a hand-built book: levels that straddle a pass and the tile-to-ring seam -----------------------------------------------------------------------
def _deep_bids(env, market, agents, rows):
    """`rows` = (price, qty, owner) resting bids in queue order, many per price - more than limit orders could put there (an owner rests once per price), so through
    the state dump, as fuzz_cases.prefill_book does -, no asks, the traders' escrow set to match"""
    from decimal import Decimal

    from gym_continuousdoubleauction_amd import _capi as K
    s = env.get_state(market)
    hold = [0] * agents
    for k, (price, q, owner) in enumerate(rows):
        o = s.bids[k]
        o.price, o.qty, o.owner, o.order_id, o.timestamp = price, q, owner, k + 1, k + 1
        hold[owner] += price * q
    s.n_bids, s.n_asks = len(rows), 0
    s.lob_time = s.next_order_id = len(rows)
    for j in range(agents):
        cash = K.dec_to_decimal(s.acc[j].cash)
        s.acc[j].cash_on_hold = K.decimal_to_dec(Decimal(hold[j]) * Decimal("1.0"))
        s.acc[j].cash = K.decimal_to_dec(cash - Decimal(hold[j]) * Decimal("1.0"))
    env.set_state(market, s)


@pytest.mark.parametrize("cap", [256, 512])
def test_deep_levels_are_followed_through_the_passes_and_into_the_ring(cap):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd import depth as D
    a, L = 4, 3
    tick = 5
    env = CDAVecEnv(_cfg(a, cap), 3, with_info=False, market_configs=[{"tick_size": tick}] * 3)
    env.reset(seed=3)
    sizes = (70, 200, 5)                                            # orders per level: the second level straddles passes 1 .. 4 and, on the 256 tile, the seam
    rows, k = [], 0
    for lv, cnt in enumerate(sizes):
        for _ in range(cnt):
            rows.append(((60 - lv) * tick, 1 + k % 5, k % a, k + 1, k + 1)); k += 1
    bids = np.array(rows, np.int32)
    none = np.zeros((0, 5), np.int32)
    six = np.array([((70 + 2 * j) * tick, 2 + j, j % a, j + 1, j + 1) for j in range(6)], np.int32)       # more levels than `levels` on one side, none on the other
    _deep_bids(env, 0, a, [tuple(r[:3]) for r in bids.tolist()])
    assert _np(env.seed_books(none, six, market=1)[1])[0].tolist()[:3] == [len(six), 0, 0]
    env.enable_depth(8, L)
    b, s = env.get_book(0)
    assert len(b) == sum(sizes) and len(s) == 0 and np.array_equal(b[:, :3], bids[:, :3])
    if cap == 256:
        assert len(b) > cap and env.book_spill > 0                   # the tile cannot hold the side: it continues in the HBM ring
    vol = [int(bids[bids[:, 0] == (60 - lv) * tick, 1].sum()) for lv in range(3)]
    want = [D.record_from_orders(0, *env.get_book(m), L) for m in range(3)]
    assert want[0].tolist() == [0, D.BID, 3, 0, 300, vol[0], 0, 0, 295, vol[1], 0, 0, 290, vol[2], 0, 0]
    assert want[1].tolist() == [0, D.ASK | D.ASK_MORE, 0, 3, 0, 0, 350, 2, 0, 0, 360, 3, 0, 0, 370, 4] and want[2].tolist() == [0] * 16
    env.step(*env.random_actions(0, action_seed=2))
    rec, cnt, _ = (_np(x) for x in env.depth_series())
    assert cnt.tolist() == [1, 1, 1]
    for m in range(3):
        assert rec[m, 0].tolist() == want[m].tolist(), (m, rec[m, 0], want[m])
    base, lev, shape, _ = (_np(x) for x in env.depth_profile(3))      # distances in ticks of the market's own row: 0, 1, 2 on the bids; 0, 2, 4 on the asks (4 clips to 3)
    for m in range(3):
        for got, spec in zip((base, lev, shape), D.profile_from_records(rec[m, :1], L, 3, tick)):
            assert np.array_equal(got[m], spec), (m, got[m], spec)
    assert shape[0, 0].tolist() == [vol[0], vol[1], vol[2], 0] and shape[1, 1].tolist() == [2, 0, 3, 4] and lev[1, 1, :, 2].tolist() == [0, 2, 4]
    env.enable_depth(8, 2)                                           # fewer levels than the side has: the walk stops inside the second level's successor
    w2 = D.record_from_orders(1, *env.get_book(0), 2)
    env.step(*env.random_actions(1, action_seed=2))
    rec = _np(env.depth_series()[0])
    assert rec[0, 0].tolist() == w2.tolist() and rec[0, 0, 1] & D.BID_MORE
    assert (_np(env.check_invariants()) == 0).all()
    env.close()


# ---- 5. every entry point records; the refusals ---------------------------------------------------------------------------------------------------------
def _witness(env, t_steps):
    """every market's record of the coming step from book_levels(levels + 1)"""
    from gym_continuousdoubleauction_amd import depth as D
    L = env.depth_levels
    lv = _np(env.book_levels(L + 1))
    return [D.record_from_levels(t_steps[m], lv[m, 0], lv[m, 1], L) for m in range(env.n_markets)]


def _eager(env, steps, do_step, markets=None):
    want = []
    for t in range(steps):
        want.append(_witness(env, [t] * env.n_markets))
        do_step(t)
    rec, cnt, _ = (_np(x) for x in env.depth_series())
    for m in (range(env.n_markets) if markets is None else markets):
        assert cnt[m] == steps and np.array_equal(rec[m, :steps], np.array([w[m] for w in want])), m
    return rec, cnt


def test_step_range_records_its_range_only():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd._lib import check as ok, lib
    n, a = 24, 4
    env = CDAVecEnv(_cfg(a), n, with_info=False)
    env.reset(seed=7)
    env.enable_depth(32, 4)
    st = torch.cuda.current_stream().cuda_stream

    def ranged(t):
        cat, mean, sigma, price, off = (x[0] for x in env.random_actions_device(t, 1, action_seed=3))
        ok(lib().cda_step_range(env._h, 8, 8, cat.data_ptr(), mean.data_ptr(), sigma.data_ptr(), price.data_ptr(), off.data_ptr(), None,
                                env.obs.data_ptr(), env.reward.data_ptr(), env._term.data_ptr(), env._trunc.data_ptr(), None, st), "cda_step_range")
        torch.cuda.synchronize()
    rec, cnt = _eager(env, 5, ranged, markets=range(8, 16))
    outside = [m for m in range(n) if not 8 <= m < 16]
    assert not cnt[outside].any() and not rec[outside].any() and not _np(env.depth_meta())[outside].any()
    assert (_np(env.depth_meta())[8:16, [0, 2]] == 5).all()
    env.close()


def test_group_launches_and_run_scripted_record():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a = 24, 4
    env = CDAVecEnv(_cfg(a), n, with_info=False, groups=2)
    env.reset(seed=8)
    env.enable_depth(32, 4)
    rng = np.random.default_rng(9)

    def grouped(t):
        env.step(*_actions(rng, n, a), pipelined=True)
        env.sync()
    _eager(env, 6, grouped)
    env.close()
    env = CDAVecEnv(_cfg(a), n, with_info=False)
    env.reset(seed=8)
    slots = np.zeros((n, a), np.int32)
    slots[:, 0], slots[:, 1] = 1, 2
    env.set_scripted(slots, ["maker", "taker"], seed=9)
    env.enable_depth(32, 4)
    rec, _ = _eager(env, 8, lambda t: env.run_scripted(1, others="random", action_seed=3))
    assert ((rec[:, :8, 1] & 3) == 3).any()
    env.close()


def test_the_recorder_runs_behind_the_schedule_and_every_refusal():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd import _capi as K
    from gym_continuousdoubleauction_amd import depth as D
    from gym_continuousdoubleauction_amd import orders as OR
    from gym_continuousdoubleauction_amd._lib import CDAError, lib
    n, a, max_step, Lv = 6, 4, 8, 2
    env = CDAVecEnv(_cfg(a, max_step=max_step), n, with_info=False)
    L = lib()
    assert L.cda_policy_step_supported(env._h) == 1
    env.reset(seed=11)
    bids = np.array([[50, 3, 0, 1, 1], [50, 4, 1, 2, 2], [48, 9, 2, 3, 3], [47, 1, 2, 4, 4]], np.int32)
    asks = np.array([[55, 2, 2, 5, 5], [56, 1, 3, 6, 6]], np.int32)
    env.set_order_schedule(OR.schedule_with_seed(bids, asks, [[[] for _ in range(max_step - 1)]]), market_schedule=[0] * (n - 1) + [-1])
    with pytest.raises(RuntimeError, match="enable_depth"):
        env.depth_series()
    env.enable_depth(16, Lv)
    assert L.cda_policy_step_supported(env._h) == 0
    assert all(len(s) == 0 for s in env.get_book(0))            # the book is empty until the step's own schedule launch seeds it
    env.step(*_actions(np.random.default_rng(1), n, a))
    rec, cnt, _ = (_np(x) for x in env.depth_series())
    seed = D.record_from_orders(0, bids, asks, Lv)
    assert seed.tolist() == [0, D.BID | D.ASK | D.BID_MORE, 2, 2, 50, 7, 55, 2, 48, 9, 56, 1] and cnt.tolist() == [1] * n
    for m in range(n - 1):
        assert np.array_equal(rec[m, 0], seed), (m, rec[m, 0])  # the step-0 ladder shows the seed: the recorder runs behind the schedule
    assert rec[n - 1, 0].tolist() == [0] * 12
    env.clear_order_schedule()
    assert L.cda_policy_step_supported(env._h) == 0             # still off: depth is on
    with pytest.raises(CDAError, match="cda_run_random"):
        env.run_random(4)
    # the C-level refusals: nothing is launched behind any
    out = torch.zeros(4096, dtype=torch.int64, device=env.device)
    info = torch.zeros((n, 4), dtype=torch.int32, device=env.device)
    p, ip, st = out.data_ptr(), info.data_ptr(), torch.cuda.current_stream().cuda_stream
    arr = lambda *v: (C.c_int32 * max(1, len(v)))(*v)           # noqa: E731
    assert L.cda_depth_series(env._h, 0, n, 0, 4, p, None, ip, st) == K.OK and L.cda_depth_profile(env._h, 0, n, 0, 8, p, p + 1024, p + 2048, ip, st) == K.OK
    assert L.cda_depth_imbalance(env._h, 0, n, 0, arr(1, 2), 2, Lv, 4, p, p + 8192, ip, st) == K.OK
    assert L.cda_depth_ofi(env._h, 0, n, 0, arr(0, 1), 2, 1, arr(1, 2), 2, p, p + 8192, ip, st) == K.OK
    for bad in ((0, n + 1), (-1, 2), (0, 0), (n, 1)):
        assert L.cda_depth_meta(env._h, *bad, p, st) == K.ERR_INVALID and L.cda_depth_series(env._h, *bad, 0, 4, p, None, ip, st) == K.ERR_INVALID
        assert L.cda_depth_profile(env._h, *bad, 0, 8, p, p + 1024, p + 2048, ip, st) == K.ERR_INVALID
        assert L.cda_depth_imbalance(env._h, *bad, 0, arr(1), 1, 1, 4, p, p + 8192, ip, st) == K.ERR_INVALID
        assert L.cda_depth_ofi(env._h, *bad, 0, arr(0), 1, 1, arr(1), 1, p, p + 8192, ip, st) == K.ERR_INVALID
    assert L.cda_depth_meta(env._h, 0, n, None, st) == K.ERR_INVALID and L.cda_depth_meta(env._h, 0, n, p + 2, st) == K.ERR_INVALID
    for bad in ((2, 4, p, None, ip), (0, 0, p, None, ip), (0, 4, None, None, ip), (0, 4, p + 8, None, ip), (0, 4, p, p + 2, ip), (0, 4, p, None, ip + 2)):
        assert L.cda_depth_series(env._h, 0, n, *bad, st) == K.ERR_INVALID, bad[:2]
    for bad in ((2, 8, p, p, p, ip), (0, 0, p, p, p, ip), (0, 257, p, p, p, ip), (0, 8, None, p, p, ip), (0, 8, p, None, p, ip), (0, 8, p, p, None, ip),
                (0, 8, p + 4, p, p, ip), (0, 8, p, p + 4, p, ip), (0, 8, p, p, p + 4, ip), (0, 8, p, p, p, ip + 2)):
        assert L.cda_depth_profile(env._h, 0, n, *bad, st) == K.ERR_INVALID, bad[:2]
    for bad in ((2, arr(1), 1, 1, 4, p, p, ip), (0, None, 1, 1, 4, p, p, ip), (0, arr(1), 0, 1, 4, p, p, ip), (0, arr(*[1] * 9), 9, 1, 4, p, p, ip), (0, arr(0), 1, 1, 4, p, p, ip),
                (0, arr(1), 1, 0, 4, p, p, ip), (0, arr(1), 1, Lv + 1, 4, p, p, ip), (0, arr(1), 1, 1, 0, p, p, ip), (0, arr(1), 1, 1, 65, p, p, ip),
                (0, arr(1), 1, 1, 4, None, p, ip), (0, arr(1), 1, 1, 4, p, None, ip), (0, arr(1), 1, 1, 4, p + 4, p, ip), (0, arr(1), 1, 1, 4, p, p + 4, ip)):
        assert L.cda_depth_imbalance(env._h, 0, n, *bad, st) == K.ERR_INVALID, bad[:5]
    for bad in ((2, arr(0), 1, 1, arr(1), 1, p, p, ip), (0, None, 1, 1, arr(1), 1, p, p, ip), (0, arr(-1), 1, 1, arr(1), 1, p, p, ip), (0, arr(0), 1, 0, arr(1), 1, p, p, ip),
                (0, arr(0), 1, 1, None, 1, p, p, ip), (0, arr(0), 1, 1, arr(1), 0, p, p, ip), (0, arr(0), 1, 1, arr(1, 1, 1, 1, 1), 5, p, p, ip),
                (0, arr(0), 1, 1, arr(0), 1, p, p, ip), (0, arr(0), 1, 1, arr(Lv + 1), 1, p, p, ip), (0, arr(0), 1, 1, arr(1), 1, None, p, ip),
                (0, arr(0), 1, 1, arr(1), 1, p, None, ip), (0, arr(0), 1, 1, arr(1), 1, p + 4, p, ip), (0, arr(0), 1, 1, arr(1), 1, p, p, ip + 2)):
        assert L.cda_depth_ofi(env._h, 0, n, *bad, st) == K.ERR_INVALID, bad[:6]
    for cap_, lv in ((0, 4), ((1 << 20) + 1, 4), (16, 0), (16, 17)):
        assert L.cda_depth_enable(env._h, cap_, lv) == K.ERR_INVALID
    assert env.depth_capacity == 16 and env.depth_levels == Lv      # a refused enable leaves the env as it was
    env.disable_depth()
    assert L.cda_depth_meta(env._h, 0, n, p, st) == K.ERR_UNSUPPORTED and L.cda_depth_series(env._h, 0, n, 0, 4, p, None, ip, st) == K.ERR_UNSUPPORTED
    assert L.cda_depth_profile(env._h, 0, n, 0, 8, p, p, p, ip, st) == K.ERR_UNSUPPORTED
    assert L.cda_depth_imbalance(env._h, 0, n, 0, arr(1), 1, 1, 4, p, p, ip, st) == K.ERR_UNSUPPORTED
    assert L.cda_depth_ofi(env._h, 0, n, 0, arr(0), 1, 1, arr(1), 1, p, p, ip, st) == K.ERR_UNSUPPORTED
    assert env.depth_capacity == 0 and env.depth_levels == 0 and L.cda_policy_step_supported(env._h) == 1
    torch.cuda.synchronize()
    env.run_random(4)
    env.close()


# ---- 6. rollouts: episodes end inside the graphs -----------------------------------------------------------------------------------------------------------
def test_rollout_chains_record_across_the_in_kernel_auto_reset_and_refuse_a_toggle():
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd import depth as D
    from gym_continuousdoubleauction_amd._lib import lib
    N, A, T, max_step, L = 32, 4, 48, 20, 6
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": max_step, "is_render": False}
    env = CDAVecEnv(dict(cfg, auto_reset=True), n_markets=N, with_info=False)
    env.reset(seed=300)
    env.enable_depth(64, L)
    assert lib().cda_policy_step_supported(env._h) == 0
    roll = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=1), T, groups=2, seed=5)
    b = {k: _np(v).copy() for k, v in roll.run().items()}
    torch.cuda.synchronize()
    assert roll.graphs is not None
    ora = O.OracleEnv(cfg, N)
    assert np.array_equal(ora.reset(np.arange(300, 300 + N, dtype=np.uint64)).view(np.uint32), b["obs"][0].view(np.uint32))
    rp = DepthReplay(N, 64, L)
    for t in range(T):
        for m in range(N):
            ts = ora.get_state(m).t_step
            rp.visit(m, ts, D.record_from_orders(ts, *ora.get_book(m), L))
        oo, orw, ot, otr, _ = ora.step(*(b[k][t] for k in ("category", "size_mean", "size_sigma", "price", "price_offset")))
        assert np.array_equal(b["reward"][t].view(np.uint64), orw.view(np.uint64)), t
        done = ((ot != 0) | (otr != 0)).astype(np.uint8)
        if done.any():
            ora.reset(None, done)
        for m in range(N):
            rp.clock(m, ora.get_state(m).t_step)
    ora.close()
    assert all(rp.rolled(m)["n_episode"] == T - 2 * max_step and rp.rolled(m)["n_prev"] == max_step for m in range(N))      # two episodes ended inside the graphs
    assert check(env, rp, "rollout") == N * (T - max_step)
    env.disable_depth()
    with pytest.raises(RuntimeError, match="depth tape"):
        roll.run()
    env.enable_depth(64, L)
    with pytest.raises(RuntimeError, match="depth tape"):
        roll.run()
    env.close()


# ---- 7. restores move the clock -----------------------------------------------------------------------------------------------------------------------------
def test_a_restore_restarts_the_current_episode_partial_and_keeps_the_previous():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a, L = 8, 4, 4
    env = CDAVecEnv(_cfg(a, max_step=64), n, with_info=False)
    env.reset(seed=31)
    env.enable_depth(128, L)
    rp = DepthReplay(n, 128, L)
    clock = [0] * n

    def run(t0, t1):
        for t in range(t0, t1):
            for m, w in enumerate(_witness(env, clock)):
                rp.visit(m, clock[m], w)
            env.step(*env.random_actions(t, action_seed=5))
            for m in range(n):
                clock[m] += 1
                rp.clock(m, clock[m])

    def moved(markets, t_step):
        for m in markets:
            clock[m] = t_step
            rp.clock(m, t_step)
    run(0, 12)
    env.reset(seed=32)                                         # a finished episode to remember
    moved(range(n), 0)
    run(0, 10)
    early = env.snapshot(2, 2)                                 # markets 2, 3 at step 10
    run(10, 30)
    env.restore(early, first=2)                                # 30 -> 10
    moved((2, 3), 10)
    check(env, rp, "restored, before a record")                # the readers roll at once: empty, partial, starting at step 10; the previous episode is kept
    assert rp.held(2)[1:] == (0, 0, 10, 1) and rp.held(2, "previous")[1:] == (12, 0, 0, 0) and rp.rolled(2)["gap"] == 30
    run(30, 33)
    late = env.snapshot(6, 2)                                  # markets 6, 7 at step 33
    check(env, rp, "three records behind the restore")
    assert rp.held(2)[1:] == (3, 0, 10, 1) and rp.held(5)[1:] == (33, 0, 0, 0)
    env.restore(late, first=2)                                 # the reverse: 13 -> 33
    moved((2, 3), 33)
    run(33, 35)
    check(env, rp, "forward restore")
    assert rp.held(2)[1:] == (2, 0, 33, 1) and rp.rolled(2)["gap"] == 33 and rp.held(2, "previous")[1] == 12
    env.close()


# ---- 8. the recorder writes nothing but its own buffers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_info", [True, False], ids=["info", "noinfo"])
def test_a_twin_stepped_without_depth_is_byte_identical(with_info):
    from hip_env import HipEnv
    n, a, steps = 24, 4, 40
    cfg = _cfg(a, max_step=24, auto_reset=True)
    on, off = HipEnv(cfg, n, with_info=with_info), HipEnv(cfg, n, with_info=with_info)
    on.env.enable_depth(16, 10)
    on.env.enable_tape(256); off.env.enable_tape(256)
    seeds = np.arange(500, 500 + n, dtype=np.uint64)
    assert np.array_equal(on.reset(seeds).view(np.uint32), off.reset(seeds).view(np.uint32))
    rng = np.random.default_rng(77)
    for t in range(steps):
        acts = _actions(rng, n, a)
        r0, r1 = off.step(*acts), on.step(*acts)
        assert np.array_equal(r0[0].view(np.uint32), r1[0].view(np.uint32)) and np.array_equal(r0[1].view(np.uint64), r1[1].view(np.uint64)), t
    for i in range(n):
        assert bytes(on.get_state(i)) == bytes(off.get_state(i)), i
    assert torch.equal(on.env.drain_tape()[0], off.env.drain_tape()[0])
    assert (_np(on.env.check_invariants()) == 0).all() and (on.flags() == off.flags()).all()
    assert int(_np(on.env.depth_meta())[:, 0].sum()) == n * steps
    on.close(); off.close()


# ---- 9. the evaluation loop -------------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_saves_the_ladders_and_reports_the_book_shape(tmp_path):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd import depth as D
    from gym_continuousdoubleauction_amd import evaluate as EV
    N, A, E, max_step, L = 32, 4, 2, 24, 6
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    pol = mlp.FusedPolicy("cuda:0", seed=5)
    path = str(tmp_path / "depth.npz")
    keep = {}
    res = EV.evaluate(env, pol, opponents=["random", "maker"], trained_slots=1, episodes=E, seed=3, depth=path, depth_levels=L, book_shape_report=True, bar_steps=2, keep=keep)
    plain = EV.evaluate(env, pol, opponents=["random", "maker"], trained_slots=1, episodes=E, seed=3)
    assert res["summary"] == plain["summary"] and "depth" not in plain and not env.depth_enabled      # the recorder changed nothing, and the env's setting is back
    z = D.load(path)
    assert z["records"].shape == (N, max_step, 4 * (1 + L)) and int(z["levels"]) == L and z["counts"].tolist() == [max_step] * N
    assert (z["records"][:, :, 0] == np.arange(max_step)).all() and list(z["module_names"]) == list(res["modules"]) and not z["info"][:, [1, 3]].any()
    # the same actions replayed by plain steps on an env with depth on: the same ladders, and the report's rows are the per-market specifications, summed
    other = CDAVecEnv(cfg, n_markets=N, with_info=False)
    other.enable_depth(2 * max_step, L)
    other.reset(seed=(np.uint64(3) * np.uint64(N) + np.arange(N, dtype=np.uint64)))
    acts = {k: v.numpy() for k, v in keep["actions"].items()}
    for step in range(E * max_step):
        other.step(acts["category"][step], acts["size_mean"][step], acts["size_sigma"][step], acts["price"][step], acts["price_offset"][step])
    rec, cnt, _ = (_np(x) for x in other.depth_series(max_step, episode="previous"))
    other.close()
    assert np.array_equal(rec, z["records"]) and np.array_equal(cnt, z["counts"])
    about, rows = res["depth"]["about"], res["depth"]["rows"]
    depths = sorted({1, 5, L})
    assert about["levels"] == L and about["markets"] == N and about["records"] == N * max_step and about["records_lost"] == 0 and about["depths"] == depths and about["bar_steps"] == 2
    prof = [D.profile_from_records(rec[m], L, EV.BOOK_SHAPE_MAX_DIST) for m in range(N)]
    imb = [D.imbalance_from_records(rec[m], L, EV.BOOK_SHAPE_LAGS, L, EV.BOOK_SHAPE_HALF) for m in range(N)]
    ofi = [D.ofi_from_records(rec[m], L, EV.BOOK_SHAPE_OFI_LAGS, 2, depths) for m in range(N)]
    for key, tables, j in (("profile", prof, 0), ("levels", prof, 1), ("shape", prof, 2), ("response", imb, 0), ("imbalance", imb, 1), ("ofi_lagged", ofi, 0), ("ofi", ofi, 1)):
        assert np.array_equal(np.array(rows[key], np.int64), sum(t[j] for t in tables)), key
    assert rows["profile"][1] > 0 and set(res["depth"]) >= {"profile", "imbalance", "ofi", "about", "rows"} and set(res["depth"]["ofi"]["regression"]) == {"K1", "K5", "K6"}
    with pytest.raises(ValueError, match="levels"):
        EV.evaluate(env, pol, episodes=1, depth=path, depth_levels=17)
    env.close()
