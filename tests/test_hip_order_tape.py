"""GPU: the order tape (include/cda.h cda_order_tape_*, cda_order_flow, cda_order_fills; CDAVecEnv.enable_order_tape / order_tape_series / order_flow /
order_fills).  The ground truth of a record is the CPU oracle replayed beside the env - its Trace of every step (the decoded orders and the execution order) and
its book ahead of the step, through order_tape.record_from_decoded, fed to tests/order_tape_replay.py, which applies the episode rule - and, for the reference
itself, the committed golden traces.  The reductions are held to their numpy specifications (order_tape.flow_from_records, fills_from_records - which
tests/test_order_tape_host.py pins to hand-worked answers) on what the rings hold.  Integers only: every comparison is exact.  The oracle's run of a case is
computed once and shared."""
import copy
import functools

import numpy as np
import pytest
import torch

import golden_util as G
import oracle_lib as O
import schedule_util as SU
from order_tape_replay import OrderReplay, decoded_of, touch_of

pytestmark = pytest.mark.gpu

MAX_STEP = 20                                                    # a horizon short enough that two episodes end inside a run
STEPS = 48
RING, TAPE_CAP = 64, 4096
# n, a, tile, n_hist, tick, the form of `present`
CASES = {"24x4-256-h4-t1-all": (24, 4, 256, 4, 1, "all"), "8x1-256-h1-t7-mask": (8, 1, 256, 1, 7, "mask"), "8x7-512-h16-t7-dict": (8, 7, 512, 16, 7, "dict"),
         "8x16-256-h1-t1-dict": (8, 16, 256, 1, 1, "dict"), "8x16-512-h4-t7-mask": (8, 16, 512, 4, 7, "mask")}
GOLDENS = ("perm_s91", "permshuf8_s94", "subset_s31", "A16_aggr_s71", "edge_price0_s407", "edge_pricetop_tickmax_s408", "bigsize_aggr_s82", "tick7_aggr8_s303",
           "reset_s51")
GOLDEN_STEPS = 64


def _np(t):
    return t.cpu().numpy()


def _cfg(a, cap=0, max_step=MAX_STEP, **kw):
    return dict({"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "book_capacity": cap}, **kw)


def _done_set(e, market, a):
    s = e.get_state(market)
    s.done_mask = (1 << a) - 1
    e.set_state(market, s)


def _touch_state(e, market):
    """a set_state that changes nothing: the device forgets its cached level aggregation, so the next visit walks the book"""
    e.set_state(market, e.get_state(market))


def _over(s, a, max_step=MAX_STEP):
    return bin(s.done_mask).count("1") == a or s.t_step >= max_step


def _present(rng, n, a, form):
    if form == "all":
        return None
    keep = (rng.random((n, a)) < 0.75).astype(np.uint8)
    if form == "mask":
        return keep
    out = np.zeros((n, a), np.uint8)
    for m in range(n):
        out[m] = (1 + rng.permutation(a)) * keep[m]              # 1 + the agent's place in the caller's dict; 0 = not in it
    return out


def _generator(s):
    g = np.random.Generator(np.random.PCG64(0))
    st = g.bit_generator.state
    st["state"] = {"state": (int(s.rng_state_hi) << 64) | int(s.rng_state_lo), "inc": (int(s.rng_inc_hi) << 64) | int(s.rng_inc_lo)}
    st["has_uint32"], st["uinteger"] = int(s.rng_has_uint32), int(s.rng_uinteger)
    g.bit_generator.state = st
    return g


def _needs_redraw(s, n_present):
    """did one of the step's n normals need more than its first 64-bit draw: the generator's state behind the normals against its state behind as many raw draws"""
    a, b = _generator(s), _generator(s)
    a.standard_normal(n_present); b.bit_generator.random_raw(n_present)
    return a.bit_generator.state["state"] != b.bit_generator.state["state"]


def _levels(rows):
    return len(np.unique(rows[:, 0])) if len(rows) else 0


def oracle_record(ora, m, s, books, pres, raw, cover, tick):
    """market m's record of the step the oracle has just taken (state `s` and `books` from ahead of it), and what the step covers"""
    from gym_continuousdoubleauction_amd import order_tape as OT
    a = ora.A
    dec, order = decoded_of(ora.trace[m], a, pres)
    n_pres = a if pres is None else int((np.asarray(pres) != 0).sum())
    cover["zero_orders"] |= len(order) == 0
    cover["all_orders"] |= len(order) == a
    cover["redraw"] |= n_pres > 0 and _needs_redraw(s, n_pres)
    for ag in range(a):
        side, typ, _, price = dec[ag]
        if side < 0:
            continue
        cover["pairs"].add((int(typ), int(side)))
        level = min(max(int(raw[ag][1]), 0), 9)
        if typ != OT.T_MARKET and _levels(books[side]) <= level:
            cover["fallback"] = True
        if typ != OT.T_MARKET and price == tick:
            cover["floor"] = True
    return OT.record_from_decoded(s.t_step, touch_of(*books), dec, order, pres, raw)


def new_cover():
    return dict(zero_orders=False, all_orders=False, redraw=False, fallback=False, floor=False, cache_invalid=False, cache_valid=False, pairs=set())


@functools.lru_cache(maxsize=None)
def reference(case):
    """The oracle's run of a case, once: the actions, the observations behind every step, the step's own lob_actions and the replay of the recorder (a copy of it
    at every step count in `marks`).  At step 10 market 3's episode is declared over (no record, the step ends it); ahead of step 12 market 1 gets a set_state
    that changes nothing (the device's level cache is invalid for that visit)."""
    n, a, cap, hist, tick, form = CASES[case]
    cfg = _cfg(a, cap, n_hist=hist, tick_size=tick)
    ora = O.OracleEnv(cfg, n)
    seeds = np.arange(800, 800 + n, dtype=np.uint64)
    out = {"obs0": ora.reset(seeds).copy(), "seeds": seeds, "acts": [], "present": [], "obs": [], "lob": [], "live": [], "marks": {}, "cover": new_cover()}
    rp, rng = OrderReplay(n, RING, a), np.random.default_rng(5)
    for t in range(STEPS):
        if t == 10:
            _done_set(ora, 3, a)
        if t == 12:
            _touch_state(ora, 1)
        acts, pres = SU.law(rng, n, a), _present(rng, n, a, form)
        if t % 7 == 3:
            acts[0][:] = 0 if t % 2 else np.where(acts[0] == 0, 1, acts[0])        # a step in which everybody passes, one in which nobody does
        pre = [(ora.get_state(m), ora.get_book(m)) for m in range(n)]
        oo, _, ot, otr, info = ora.step(*acts, pres)
        live = np.zeros(n, bool)
        for m, (s, books) in enumerate(pre):
            if _over(s, a):
                continue
            live[m] = True
            raw = np.stack([acts[0][m], acts[3][m], acts[4][m]], axis=1)
            rp.visit(m, s.t_step, oracle_record(ora, m, s, books, None if pres is None else pres[m], raw, out["cover"], tick))
            if t == 12 and m == 1:
                out["cover"]["cache_invalid"] |= len(books[0]) + len(books[1]) > 0
            else:
                out["cover"]["cache_valid"] = True
        done = ((ot != 0) | (otr != 0)).astype(np.uint8)
        oo = oo.copy()
        if done.any():
            oo[done == 1] = ora.reset(None, done)[done == 1]
        for m in range(n):
            rp.clock(m, ora.get_state(m).t_step)
        out["acts"].append(acts); out["present"].append(pres); out["obs"].append(oo); out["lob"].append(info["lob_actions"].copy()); out["live"].append(live)
        if t + 1 in (MAX_STEP, STEPS):
            out["marks"][t + 1] = copy.deepcopy(rp)
    assert (ora.flags() == 0).all()
    ora.close()
    return out


def check(env, rp, tag, tick=1):
    """order_tape_meta, order_tape_series and the two reductions of both remembered episodes against the replay; -> records seen"""
    from gym_continuousdoubleauction_amd import order_tape as OT
    n, a = env.n_markets, env.num_agents
    seen = 0
    meta = _np(env.order_tape_meta())
    for m in range(n):
        assert OT.meta_from_words(meta[m]) == rp.rolled(m), (tag, m)
    for which in ("current", "previous"):
        rec, cnt, info = (_np(x) for x in env.order_tape_series(episode=which))
        flow, finfo = (_np(x) for x in env.order_flow(episode=which))
        assert rec.dtype == np.int32 and rec.shape[0] == n and rec.shape[2] == 4 * (1 + a) and flow.shape == (n, a, 32) and flow.dtype == np.int64
        with_tape = env.tape_enabled
        if with_tape:
            fills, xinfo = (_np(x) for x in env.order_fills(episode=which))
            trows, tcnt = (_np(x) for x in env.tape_last(TAPE_CAP, episode=which))
            assert fills.shape == (n, a, 24) and xinfo.shape == (n, 8)
        for m in range(n):
            want, count, lost, step0, partial = rp.held(m, which)
            c = int(cnt[m])
            assert c == count, (tag, which, m, c, count)
            got = rec[m, :c].reshape(c, 1 + a, 4)
            assert np.array_equal(got, want), (tag, which, m, np.argwhere(got != want)[:4], got[got != want][:4], want[got != want][:4])
            assert not rec[m, c:].any(), (tag, which, m)
            assert info[m].tolist() == [count, lost, step0, partial] == finfo[m].tolist(), (tag, which, m, info[m], finfo[m])
            assert np.array_equal(flow[m], OT.flow_from_records(want, tick)), (tag, which, m)
            if with_tape:
                held = trows[m, :int(tcnt[m])]
                assert np.array_equal(fills[m], OT.fills_from_records(held, want, a)), (tag, which, m)
                assert xinfo[m, :4].tolist() == [count, lost, step0, partial] and xinfo[m, 4] == tcnt[m], (tag, which, m, xinfo[m])
                assert xinfo[m, 6] == (int(held[0, 7]) >> 2 if len(held) else -1), (tag, which, m)
            seen += c
    return seen


def _run_case(case, with_info):
    from gym_continuousdoubleauction_amd import order_tape as OT
    from hip_env import HipEnv
    n, a, cap, hist, tick, form = CASES[case]
    ref = reference(case)
    hip = HipEnv(_cfg(a, cap, n_hist=hist, tick_size=tick, auto_reset=True), n, with_info=with_info)
    env = hip.env
    env.enable_order_tape(RING)
    env.enable_tape(TAPE_CAP)
    assert env.book_capacity == cap and env.order_tape_enabled and env.order_tape_capacity == RING
    assert np.array_equal(hip.reset(ref["seeds"]).view(np.uint32), ref["obs0"].view(np.uint32))
    seen, lob = {}, []
    for t in range(STEPS):
        if t == 10:
            _done_set(hip, 3, a)
        if t == 12:
            _touch_state(hip, 1)
        ho, _, _, _, info = hip.step(*ref["acts"][t], ref["present"][t])
        assert np.array_equal(ho.view(np.uint32), ref["obs"][t].view(np.uint32)), t
        if with_info:
            live = ref["live"][t]
            assert np.array_equal(info["lob_actions"][live], ref["lob"][t][live]), t
            lob.append(info["lob_actions"].copy())
        if t + 1 in ref["marks"]:
            seen[t + 1] = check(env, ref["marks"][t + 1], f"{case} after {t + 1} steps", tick)
    if with_info:                                                # the tape's view of the decoded orders IS the step's own lob_actions tensor
        rec, cnt, inf = (_np(x) for x in env.order_tape_series(episode="current"))
        for m in range(n):
            c, s0 = int(cnt[m]), int(inf[m, 2])
            if m == 3 or c == 0:
                continue
            assert c == STEPS - 2 * MAX_STEP and s0 == 0
            assert np.array_equal(OT.lob_actions(rec[m, :c]), np.stack([lob[2 * MAX_STEP + j][m] for j in range(c)])), m
    assert (_np(env.check_invariants()) == 0).all()
    return hip, ref, seen


# ---- 1. against the oracle: the series and the reductions, across the in-kernel auto reset ------------------------------------------------------------------
@pytest.mark.parametrize("with_info", [True, False], ids=["info", "noinfo"])
@pytest.mark.parametrize("case", list(CASES))
def test_series_and_reductions_of_both_episodes_equal_the_oracle_s_decoded_orders(case, with_info):
    n = CASES[case][0]
    hip, ref, seen = _run_case(case, with_info)
    live = n - (1 if n > 3 else 0)
    # after MAX_STEP steps, right behind the step that ended the episodes and before any recorder saw the reset: the readers' own roll decides
    assert seen[MAX_STEP] >= MAX_STEP * live and seen[STEPS] >= (STEPS - MAX_STEP) * live
    rp = ref["marks"][MAX_STEP]
    assert sum(rp.rolled(m)["n_episode"] == 0 and rp.rolled(m)["n_prev"] == MAX_STEP for m in range(n)) >= live
    hip.close()


# ---- 2. against the reference itself: the committed golden traces ---------------------------------------------------------------------------------------------
def _golden_want(r, steps):
    a = r["cat"].shape[1]
    la = np.full((steps, a, 4), -1, np.int64)
    ex = np.full((steps, a), -1, np.int64)
    for t in range(steps):
        has = r["dec_type"][t] != -9
        has &= r["dec_side"][t] != 2
        la[t][has] = np.stack([r["dec_side"][t], r["dec_type"][t], r["dec_size"][t], r["dec_price"][t]], axis=1)[has]
        k = int(r["n_acts"][t])
        ex[t, :k] = r["exec_order"][t][:k]
    return la, ex


@pytest.mark.parametrize("name", GOLDENS)
def test_the_tape_holds_the_reference_s_decoded_orders_and_execution_order(name):
    from gym_continuousdoubleauction_amd import order_tape as OT
    from hip_env import HipEnv
    r = G.load(name)
    steps = min(GOLDEN_STEPS, r["cat"].shape[0])
    hip = HipEnv(r["config"], n_markets=1)
    hip.env.enable_order_tape(128)
    G.run_group(hip, [r], state_every=0, max_steps=steps)
    la, ex = _golden_want(r, steps)
    parts = []
    for which in ("previous", "current"):
        rec, cnt, info = (_np(x) for x in hip.env.order_tape_series(128, episode=which))
        parts.append(rec[0, :int(cnt[0])])
        assert info[0, 1] == 0                                   # nothing lost to the ring
    got = np.concatenate(parts)
    k = len(got)
    assert k >= 1 and (len(r["resets"]) > 0 or k == steps), (name, k, steps)      # the last two episodes of the replayed steps (a trace with resets may have more)
    assert np.array_equal(OT.lob_actions(got), la[steps - k:]), name
    assert np.array_equal(OT.exec_order(got), ex[steps - k:]), name
    assert not (OT.as_rows(got)[:, 1:, 0] & OT.CLAMPED)[OT.as_rows(got)[:, 1:, 0] >= 0].any() and (hip.flags() == 0).all()
    hip.close()


# ---- 3. coverage, from host data alone ---------------------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_what_the_recorder_can_get_wrong():
    cov = [reference(c)["cover"] for c in CASES]
    pairs = set().union(*(c["pairs"] for c in cov))
    tick_floor = False
    for name in GOLDENS:
        r = G.load(name)
        steps = min(GOLDEN_STEPS, r["cat"].shape[0])
        la, _ = _golden_want(r, steps)
        pairs |= {(int(t), int(s)) for s, t in la[la[:, :, 0] >= 0][:, :2]}
        tick = int(r["config"].get("tick_size", 1))
        lim = (la[:, :, 0] >= 0) & (la[:, :, 1] != 0)
        tick_floor |= bool((la[lim][:, 3] == tick).any())
    assert pairs == {(t, s) for t in range(4) for s in range(2)}, sorted(pairs)
    assert any(c["zero_orders"] for c in cov) and any(c["all_orders"] for c in cov), "no step with 0 orders / with A orders"
    assert any(c["fallback"] for c in cov), "no order priced from last_price because its level is empty"
    assert tick_floor or any(c["floor"] for c in cov), "no price at the one-tick floor"
    assert any(c["cache_invalid"] for c in cov) and all(c["cache_valid"] for c in cov), "the level cache was not seen both valid and invalid"
    assert any(c["redraw"] for c in cov), "no step whose normals needed a ziggurat redraw"


def test_a_clamped_price_sets_bit_8_and_the_step_flags_the_overflow():
    """the oracle does not clamp: device only, the shape of test_hip_domain_flags.test_price_clamp_edge.  (The size clamp cannot be reached: see the table there.)"""
    from gym_continuousdoubleauction_amd import _capi as K
    from gym_continuousdoubleauction_amd import order_tape as OT
    from hip_env import HipEnv
    top = (1 << 24) - 1
    hip = HipEnv(_cfg(4, max_step=100, init_cash=10 ** 12), 2)
    hip.reset(np.arange(7, 9, dtype=np.uint64))
    hip.env.enable_order_tape(8)
    for i in range(2):
        s = hip.get_state(i)
        s.last_price = top - 1                                   # an empty ask side decodes level l as last_price + (l + 1) ticks
        hip.set_state(i, s)
    n, a = 2, 4
    cat, level = np.zeros((n, a), np.int32), np.zeros((n, a), np.int32)
    cat[:, 0] = 6                                                # agent 0: a limit ask
    level[1, 0] = 1                                              # market 0 decodes 2^24 - 1, market 1 2^24
    zeros = np.zeros((n, a), np.float32)
    info = hip.step(cat, zeros, zeros, level, np.ones((n, a), np.int32))[4]
    rec = OT.as_rows(_np(hip.env.order_tape_series(1)[0])[:, 0])
    assert rec[:, 1, 2].tolist() == [top, top] == list(info["lob_actions"][:, 0, 3])
    assert rec[:, 1, 0].tolist() == [OT.T_LIMIT | (OT.S_ASK << 2), OT.T_LIMIT | (OT.S_ASK << 2) | OT.CLAMPED] and rec[:, 1, 3].tolist() == [6 | (1 << 8), 6 | (1 << 4) | (1 << 8)]
    assert list(hip.flags()) == [0, K.FLAG_INT_OVERFLOW] and rec[:, 0].tolist() == [[0, 1 << 8 | 3 << 16, 0, 0]] * 2
    hip.close()


# ---- 4. the recorder writes nothing but its own buffers, and consumes no draw -------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_info", [True, False], ids=["info", "noinfo"])
def test_a_twin_stepped_without_the_tape_is_byte_identical_after_every_step(with_info):
    from hip_env import HipEnv
    n, a, steps = 24, 4, 30
    cfg = _cfg(a, auto_reset=True)
    on, off = HipEnv(cfg, n, with_info=with_info), HipEnv(cfg, n, with_info=with_info)
    on.env.enable_order_tape(16)
    on.env.enable_tape(256); off.env.enable_tape(256)
    seeds = np.arange(500, 500 + n, dtype=np.uint64)
    assert np.array_equal(on.reset(seeds).view(np.uint32), off.reset(seeds).view(np.uint32))
    rng = np.random.default_rng(77)
    for t in range(steps):
        acts = SU.law(rng, n, a)
        r0, r1 = off.step(*acts), on.step(*acts)
        assert np.array_equal(r0[0].view(np.uint32), r1[0].view(np.uint32)) and np.array_equal(r0[1].view(np.uint64), r1[1].view(np.uint64)), t
        assert np.array_equal(r0[2], r1[2]) and np.array_equal(r0[3], r1[3]), t
        for i in range(n):
            assert bytes(on.get_state(i)) == bytes(off.get_state(i)), (t, i)      # the whole dump, the generator's words included: the recorder drew nothing
    assert torch.equal(on.env.drain_tape()[0], off.env.drain_tape()[0])
    assert (_np(on.env.check_invariants()) == 0).all() and (on.flags() == off.flags()).all()
    assert int(_np(on.env.order_tape_meta())[:, 0].sum()) == n * steps
    on.close(); off.close()


# ---- 5. behind a played order schedule and after a hook; every refusal ------------------------------------------------------------------------------------------
def test_prices_resolve_against_the_book_the_step_meets_and_every_refusal():
    from gym_continuousdoubleauction_amd import _capi as K
    from gym_continuousdoubleauction_amd import order_tape as OT
    from gym_continuousdoubleauction_amd import orders as OR
    from gym_continuousdoubleauction_amd._lib import CDAError, lib
    from hip_env import HipEnv
    n, a, max_step = 6, 4, 8
    cfg = _cfg(a, max_step=max_step)
    hip, ora = HipEnv(cfg, n, with_info=False), O.OracleEnv(cfg, n)
    env, L = hip.env, lib()
    assert L.cda_policy_step_supported(env._h) == 1 and L.cda_net_step_supported(env._h, 0, 0) == 1
    seeds = np.arange(11, 11 + n, dtype=np.uint64)
    hip.reset(seeds); ora.reset(seeds)
    bids = np.array([[50, 3, 0, 1, 1], [50, 4, 1, 2, 2], [48, 9, 2, 3, 3], [47, 1, 2, 4, 4]], np.int32)
    asks = np.array([[55, 2, 2, 5, 5], [56, 1, 3, 6, 6]], np.int32)
    rows = OR.schedule_with_seed(bids, asks, [[[(1, K.T_LIMIT, K.S_BID, 2, 52, 0)] if t == 1 else [] for t in range(max_step - 1)]])
    sched_of = [0] * (n - 1) + [-1]
    env.set_order_schedule(rows, market_schedule=sched_of)
    spec = SU.Scheduled(ora, rows, sched_of, a, max_step, auto_reset=False)
    with pytest.raises(RuntimeError, match="enable_order_tape"):
        env.order_tape_series()
    env.enable_order_tape(16)
    assert L.cda_policy_step_supported(env._h) == 0 and L.cda_net_step_supported(env._h, 0, 0) == 0
    rp, rng = OrderReplay(n, 16, a), np.random.default_rng(1)
    cover = new_cover()
    for t in range(4):
        if t == 3:                                               # a hook between two steps: the cached levels no longer describe the book
            for e in (hip, ora):
                e.place_order(2, 3, K.T_LIMIT, K.S_ASK, 5, 53)
        acts = SU.law(rng, n, a)
        acts[3][:] = rng.integers(0, 3, (n, a))                  # price levels the seeded book has
        spec.play_all()
        pre = [(ora.get_state(m), ora.get_book(m)) for m in range(n)]
        ora.step(*acts)
        for m, (s, books) in enumerate(pre):
            rp.visit(m, s.t_step, oracle_record(ora, m, s, books, None, np.stack([acts[0][m], acts[3][m], acts[4][m]], axis=1), cover, 1))
            rp.clock(m, s.t_step + 1)
        hip.step(*acts)
        for m in range(n):
            SU.same_market(hip, ora, m, tag=t)
    head = rp.held(0)[0][0, 0]
    assert head[0] == 0 and head[1] & 3 == OT.BID | OT.ASK and head[2:].tolist() == [50, 55]      # the step-0 touch is the seed's: the recorder runs behind the schedule
    assert rp.held(n - 1)[0][0, 0, 1] & 3 == 0                   # the market without a schedule starts empty
    check(env, rp, "schedule and hook")
    env.clear_order_schedule()
    assert L.cda_policy_step_supported(env._h) == 0              # still off: the order tape is on
    with pytest.raises(CDAError, match="cda_run_random"):
        env.run_random(4)
    # the C-level refusals: nothing is launched behind any
    out = torch.zeros(8192, dtype=torch.int64, device=env.device)
    info = torch.zeros((n, 8), dtype=torch.int32, device=env.device)
    p, ip, st = out.data_ptr(), info.data_ptr(), torch.cuda.current_stream().cuda_stream
    assert L.cda_order_tape_series(env._h, 0, n, 0, 4, p, None, ip, st) == K.OK and L.cda_order_flow(env._h, 0, n, 0, p, ip, st) == K.OK
    assert L.cda_order_fills(env._h, 0, n, 0, p, ip, st) == K.ERR_UNSUPPORTED                                          # the trade tape is off
    for bad in ((0, n + 1), (-1, 2), (0, 0), (n, 1)):
        assert L.cda_order_tape_meta(env._h, *bad, p, st) == K.ERR_INVALID and L.cda_order_tape_series(env._h, *bad, 0, 4, p, None, ip, st) == K.ERR_INVALID
        assert L.cda_order_flow(env._h, *bad, 0, p, ip, st) == K.ERR_INVALID and L.cda_order_fills(env._h, *bad, 0, p, ip, st) == K.ERR_INVALID
    assert L.cda_order_tape_meta(env._h, 0, n, None, st) == K.ERR_INVALID and L.cda_order_tape_meta(env._h, 0, n, p + 2, st) == K.ERR_INVALID
    for bad in ((2, 4, p, None, ip), (0, 0, p, None, ip), (0, 4, None, None, ip), (0, 4, p + 8, None, ip), (0, 4, p, p + 2, ip), (0, 4, p, None, ip + 2)):
        assert L.cda_order_tape_series(env._h, 0, n, *bad, st) == K.ERR_INVALID, bad[:2]
    for fn in (L.cda_order_flow, L.cda_order_fills):
        for bad in ((2, p, ip), (-1, p, ip), (0, None, ip), (0, p + 4, ip), (0, p, ip + 2)):
            assert fn(env._h, 0, n, *bad, st) == K.ERR_INVALID, bad[:1]
    for cap_ in (0, 3, 24, (1 << 20) + 1, 1 << 21):
        assert L.cda_order_tape_enable(env._h, cap_) == K.ERR_INVALID
    assert env.order_tape_capacity == 16                         # a refused enable leaves the env as it was
    with pytest.raises(ValueError, match="power of two"):
        env.enable_order_tape(48)
    env.enable_tape(64)
    assert L.cda_order_fills(env._h, 0, n, 0, p, ip, st) == K.OK
    env.disable_order_tape()
    assert L.cda_order_tape_meta(env._h, 0, n, p, st) == K.ERR_UNSUPPORTED and L.cda_order_tape_series(env._h, 0, n, 0, 4, p, None, ip, st) == K.ERR_UNSUPPORTED
    assert L.cda_order_flow(env._h, 0, n, 0, p, ip, st) == K.ERR_UNSUPPORTED and L.cda_order_fills(env._h, 0, n, 0, p, ip, st) == K.ERR_UNSUPPORTED
    assert L.cda_order_flow(env._h, 0, n, 2, p, ip, st) == K.ERR_INVALID                                               # INVALID first, then UNSUPPORTED
    env.disable_tape()
    assert env.order_tape_capacity == 0 and not env.order_tape_enabled and L.cda_policy_step_supported(env._h) == 1
    torch.cuda.synchronize()
    env.run_random(4)
    hip.close(); ora.close()


# ---- 6. ranges and the other entry points ------------------------------------------------------------------------------------------------------------------------
def _oracle_steps(cfg, n, seed, steps, acts_of, first=None, count=None):
    """an oracle stepped beside an env: -> the replay of the recorder over [first, first + count)"""
    a = cfg["num_of_agents"]
    ora = O.OracleEnv(cfg, n)
    ora.reset(np.arange(seed, seed + n, dtype=np.uint64))
    rp, cover = OrderReplay(n, 32, a), new_cover()
    lo, hi = (0, n) if first is None else (first, first + count)
    for t in range(steps):
        acts = acts_of(t)
        pre = [(ora.get_state(m), ora.get_book(m)) for m in range(lo, hi)]
        ora.step(*acts, None, first, count)
        for m, (s, books) in zip(range(lo, hi), pre):
            rp.visit(m, s.t_step, oracle_record(ora, m, s, books, None, np.stack([acts[0][m], acts[3][m], acts[4][m]], axis=1), cover, 1))
            rp.clock(m, s.t_step + 1)
    ora.close()
    return rp


def test_step_range_records_its_range_only():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd._lib import check as ok, lib
    n, a = 24, 4
    cfg = _cfg(a)
    env = CDAVecEnv(cfg, n, with_info=False)
    env.reset(seed=np.arange(7, 7 + n, dtype=np.uint64))
    env.enable_order_tape(32)
    st = torch.cuda.current_stream().cuda_stream
    dev_acts = [[x[0] for x in env.random_actions_device(t, 1, action_seed=3)] for t in range(5)]
    for cat, mean, sigma, price, off in dev_acts:
        ok(lib().cda_step_range(env._h, 8, 8, cat.data_ptr(), mean.data_ptr(), sigma.data_ptr(), price.data_ptr(), off.data_ptr(), None,
                                env.obs.data_ptr(), env.reward.data_ptr(), env._term.data_ptr(), env._trunc.data_ptr(), None, st), "cda_step_range")
    torch.cuda.synchronize()
    rp = _oracle_steps(cfg, n, 7, 5, lambda t: tuple(_np(x) for x in dev_acts[t]), 8, 8)
    assert check(env, rp, "step_range") == 8 * 5
    rec, cnt, _ = (_np(x) for x in env.order_tape_series())
    outside = [m for m in range(n) if not 8 <= m < 16]
    assert not cnt[outside].any() and not rec[outside].any() and not _np(env.order_tape_meta())[outside].any()
    assert (_np(env.order_tape_meta())[8:16, [0, 2]] == 5).all()
    env.close()


def test_group_launches_and_run_scripted_record():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd import order_tape as OT
    n, a = 24, 4
    cfg = _cfg(a)
    env = CDAVecEnv(cfg, n, with_info=False, groups=2)
    env.reset(seed=np.arange(8, 8 + n, dtype=np.uint64))
    env.enable_order_tape(32)
    rng = np.random.default_rng(9)
    acts = [SU.law(rng, n, a) for _ in range(6)]
    for t in range(6):
        env.step(*acts[t], pipelined=True)
        env.sync()
    assert check(env, _oracle_steps(cfg, n, 8, 6, lambda t: acts[t]), "groups") == n * 6
    env.close()
    # scripted slots: their orders are in the step's action buffers when the recorder runs - every fill finds its initiator's order
    env = CDAVecEnv(cfg, n, with_info=False)
    env.reset(seed=8)
    slots = np.zeros((n, a), np.int32)
    slots[:, 0], slots[:, 1] = 1, 2
    env.set_scripted(slots, ["maker", "taker"], seed=9)
    env.enable_order_tape(32); env.enable_tape(1024)
    for _ in range(8):
        env.run_scripted(1, others="random", action_seed=3)
    rec, cnt, _ = (_np(x) for x in env.order_tape_series())
    fills = _np(env.order_fills()[0])
    trows, tcnt = (_np(x) for x in env.tape_last(1024))
    assert cnt.tolist() == [8] * n and tcnt.sum() > 0
    r = rec.reshape(n, -1, 1 + a, 4)[:, :8]
    assert ((r[:, :, 1, 0] & 3) == OT.T_LIMIT).any() and ((r[:, :, 2, 0] >> 2) & 3 != OT.S_NONE).any()            # the maker's quotes, the taker's orders
    assert not fills[:, :, OT.FILL["unmatched_fills"]].any()
    assert fills[:, :, [3, 7, 11, 15]].sum() == sum(int(trows[m, :tcnt[m], 2].sum()) for m in range(n))
    for m in range(n):
        assert np.array_equal(fills[m], OT.fills_from_records(trows[m, :tcnt[m]], r[m], a)), m
    env.close()


# ---- 7. + 9. captured chains; the loop closes ------------------------------------------------------------------------------------------------------------------------
def test_captured_chains_record_across_the_auto_reset_and_the_recorded_flow_replays_as_a_stream():
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd import order_tape as OT
    from gym_continuousdoubleauction_amd import orders as OR
    from gym_continuousdoubleauction_amd._lib import lib
    N, A, T, max_step = 24, 4, 28, 20
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": max_step, "is_render": False}
    env = CDAVecEnv(dict(cfg, auto_reset=True), n_markets=N, with_info=False)
    env.reset(seed=300)
    env.enable_order_tape(64); env.enable_tape(TAPE_CAP)
    assert lib().cda_policy_step_supported(env._h) == 0
    roll = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=1), T, groups=2, seed=5)
    b = {k: _np(v).copy() for k, v in roll.run().items()}
    torch.cuda.synchronize()
    assert roll.graphs is not None
    ora = O.OracleEnv(cfg, N)
    assert np.array_equal(ora.reset(np.arange(300, 300 + N, dtype=np.uint64)).view(np.uint32), b["obs"][0].view(np.uint32))
    rp, cover = OrderReplay(N, 64, A), new_cover()
    la, ex = [], []
    for t in range(T):
        acts = tuple(b[k][t] for k in ("category", "size_mean", "size_sigma", "price", "price_offset"))
        pre = [(ora.get_state(m), ora.get_book(m)) for m in range(N)]
        _, orw, ot, otr, info = ora.step(*acts)
        assert np.array_equal(b["reward"][t].view(np.uint64), orw.view(np.uint64)), t
        for m, (s, books) in enumerate(pre):
            rp.visit(m, s.t_step, oracle_record(ora, m, s, books, None, np.stack([acts[0][m], acts[3][m], acts[4][m]], axis=1), cover, 1))
        if t < max_step:
            la.append(info["lob_actions"].copy()); ex.append(np.array([[ora.trace[i].exec_order[j] for j in range(A)] for i in range(N)]))
        done = ((ot != 0) | (otr != 0)).astype(np.uint8)
        if done.any():
            ora.reset(None, done)
        for m in range(N):
            rp.clock(m, ora.get_state(m).t_step)
    ora.close()
    assert all(rp.rolled(m)["n_episode"] == T - max_step and rp.rolled(m)["n_prev"] == max_step for m in range(N))      # an episode ended inside the graphs
    assert check(env, rp, "rollout") == N * T
    # the previous episode is complete: its stream is the stream the oracle's trace gives, and a fresh twin that is handed it holds the same fills
    la, ex = np.stack(la), np.stack(ex)
    rec, cnt, info = (_np(x) for x in env.order_tape_series(episode="previous"))
    assert cnt.tolist() == [max_step] * N and not info[:, [1, 3]].any()
    streams = [OT.to_stream(rec[m, :max_step], mark_every=4) for m in range(N)]
    for m in range(N):
        assert streams[m] == OR.from_lob_actions(la[:, m], ex[:, m], mark_every=4), m
    twin = CDAVecEnv(cfg, n_markets=N, with_info=False)
    twin.reset(seed=300)
    twin.enable_tape(TAPE_CAP)
    twin.submit_orders(streams)
    want, wcnt = (_np(x) for x in env.tape_last(TAPE_CAP, episode="previous"))
    got, gcnt = (_np(x) for x in twin.tape_last(TAPE_CAP))
    assert np.array_equal(wcnt, gcnt) and wcnt.sum() > N
    want, got = want.copy(), got.copy()
    want[:, :, 7] &= 3; got[:, :, 7] &= 3                        # (every field but the step index: the twin takes no env step)
    for j, f in enumerate(("time", "price", "quantity", "counter_id", "counter_order_id", "counter_left", "init_id", "sides_step")):
        assert np.array_equal(got[:, :, j], want[:, :, j]), f
    twin.close()
    env.disable_order_tape()
    with pytest.raises(RuntimeError, match="order tape"):
        roll.run()
    env.enable_order_tape(64)
    with pytest.raises(RuntimeError, match="order tape"):
        roll.run()
    env.close()


# ---- 8. short rings and restores ---------------------------------------------------------------------------------------------------------------------------------
def test_a_ring_shorter_than_the_episode_reports_the_loss_and_its_fills_are_unmatched():
    from gym_continuousdoubleauction_amd import order_tape as OT
    from hip_env import HipEnv
    case = "24x4-256-h4-t1-all"
    n, a, cap, hist, tick, _ = CASES[case]
    ref = reference(case)
    hip = HipEnv(_cfg(a, cap, n_hist=hist, tick_size=tick, auto_reset=True), n, with_info=False)
    env, ring = hip.env, 16
    env.enable_order_tape(ring); env.enable_tape(TAPE_CAP)
    hip.reset(ref["seeds"])
    for t in range(MAX_STEP - 1):
        if t == 10:
            _done_set(hip, 3, a)
        if t == 12:
            _touch_state(hip, 1)
        hip.step(*ref["acts"][t], ref["present"][t])
    rp = copy.deepcopy(ref["marks"][MAX_STEP])
    rp.capacity = ring
    for m in range(n):                                           # (the reference has taken one step more, the one that ended the episode: drop its record)
        rp.records[m].pop(); rp.meta[m]["n_total"] -= 1; rp.meta[m]["n_episode"] -= 1
        rp.clock(m, rp.meta[m]["first"] + rp.meta[m]["n_episode"])
    live = [m for m in range(n) if m != 3]
    check(env, rp, "short ring", tick)
    rec, cnt, info = (_np(x) for x in env.order_tape_series())
    assert rec.shape[1] == ring and cnt[live].tolist() == [ring] * len(live) and info[live, 1].tolist() == [MAX_STEP - 1 - ring] * len(live)
    assert info[live, 2].tolist() == [MAX_STEP - 1 - ring] * len(live)
    fills, xinfo = (_np(x) for x in env.order_fills())
    trows, tcnt = (_np(x) for x in env.tape_last(TAPE_CAP))
    early = sum(int(((trows[m, :tcnt[m], 7] >> 2) < MAX_STEP - 1 - ring).sum()) for m in live)
    assert early > 0 and fills[live][:, :, OT.FILL["unmatched_fills"]].sum() == early      # the fills of the lost steps are counted, never attributed
    rec, cnt, _ = (_np(x) for x in env.order_tape_series(4, first_market=5, n_markets=2))   # the last k of what is held; a sub-range
    assert rec.shape == (2, 4, 4 * (1 + a)) and cnt.tolist() == [4, 4] and np.array_equal(rec[1].reshape(4, 1 + a, 4), rp.held(6)[0][-4:])
    hip.close()


def test_a_restore_restarts_the_current_episode_partial_and_keeps_the_previous():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd import order_tape as OT
    n, a = 8, 4
    env = CDAVecEnv(_cfg(a, max_step=64), n, with_info=False)
    env.reset(seed=31)
    env.enable_order_tape(128)
    meta = [OT.new_meta() for _ in range(n)]
    clock = [0] * n

    def run(t0, t1):
        for t in range(t0, t1):
            env.step(*env.random_actions(t, action_seed=5))
            for m in range(n):
                meta[m] = OT.record(meta[m], clock[m])
                clock[m] += 1

    def held(m, which="current"):
        sp = OT.span(OT.roll(meta[m], clock[m]), 128, which)
        return sp["count"], sp["lost"], sp["step0"], sp["partial"]

    def same(tag):
        words = _np(env.order_tape_meta())
        for which in ("current", "previous"):
            rec, cnt, info = (_np(x) for x in env.order_tape_series(episode=which))
            for m in range(n):
                assert OT.meta_from_words(words[m]) == OT.roll(meta[m], clock[m]), (tag, m)
                c, lost, s0, partial = held(m, which)
                assert info[m].tolist() == [c, lost, s0, partial] and cnt[m] == c and rec[m, :c, 0].tolist() == list(range(s0, s0 + c)), (tag, which, m)
    run(0, 12)
    env.reset(seed=32)                                         # a finished episode to remember
    clock[:] = [0] * n
    run(0, 10)
    early = env.snapshot(2, 2)                                 # markets 2, 3 at step 10
    run(10, 30)
    env.restore(early, first=2)                                # 30 -> 10
    clock[2] = clock[3] = 10
    same("restored, before a record")                          # the readers roll at once: empty, partial, starting at step 10; the previous episode is kept
    assert held(2) == (0, 0, 10, 1) and held(2, "previous") == (12, 0, 0, 0)
    run(30, 33)
    same("three records behind the restore")
    assert held(2) == (3, 0, 10, 1) and held(5) == (33, 0, 0, 0)
    env.close()


# ---- 10. the evaluation loop -------------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_saves_the_orders_and_reports_the_order_flow(tmp_path):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd import evaluate as EV
    from gym_continuousdoubleauction_amd import order_tape as OT
    N, A, E, max_step = 32, 4, 2, 24
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    pol = mlp.FusedPolicy("cuda:0", seed=5)
    path, tpath = str(tmp_path / "orders.npz"), str(tmp_path / "tape.npz")
    keep = {}
    res = EV.evaluate(env, pol, opponents=["random", "maker"], trained_slots=1, episodes=E, seed=3, orders=path, order_flow_report=True, tape=tpath, keep=keep)
    plain = EV.evaluate(env, pol, opponents=["random", "maker"], trained_slots=1, episodes=E, seed=3)
    assert res["summary"] == plain["summary"] and "orders" not in plain and not env.order_tape_enabled      # the recorder changed nothing, and the env's setting is back
    z = OT.load(path)
    assert z["records"].shape == (N, max_step, 4 * (1 + A)) and int(z["num_agents"]) == A and z["counts"].tolist() == [max_step] * N
    assert (z["records"][:, :, 0] == np.arange(max_step)).all() and list(z["module_names"]) == list(res["modules"]) and not z["info"][:, [1, 3]].any()
    about, tables, modules = res["orders"], keep["order_tables"], keep["modules"]
    assert about["markets"] == N and about["records"] == N * max_step and about["records_lost"] == 0 and tables["counted"].all()
    for m in range(N):                                           # the per-market tables are the specifications of the saved records
        assert np.array_equal(tables["flow"][m], OT.flow_from_records(z["records"][m])), m
    names = list(res["modules"])
    for key, words in (("flow", OT.FLOW_WORDS), ("fills", OT.FILL_WORDS)):
        total = np.zeros(words, np.int64)
        for i, name in enumerate(names):
            row = np.array(res["modules"][name]["orders"][key], np.int64)
            assert np.array_equal(row, tables[key][modules == i].sum(axis=0)), (key, name)
            total += row
        assert np.array_equal(total, OT.pool(tables[key]).sum(axis=0)), key
    pol_block = res["modules"]["policy"]["orders"]
    assert pol_block["steps_present"] == N * max_step and set(pol_block) >= {"type_share", "placement_share", "immediate_fill_ratio", "maker_share", "order_to_trade"}
    assert res["modules"]["opponent_1"]["orders"]["orders"] > 0      # the scripted maker's quotes are in the tape
    env.close()
