"""CPU: the order tape's host side - order_tape.py's record builder, views and the two numpy specifications on hand-worked records, the replay of the
recorder's episode rule (tests/order_tape_replay.py), the round trip into orders.from_lob_actions, and the library's argument check
(cda_order_tape_check_host: no env, no device).  Integers only: every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_continuousdoubleauction_amd import order_tape as OT
from gym_continuousdoubleauction_amd import orders as OR
from gym_continuousdoubleauction_amd import quotes as Q
from order_tape_replay import OrderReplay, touch_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
ENTRY_POINTS = ["cda_order_tape_enable", "cda_order_tape_disable", "cda_order_tape_capacity", "cda_order_tape_meta", "cda_order_tape_series", "cda_order_flow",
                "cda_order_fills", "cda_order_tape_check_host"]
B, S, NONE = OT.S_BID, OT.S_ASK, -1
MKT, LIM, MOD, CXL = OT.T_MARKET, OT.T_LIMIT, OT.T_MODIFY, OT.T_CANCEL


def rec(step, touch, orders, order=None, present=None, raw=None, clamped=None):
    """a record from {agent: (side, type, size, price)}; the others pass"""
    a_n = 4
    dec = np.full((a_n, 4), -1, np.int64)
    for a, o in orders.items():
        dec[a] = o
    acting = sorted(orders)
    return OT.record_from_decoded(step, touch, dec, acting if order is None else order, present, np.zeros((a_n, 3), int) if raw is None else raw, clamped)


def fill(step, init, counter, qty, price=100, init_side=0):
    return [0, price, qty, counter, 0, 0, init, (step << 2) | (init_side << 1) | (1 - init_side)]


# ---- 1. a record ----------------------------------------------------------------------------------------------------------------------------------------------
def test_record_from_decoded_words_ranks_and_the_absent():
    raw = [[3, 12, 5], [0, 0, 0], [9, -1, 1], [6, 2, 2]]
    r = OT.record_from_decoded(7, (99, None), [[B, MOD, 5, 98], [-1] * 4, [S, MKT, 3, -1], [S, LIM, 2, 104]], [3, 0, 2], [1, 1, 1, 1], raw,
                               clamped=[0, 0, 0, 1])
    assert r.dtype == np.int32 and r.shape == (5, 4)
    assert r[0].tolist() == [7, OT.BID | (3 << 8) | (1 << 16), 99, 0]
    assert r[1].tolist() == [MOD | (B << 2) | (1 << 4), 5, 98, 3 | (9 << 4) | (2 << 8)]              # executed second; level 12 clamps to 9, offset 5 to 2
    assert r[2].tolist() == [MKT | (OT.S_NONE << 2), -1, -1, 0]                                       # a pass
    assert r[3].tolist() == [MKT | (S << 2) | (2 << 4), 3, -1, 8 | (0 << 4) | (1 << 8)]              # category 9 clamps to 8, level -1 to 0
    assert r[4].tolist() == [LIM | (S << 2) | (0 << 4) | OT.CLAMPED, 2, 104, 6 | (2 << 4) | (2 << 8)]
    absent = OT.record_from_decoded(0, (None, None), [[B, LIM, 1, 10], [S, LIM, 1, 12]], [1], [0, 2], [[2, 0, 1], [6, 0, 1]])
    assert absent.tolist() == [[0, 1 << 8, 0, 0], [-1, -1, -1, 0], [LIM | (S << 2), 1, 12, 6 | (1 << 8)]]   # an absent agent's order is not in the step
    with pytest.raises(ValueError, match="exec_order"):
        OT.record_from_decoded(0, (None, None), [[B, LIM, 1, 10], [S, LIM, 1, 12]], [0, 0], None, [[2, 0, 1], [6, 0, 1]])
    v = OT.as_orders(np.stack([r, r]))
    assert v["head"]["step"].tolist() == [7, 7] and v["slot"]["price"][0].tolist() == [98, -1, -1, 104] and OT.as_rows(v).shape == (2, 5, 4)
    assert OT.as_rows(np.stack([r, r]).reshape(2, -1)).shape == (2, 5, 4) and OT.as_rows(np.zeros((0, 20), np.int32)).shape == (0, 5, 4)


def test_views_round_trip_into_the_order_streams():
    rng = np.random.default_rng(3)
    T, A = 12, 4
    la = np.full((T, A, 4), -1, np.int64)
    ex = np.full((T, A), -1, np.int64)
    rows = []
    for t in range(T):
        acting = [a for a in range(A) if rng.random() < 0.7]
        for a in acting:
            typ = int(rng.integers(0, 4))
            la[t, a] = (int(rng.integers(0, 2)), typ, int(rng.integers(1, 9)), -1 if typ == MKT else int(rng.integers(90, 110)))
        order = [int(x) for x in rng.permutation(acting)]
        ex[t, :len(order)] = order
        rows.append(OT.record_from_decoded(t, (95, 105), la[t], order, None, np.zeros((A, 3), int)))
    series = np.stack(rows)
    assert np.array_equal(OT.lob_actions(series), la) and np.array_equal(OT.exec_order(series), ex)
    assert OT.to_stream(series, mark_every=5) == OR.from_lob_actions(la, ex, 5) and len(OT.to_stream(series)) == int((la[:, :, 0] >= 0).sum())
    assert OT.to_schedule(series, traders=(1, 3)) == OR.schedule_from_lob_actions(la, ex, (1, 3))
    msgs = OT.messages(series)
    assert len(msgs) == int((la[:, :, 0] >= 0).sum()) and msgs.dtype == OT.MSG_DTYPE
    flat = [(m[5], m[0]) for m in OT.to_stream(series)]                                               # (step tag, agent) in execution order
    assert [(int(m["step"]), int(m["agent"])) for m in msgs] == flat
    k = 0
    for t in range(T):
        for rank, a in enumerate(ex[t][ex[t] >= 0]):
            m = msgs[k]; k += 1
            assert (m["rank"], m["side"], m["type"], m["size"], m["price"], m["best_bid"], m["best_ask"]) == (rank, *la[t, a], 95, 105)
    bad = series.copy()
    bad[0, 1:, 0] = np.where(bad[0, 1:, 0] >= 0, bad[0, 1:, 0] & ~0xF0, bad[0, 1:, 0])                 # every rank 0
    if (OT.lob_actions(bad[:1])[0, :, 0] >= 0).sum() > 1:
        with pytest.raises(ValueError, match="permutation"):
            OT.exec_order(bad)


# ---- 2. the order-flow table ------------------------------------------------------------------------------------------------------------------------------------
def test_every_placement_class_at_its_boundary():
    F = OT.FLOW
    tick = 5

    def one(touch, side, price):
        out = OT.flow_from_records([rec(0, touch, {0: (side, LIM, 1, price)})], tick)
        return {k: int(out[0, F[k]]) for k in ("crossing", "inside", "at_touch", "behind", "behind_ticks", "no_reference")}
    z = dict(crossing=0, inside=0, at_touch=0, behind=0, behind_ticks=0, no_reference=0)
    two = (100, 110)
    assert one(two, B, 110) == dict(z, crossing=1) and one(two, B, 105) == dict(z, inside=1) and one(two, B, 100) == dict(z, at_touch=1)
    assert one(two, B, 95) == dict(z, behind=1, behind_ticks=1) and one(two, B, 70) == dict(z, behind=1, behind_ticks=6)
    assert one(two, S, 100) == dict(z, crossing=1) and one(two, S, 105) == dict(z, inside=1) and one(two, S, 110) == dict(z, at_touch=1)
    assert one(two, S, 125) == dict(z, behind=1, behind_ticks=3) and one(two, B, 200) == dict(z, crossing=1)
    # a one-sided book: the other side cannot be crossed; the own side may be the empty one
    assert one((100, None), B, 500) == dict(z, inside=1) and one((100, None), S, 100) == dict(z, crossing=1) and one((100, None), S, 101) == dict(z, no_reference=1)
    assert one((None, 110), S, 5) == dict(z, inside=1) and one((None, 110), B, 110) == dict(z, crossing=1) and one((None, 110), B, 109) == dict(z, no_reference=1)
    # an empty book
    assert one((None, None), B, 100) == dict(z, no_reference=1) and one((None, None), S, 100) == dict(z, no_reference=1)


def test_flow_counts_presence_types_and_sizes_and_classes_only_limit_orders():
    F = OT.FLOW
    rows = [rec(0, (100, 110), {0: (B, MKT, 3, -1), 1: (S, LIM, 4, 110), 2: (S, MOD, 5, 90), 3: (B, CXL, 6, 120)}, order=[3, 1, 0, 2]),
            rec(1, (100, 110), {0: (B, MKT, 7, -1), 1: (B, LIM, 2, 99)}, present=[1, 1, 0, 1]),
            rec(2, (None, None), {}, present=[1, 0, 0, 0])]
    out = OT.flow_from_records(rows)
    assert out.shape == (4, OT.FLOW_WORDS) and out.dtype == np.int64 and not out[:, len(OT.FLOW_FIELDS):].any()
    assert out[:, F["present"]].tolist() == [3, 2, 1, 2] and out[:, F["absent"]].tolist() == [0, 1, 2, 1] and out[:, F["passes"]].tolist() == [1, 0, 0, 1]
    assert (out[0, F["market_bid_orders"]], out[0, F["market_bid_qty"]]) == (2, 10) and (out[1, F["limit_ask_orders"]], out[1, F["limit_ask_qty"]]) == (1, 4)
    assert (out[1, F["limit_bid_orders"]], out[1, F["limit_bid_qty"]]) == (1, 2) and (out[2, F["modify_ask_qty"]], out[3, F["cancel_bid_qty"]]) == (5, 6)
    assert out[1, F["at_touch"]] == 1 and out[1, F["behind"]] == 1 and out[1, F["behind_ticks"]] == 1
    assert not out[[0, 2, 3]][:, F["crossing"]:].any()                                                # a modify at a crossing price is not classed
    assert np.array_equal(OT.pool(np.stack([out, out])), 2 * out) and OT.pool(out[None]).shape == (4, OT.FLOW_WORDS)
    s = OT.summary(out[1])
    assert s["orders"] == 2 and s["type_share"]["limit"] == 1.0 and s["placement_share"]["at_touch"] == 0.5 and s["mean_ticks_behind"] == 1.0 and s["pass_fraction"] == 0.0
    assert OT.summary(out[2])["type_share"]["modify"] == 1.0 and OT.summary(np.zeros(32, np.int64))["pass_fraction"] is None


# ---- 3. fills against orders ------------------------------------------------------------------------------------------------------------------------------------
def test_fills_are_attributed_by_step_and_initiator_or_counted_unmatched():
    X = OT.FILL
    rows = [rec(4, (100, 110), {0: (B, MKT, 9, -1), 1: (S, LIM, 4, 100)}),                           # agent 2 and 3 pass
            rec(5, (100, 110), {0: (B, LIM, 5, 110), 2: (S, MKT, 2, -1)}),
            rec(6, (100, 110), {3: (B, MOD, 1, 100)})]
    tape = [fill(4, 0, 1, 3), fill(4, 0, 3, 2), fill(4, 1, 0, 4, init_side=1),                        # step 4: agent 0's market order fills twice, agent 1's crossing ask once
            fill(4, 2, 1, 1),                                                                          # ... and a fill whose initiator PASSED in that step (a hook's order)
            fill(5, 0, 0, 5),                                                                          # a self trade
            fill(6, 3, 1, 1), fill(7, 0, 1, 8), fill(3, 1, 0, 6)]                                      # step 7 and step 3: beyond the held span on either end
    out = OT.fills_from_records(np.array(tape, np.int32), np.stack(rows))
    assert out.shape == (4, OT.FILL_WORDS) and not out[:, len(OT.FILL_FIELDS):].any()
    assert out[0, :4].tolist() == [1, 9, 1, 5] and out[0, 4:8].tolist() == [1, 5, 1, 5]                # market: one order of 9, filled 3 + 2; limit: the self trade
    assert out[1, 4:8].tolist() == [1, 4, 1, 4] and out[2, :4].tolist() == [1, 2, 0, 0] and out[3, 8:12].tolist() == [1, 1, 1, 1]
    assert out[:, X["maker_fills"]].tolist() == [3, 4, 0, 1] and out[:, X["maker_qty"]].tolist() == [15, 13, 0, 2]
    assert out[:, X["self_fills"]].tolist() == [1, 0, 0, 0] and out[0, X["self_qty"]] == 5
    assert out[:, X["unmatched_fills"]].tolist() == [1, 1, 1, 0] and out[:, X["unmatched_qty"]].tolist() == [8, 6, 1, 0]
    none = OT.fills_from_records(np.array(tape, np.int32), np.zeros((0, 5, 4), np.int32))              # no order record held: every fill is unmatched
    assert none[:, X["unmatched_fills"]].sum() == len(tape) and not none[:, :16].any()
    outside = OT.fills_from_records(np.array([fill(4, 7, 0, 1), fill(4, 0, 9, 1)], np.int32), np.stack(rows))
    assert not outside[:, 16:].any() and not outside[:, [2, 3]].any()                                  # ids outside the env's agents are skipped
    with pytest.raises(ValueError, match="consecutive"):
        OT.fills_from_records(np.zeros((0, 8), np.int32), np.stack([rows[0], rows[2]]))
    s = OT.summary(OT.flow_from_records(rows)[0], out[0])
    assert s["immediate_fill_ratio"]["market"] == 5 / 9 and s["immediate_fill_share"]["limit"] == 1.0 and s["order_to_trade"] == 1.0 and s["unmatched_fills"] == 1
    assert s["maker_share"] == 15 / 25


def test_save_and_load_round_trip(tmp_path):
    rows = np.stack([rec(t, (100, 110), {0: (B, LIM, 1 + t, 100)}) for t in range(3)])
    path = str(tmp_path / "o.npz")
    OT.save(path, rows.reshape(1, 3, -1), counts=[3], modules=np.zeros((1, 4), np.int32))
    z = OT.load(path)
    assert np.array_equal(z["records"], rows.reshape(1, 3, -1)) and int(z["num_agents"]) == 4 and z["counts"].tolist() == [3] and list(z["slot_fields"]) == list(OT.SLOT_DTYPE.names)
    assert OT.as_orders(z["records"][0])["slot"]["size"][:, 0].tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match="order records"):
        OT.save(path, np.zeros((3, 7), np.int32))


# ---- 4. the replay of the recorder's episode rule -----------------------------------------------------------------------------------------------------------------
def test_the_replay_follows_resets_restores_and_a_short_ring():
    rp = OrderReplay(1, capacity=4, num_agents=4)
    row = lambda s: rec(s, touch_of([[100, 1]], []), {s % 4: (B, LIM, s + 1, 100)})                  # noqa: E731
    for s in range(6):
        rp.visit(0, s, row(s)); rp.clock(0, s + 1)
    rows, count, lost, step0, partial = rp.held(0)
    assert (count, lost, step0, partial) == (4, 2, 2, 0) and rows[:, 0, 0].tolist() == [2, 3, 4, 5] and rows[:, 0, 1].tolist() == [OT.BID | (1 << 8) | (3 << 16)] * 4
    rp.clock(0, 0)                                                       # a reset: the readers roll at once
    assert rp.held(0)[1] == 0 and rp.held(0, "previous")[1:] == (4, 2, 2, 0)
    rp.visit(0, 0, row(0)); rp.clock(0, 1)
    assert rp.held(0, "previous")[1:] == (3, 3, 3, 0) and rp.held(0)[1:] == (1, 0, 0, 0)
    rp.clock(0, 5)                                                       # a restore moved the clock: partial, the fragment becomes a gap
    assert rp.held(0)[1:] == (0, 0, 5, 1) and rp.rolled(0)["gap"] == 1
    rp.visit(0, 5, row(5)); rp.clock(0, 6)
    assert rp.flow(0)[:, OT.FLOW["at_touch"]].tolist() == [0, 1, 0, 0] and rp.flow(0, "previous")[:, OT.FLOW["limit_bid_qty"]].tolist() == [5, 6, 0, 0]
    # the fills of the steps the ring has lost land in unmatched_*
    fills = rp.fills(0, np.array([fill(2, 2, 0, 1), fill(3, 3, 0, 2), fill(4, 0, 1, 3)], np.int32), "previous")
    assert fills[:, OT.FILL["unmatched_qty"]].tolist() == [0, 0, 1, 2] and fills[:, 4 + 3].tolist() == [3, 0, 0, 0]
    assert OT.roll is Q.roll and OT.record is Q.record and OT.span is Q.span and OT.new_meta is Q.new_meta       # taken from quotes.py, not copied


# ---- 5. the library's host check and the header ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip_lib():
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib()


def test_the_host_check_at_each_bound_and_one_beyond(hip_lib):
    L, chk = hip_lib, hip_lib.cda_order_tape_check_host
    E, Sr, R = 0, 1, 2
    for cap in (1, 2, 1024, 1 << 20):
        assert chk(E, 4, cap, 0) == OK
    for cap in (0, -1, 3, 1000, (1 << 20) + 1, 1 << 21):
        assert chk(E, 4, cap, 0) == INVALID
    assert chk(E, 1, 16, 0) == OK and chk(E, 16, 16, 0) == OK and chk(E, 0, 16, 0) == INVALID and chk(E, 17, 16, 0) == INVALID
    assert chk(Sr, 4, 0, 1) == OK and chk(Sr, 4, 1, 1 << 20) == OK and chk(Sr, 4, 2, 1) == INVALID and chk(Sr, 4, -1, 1) == INVALID and chk(Sr, 4, 0, 0) == INVALID
    assert chk(R, 4, 0, 0) == OK and chk(R, 4, 1, 0) == OK and chk(R, 4, 2, 0) == INVALID and chk(R, 17, 0, 0) == INVALID
    assert chk(3, 4, 0, 1) == INVALID and chk(-1, 4, 16, 1) == INVALID
    # the entry points themselves: without an env nothing is launched
    one = C.c_void_p(64)
    assert L.cda_order_tape_enable(None, 16) == INVALID and L.cda_order_tape_disable(None) == INVALID and L.cda_order_tape_capacity(None) == 0
    assert L.cda_order_tape_meta(None, 0, 1, one, None) == INVALID and L.cda_order_tape_series(None, 0, 1, 0, 4, one, None, None, None) == INVALID
    assert L.cda_order_flow(None, 0, 1, 0, one, None, None) == INVALID and L.cda_order_fills(None, 0, 1, 0, one, None, None) == INVALID


def test_constants_field_tuples_and_entry_points_are_the_header_s():
    hdr = open(os.path.join(ROOT, "include", "cda.h")).read()
    for name, value in (("CDA_ORDER_FLOW_WORDS", OT.FLOW_WORDS), ("CDA_ORDER_FILL_WORDS", OT.FILL_WORDS), ("CDA_ORDER_CLAMPED", OT.CLAMPED), ("CDA_QUOTE_BID", OT.BID),
                        ("CDA_QUOTE_ASK", OT.ASK), ("CDA_MAX_AGENTS", OT.MAX_AGENTS), ("CDA_QUOTE_CAP_MAX", None)):
        if value is not None:
            assert re.search(r"#define %s\s+%d\b" % (name, value), hdr), name
    assert OT.CAP_MAX == 1 << 20 and OT.HEAD_DTYPE.itemsize == 16 and OT.SLOT_DTYPE.itemsize == 16 and OT.record_dtype(7).itemsize == 16 * 8
    for struct, dt in (("cda_order_head", OT.HEAD_DTYPE), ("cda_order_slot", OT.SLOT_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        assert tuple(re.findall(r"int32_t (\w+);", body)) == dt.names, struct
    from gym_continuousdoubleauction_amd import _lib
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|int32_t|int64_t) %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS
    inc = open(os.path.join(ROOT, "gym_continuousdoubleauction_amd", "csrc", "cda_hip.hip")).read()
    assert inc.index('#include "cda_depth.inc"') < inc.index('#include "cda_order_tape.inc"')


def test_the_entry_points_are_exported(hip_lib):
    for name in ENTRY_POINTS:
        assert hasattr(hip_lib, name), name
