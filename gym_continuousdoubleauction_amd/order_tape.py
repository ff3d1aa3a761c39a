"""The order tape on the host: the record layout of include/cda.h cda_order_head / cda_order_slot as numpy dtypes, and the SPECIFICATION, in plain numpy, of what
the device does with it - a record from plain decoded orders (record_from_decoded), the order-flow table of CDAVecEnv.order_flow (flow_from_records) and the
fills-against-orders table of CDAVecEnv.order_fills (fills_from_records) - with the views a replay needs (lob_actions, exec_order, to_stream, to_schedule,
messages), a fold (pool), the ratios a person reads (summary) and an .npz container.  The device results equal these word for word.  No device code here:
importable without a GPU.

One record per env step and market: a head word - the step, the touch ahead of the step, how many agents sent an order and how many passed - and one slot per
agent: what the step decoded from the agent's action (type, side, size, price: the `lob_actions` info words) and the rank the step's shuffle gave it in the
execution order.  The episode rule is the quote tape's (quotes.roll), over a meta row of this service's own."""
import numpy as np

from .quotes import CAP_MAX, META_FIELDS, PARTIAL, PREV_PARTIAL, meta_from_words, new_meta, record, roll, span  # noqa: F401  (re-exported: ONE episode rule)

HEAD_DTYPE = np.dtype([("step", "<i4"), ("flags", "<i4"), ("best_bid", "<i4"), ("best_ask", "<i4")])
SLOT_DTYPE = np.dtype([("code", "<i4"), ("size", "<i4"), ("price", "<i4"), ("action", "<i4")])
BID, ASK = 1, 2                                                  # bits of the head's flags (CDA_QUOTE_BID, CDA_QUOTE_ASK); bits 8..15 orders, 16..23 passes
CLAMPED = 256                                                    # bit 8 of a slot's code (CDA_ORDER_CLAMPED)
T_MARKET, T_LIMIT, T_MODIFY, T_CANCEL = 0, 1, 2, 3
S_BID, S_ASK, S_NONE = 0, 1, 2
TYPES = ("market", "limit", "modify", "cancel")
SIDES = ("bid", "ask")
MAX_AGENTS = 16
K_ROWS = 10

# the 32 int64 words per agent of CDAVecEnv.order_flow (include/cda.h CDA_ORDER_FLOW_WORDS)
FLOW_FIELDS = ("present", "passes", "absent") + tuple(f"{t}_{s}_{w}" for t in TYPES for s in SIDES for w in ("orders", "qty")) + \
              ("crossing", "inside", "at_touch", "behind", "behind_ticks", "no_reference")
FLOW_WORDS = 32
FLOW = {name: i for i, name in enumerate(FLOW_FIELDS)}
# the 24 int64 words per agent of CDAVecEnv.order_fills (CDA_ORDER_FILL_WORDS)
FILL_FIELDS = tuple(f"{t}_{w}" for t in TYPES for w in ("orders", "qty", "filled_orders", "filled_qty")) + \
              ("maker_fills", "maker_qty", "self_fills", "self_qty", "unmatched_fills", "unmatched_qty")
FILL_WORDS = 24
FILL = {name: i for i, name in enumerate(FILL_FIELDS)}
assert len(FLOW_FIELDS) == 25 and len(FILL_FIELDS) == 22

MSG_DTYPE = np.dtype([("step", "<i4"), ("rank", "<i4"), ("agent", "<i4"), ("type", "<i4"), ("side", "<i4"), ("size", "<i4"), ("price", "<i4"),
                      ("best_bid", "<i4"), ("best_ask", "<i4")])


def record_dtype(num_agents):
    """one record of an env with `num_agents` agents: the head, then a slot per agent"""
    return np.dtype([("head", HEAD_DTYPE), ("slot", SLOT_DTYPE, (int(num_agents),))])


def as_rows(series, num_agents=None):
    """int32 [K, 1 + A, 4] host array of anything that holds one market's order records (a device tensor [K, (1 + A) * 4], a structured array, nested lists)"""
    if hasattr(series, "detach"):
        series = series.detach().cpu().numpy()
    rows = np.asarray(series)
    if rows.dtype.names is not None:
        a = rows.dtype["slot"].shape[0]
        rows = np.ascontiguousarray(rows).view(np.int32).reshape(-1, 1 + a, 4)
    rows = np.asarray(rows, dtype=np.int32)
    if rows.size == 0:
        a = int(num_agents) if num_agents is not None else (rows.shape[-2] - 1 if rows.ndim == 3 else rows.shape[-1] // 4 - 1 if rows.ndim == 2 else 0)
        return np.zeros((0, 1 + max(a, 0), 4), np.int32)
    if rows.ndim == 2 and rows.shape[1] % 4 == 0:
        rows = rows.reshape(rows.shape[0], rows.shape[1] // 4, 4)
    if rows.ndim != 3 or rows.shape[2] != 4 or not 2 <= rows.shape[1] <= 1 + MAX_AGENTS or (num_agents is not None and rows.shape[1] != 1 + int(num_agents)):
        raise ValueError(f"order records must have shape [K, 1 + A, 4] or [K, (1 + A) * 4], got {rows.shape}")
    return np.ascontiguousarray(rows)


def as_orders(series, num_agents=None):
    """structured view (record_dtype(A)) of one market's rows: r['head']['step'], r['slot']['price'][:, a], ..."""
    rows = as_rows(series, num_agents)
    return rows.reshape(len(rows), -1).view(record_dtype(rows.shape[1] - 1)).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- a record
def clamp_action(category, level, offset):
    """the clamped raw action word of a slot: category 0 .. 8 | price level 0 .. 9 << 4 | price offset 0 .. 2 << 8"""
    return min(max(int(category), 0), 8) | (min(max(int(level), 0), K_ROWS - 1) << 4) | (min(max(int(offset), 0), 2) << 8)


def record_from_decoded(step, touch, decoded, exec_order, present, raw_actions, clamped=None):
    """One record from plain decoded orders: int32 [1 + A, 4].  What the recorder stores ahead of step `step`.
    touch        (best_bid, best_ask) of the book ahead of the step; None (or NaN) for an empty side.
    decoded      [A, 4] rows (side, type, size, price) as info["lob_actions"] holds them: side -1 = the agent sent no order (it passed, or was not present).
    exec_order   the acting agents in the order the step executed them (only the first len(acting) entries are read).
    present      [A] truthy where the agent was in the step's action dict; None = every agent.
    raw_actions  [A, 3] rows (category, price level, price offset) as the caller passed them (clamped here).
    clamped      [A] truthy where the decode clamped size or price; None = nowhere."""
    dec = np.asarray(decoded, dtype=np.int64).reshape(-1, 4)
    a_n = len(dec)
    pres = np.ones(a_n, bool) if present is None else np.asarray(present).reshape(-1) != 0
    raw = np.asarray(raw_actions, dtype=np.int64).reshape(a_n, 3)
    cl = np.zeros(a_n, bool) if clamped is None else np.asarray(clamped).reshape(-1) != 0
    acting = [a for a in range(a_n) if pres[a] and dec[a, 0] >= 0]
    order = [int(x) for x in np.asarray(exec_order).reshape(-1)[:len(acting)]]
    if sorted(order) != acting:
        raise ValueError(f"exec_order {order} does not list the acting agents {acting}")
    out = np.zeros((1 + a_n, 4), np.int64)
    sides = []
    for v in touch:
        sides.append(None if v is None or (isinstance(v, float) and np.isnan(v)) else int(v))
    n_pass = int(sum(1 for a in range(a_n) if pres[a] and dec[a, 0] < 0))
    out[0] = (int(step), (BID if sides[0] is not None else 0) | (ASK if sides[1] is not None else 0) | (len(acting) << 8) | (n_pass << 16), sides[0] or 0, sides[1] or 0)
    for a in range(a_n):
        if not pres[a]:
            out[1 + a] = (-1, -1, -1, 0)
        elif dec[a, 0] < 0:
            out[1 + a] = (T_MARKET | (S_NONE << 2) | (CLAMPED if cl[a] else 0), -1, -1, clamp_action(*raw[a]))
        else:
            out[1 + a] = (int(dec[a, 1]) | (int(dec[a, 0]) << 2) | (order.index(a) << 4) | (CLAMPED if cl[a] else 0), dec[a, 2], dec[a, 3], clamp_action(*raw[a]))
    return out.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- views of a series
def _sent(code):
    return (code >= 0) & (((code >> 2) & 3) != S_NONE)


def lob_actions(series):
    """[T, A, 4] rows (side, type, size, price), -1 where the agent sent no order: exactly the step's own `lob_actions` info tensor, step by step - what
    orders.from_lob_actions / schedule_from_lob_actions take"""
    r = as_rows(series).astype(np.int64)
    code = r[:, 1:, 0]
    sent = _sent(code)
    out = np.full(code.shape + (4,), -1, np.int32)
    out[..., 0] = np.where(sent, (code >> 2) & 3, -1)
    out[..., 1] = np.where(sent, code & 3, -1)
    out[..., 2] = np.where(sent, r[:, 1:, 1], -1)
    out[..., 3] = np.where(sent, r[:, 1:, 2], -1)
    return out


def exec_order(series):
    """[T, A]: step t's acting agents in the order they executed, padded with -1"""
    r = as_rows(series).astype(np.int64)
    code = r[:, 1:, 0]
    sent = _sent(code)
    out = np.full(code.shape, -1, np.int32)
    for t in range(len(r)):
        acting = np.nonzero(sent[t])[0]
        ranks = (code[t, acting] >> 4) & 15
        if sorted(ranks.tolist()) != list(range(len(acting))):
            raise ValueError(f"record {t}: the execution ranks {ranks.tolist()} are no permutation")
        out[t, ranks] = acting
    return out


def to_stream(series, mark_every=0):
    """one market's recorded flow as an order stream (orders.from_lob_actions over the tape's own decoded orders and execution order)"""
    from .orders import from_lob_actions
    return from_lob_actions(lob_actions(series), exec_order(series), mark_every)


def to_schedule(series, traders=None):
    """... and as one schedule row: a window per recorded step (orders.schedule_from_lob_actions)"""
    from .orders import schedule_from_lob_actions
    return schedule_from_lob_actions(lob_actions(series), exec_order(series), traders)


def messages(series):
    """a flat structured array (MSG_DTYPE), one row per order in execution order: step, rank, agent, type, side, size, price, best bid and best ask"""
    r = as_rows(series).astype(np.int64)
    eo = exec_order(series)
    out = []
    for t in range(len(r)):
        for rank, a in enumerate(eo[t]):
            if a < 0:
                break
            code, size, price, _ = r[t, 1 + a]
            out.append((r[t, 0, 0], rank, a, code & 3, (code >> 2) & 3, size, price, r[t, 0, 2], r[t, 0, 3]))
    return np.array(out, dtype=MSG_DTYPE)


# ---------------------------------------------------------------------------------------------------------------- the two reports
def flow_from_records(series, tick_size=1):
    """The order-flow table of ONE market's held records: int64 [A, FLOW_WORDS] (FLOW_FIELDS, then zeros).  What CDAVecEnv.order_flow computes on the device.
    Placement classes, for LIMIT orders against the record's own touch: crossing (bid price >= best_ask with the ask side non-empty; ask price <= best_bid with
    the bid side non-empty), else no_reference where the own side is empty, else inside (improves the own best), at_touch, behind with behind_ticks = the
    distance to the own best // tick_size."""
    r = as_rows(series).astype(np.int64)
    a_n = r.shape[1] - 1
    tick = max(1, int(tick_size))
    out = np.zeros((a_n, FLOW_WORDS), np.int64)
    for rec in r:
        _, flags, bb, ba = rec[0]
        for a in range(a_n):
            code, size, price, _ = rec[1 + a]
            row = out[a]
            if code < 0:
                row[FLOW["absent"]] += 1
                continue
            row[FLOW["present"]] += 1
            typ, side = code & 3, (code >> 2) & 3
            if side == S_NONE:
                row[FLOW["passes"]] += 1
                continue
            row[3 + 2 * (typ * 2 + side)] += 1
            row[3 + 2 * (typ * 2 + side) + 1] += size
            if typ != T_LIMIT:
                continue
            has_bid, has_ask = bool(flags & BID), bool(flags & ASK)
            crossing = (has_ask and price >= ba) if side == S_BID else (has_bid and price <= bb)
            own = has_bid if side == S_BID else has_ask
            d = bb - price if side == S_BID else price - ba
            if crossing:
                row[FLOW["crossing"]] += 1
            elif not own:
                row[FLOW["no_reference"]] += 1
            elif d < 0:
                row[FLOW["inside"]] += 1
            elif d == 0:
                row[FLOW["at_touch"]] += 1
            else:
                row[FLOW["behind"]] += 1
                row[FLOW["behind_ticks"]] += d // tick
    return out


def fills_from_records(tape_rows, series, num_agents=None):
    """The fills-against-orders table of ONE market's episode: its held tape rows (tape.RECORD_DTYPE rows, tape order) joined on the fill's step to its HELD order
    records (oldest first: consecutive steps) -> int64 [A, FILL_WORDS] (FILL_FIELDS, then zeros).  What CDAVecEnv.order_fills computes on the device.
    Per type: orders and submitted quantity over the held order records; filled_orders = the orders with at least one held fill as initiator in their own step,
    filled_qty = the quantity of those fills: a fill with init_id == a at step s belongs to agent a's one order of step s.  maker_*: fills with counter_id == a;
    self_*: both ids == a; unmatched_*: fills with init_id == a whose step has no held order record, or in whose step a sent no order (hook, stream or scheduled
    flow) - counted, never attributed.  A fill with an id outside 0 .. A - 1 is skipped."""
    from .tape import as_rows as tape_rows_of
    r = as_rows(series, num_agents).astype(np.int64)
    a_n = r.shape[1] - 1
    t = tape_rows_of(tape_rows).astype(np.int64) if np.size(tape_rows) else np.zeros((0, 8), np.int64)
    out = np.zeros((a_n, FILL_WORDS), np.int64)
    if len(r) and not np.array_equal(r[:, 0, 0], r[0, 0, 0] + np.arange(len(r))):
        raise ValueError("the order records are not the consecutive steps of one episode")
    for rec in r:
        for a in range(a_n):
            code, size = rec[1 + a, 0], rec[1 + a, 1]
            if code >= 0 and (code >> 2) & 3 != S_NONE:
                out[a, 4 * (code & 3)] += 1
                out[a, 4 * (code & 3) + 1] += size
    o0, o1 = (int(r[0, 0, 0]), int(r[-1, 0, 0])) if len(r) else (0, -1)
    seen = set()
    for cid, iid, n, ss in zip(t[:, 3], t[:, 6], t[:, 2], t[:, 7]):
        cid, iid, s = int(cid), int(iid), int((ss & 0xFFFFFFFF) >> 2)
        if not (0 <= cid < a_n and 0 <= iid < a_n):
            continue
        out[cid, FILL["maker_fills"]] += 1
        out[cid, FILL["maker_qty"]] += n
        if cid == iid:
            out[iid, FILL["self_fills"]] += 1
            out[iid, FILL["self_qty"]] += n
        code = int(r[s - o0, 1 + iid, 0]) if o0 <= s <= o1 else -1
        if code < 0 or (code >> 2) & 3 == S_NONE:
            out[iid, FILL["unmatched_fills"]] += 1
            out[iid, FILL["unmatched_qty"]] += n
            continue
        if (iid, s) not in seen:
            seen.add((iid, s))
            out[iid, 4 * (code & 3) + 2] += 1
        out[iid, 4 * (code & 3) + 3] += n
    return out


def pool(tables):
    """a plain sum over the leading axes of per-market tables ([N, A, W] -> [A, W]) - every word of both reports is additive"""
    t = np.asarray(tables.detach().cpu().numpy() if hasattr(tables, "detach") else tables, dtype=np.int64)
    if t.ndim < 2:
        raise ValueError(f"pool takes tables [..., A, W], got {t.shape}")
    return t.reshape(-1, t.shape[-2], t.shape[-1]).sum(axis=0)


def _ratio(x, y):
    return float(x) / float(y) if y else None


def summary(flow, fills=None):
    """The ratios a person reads off ONE row (an agent's, or a module's sum): flow [FLOW_WORDS], fills [FILL_WORDS] or None -> a dict.  Per type the share of the
    orders sent, the pass fraction, the placement shares of the limit orders and the mean ticks behind; with the fills table the immediate fill ratio per type
    (filled quantity / submitted quantity), the maker share of the agent's fills and the order-to-trade ratio.  A ratio whose denominator is 0 is None."""
    f = np.asarray(flow.detach().cpu().numpy() if hasattr(flow, "detach") else flow, dtype=np.int64).reshape(-1)
    if len(f) != FLOW_WORDS:
        raise ValueError(f"summary takes one row of {FLOW_WORDS} words, got {len(f)}")
    per_type = [int(f[3 + 4 * t] + f[3 + 4 * t + 2]) for t in range(4)]
    orders, limits = sum(per_type), per_type[T_LIMIT]
    out = {"steps_present": int(f[FLOW["present"]]), "orders": orders, "pass_fraction": _ratio(f[FLOW["passes"]], f[FLOW["present"]]),
           "type_share": {name: _ratio(per_type[t], orders) for t, name in enumerate(TYPES)},
           "placement_share": {k: _ratio(f[FLOW[k]], limits) for k in ("crossing", "inside", "at_touch", "behind", "no_reference")},
           "mean_ticks_behind": _ratio(f[FLOW["behind_ticks"]], f[FLOW["behind"]])}
    if fills is not None:
        x = np.asarray(fills.detach().cpu().numpy() if hasattr(fills, "detach") else fills, dtype=np.int64).reshape(-1)
        if len(x) != FILL_WORDS:
            raise ValueError(f"summary takes one fills row of {FILL_WORDS} words, got {len(x)}")
        taken = int(sum(x[4 * t + 3] for t in range(4)))
        taker_fills_orders = int(sum(x[4 * t + 2] for t in range(4)))
        out["immediate_fill_ratio"] = {name: _ratio(x[4 * t + 3], x[4 * t + 1]) for t, name in enumerate(TYPES)}
        out["immediate_fill_share"] = {name: _ratio(x[4 * t + 2], x[4 * t]) for t, name in enumerate(TYPES)}
        out["maker_share"] = _ratio(x[FILL["maker_qty"]], int(x[FILL["maker_qty"]]) + taken)
        out["order_to_trade"] = _ratio(orders, taker_fills_orders)
        out["unmatched_fills"] = int(x[FILL["unmatched_fills"]])
    return out


# ---------------------------------------------------------------------------------------------------------------- container
def save(path, records, counts=None, **extra):
    """records i32 [N, K, (1 + A) * 4] (or one market's [K, (1 + A) * 4]) as CDAVecEnv.order_tape_series returns them (+ counts i32 [N]; + any further arrays) -> .npz"""
    rec = records.detach().cpu().numpy() if hasattr(records, "detach") else np.asarray(records)
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    if rec.ndim not in (2, 3) or rec.shape[-1] % 4 or not 2 <= rec.shape[-1] // 4 <= 1 + MAX_AGENTS:
        raise ValueError(f"order records must have shape [N, K, (1 + A) * 4] or [K, (1 + A) * 4], got {rec.shape}")
    data = {"records": rec, "num_agents": np.int32(rec.shape[-1] // 4 - 1), "head_fields": np.array(HEAD_DTYPE.names), "slot_fields": np.array(SLOT_DTYPE.names)}
    if counts is not None:
        data["counts"] = np.asarray(counts.detach().cpu().numpy() if hasattr(counts, "detach") else counts, dtype=np.int32)
    for k, v in extra.items():
        data[k] = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    np.savez_compressed(path, **data)


def load(path):
    """the arrays save wrote, as a dict (as_orders() gives the named view of one market's rows)"""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
