"""Order streams (include/cda.h cda_submit_orders; CDAVecEnv.submit_orders / seed_books): explicit messages - market, limit, modify, cancel orders and
mark_to_mkt - played into many markets in one launch.  This module is the host side: the 16-byte message and result records as numpy structured types,
packing per-market lists into the CSR form the device reads, the validity rule, converters from what the env already hands out (info["lob_actions"], a
Level-3 book dump), and the plain-Python statement of what a result record holds; and the host side of order schedules (include/cda.h cda_schedule_*;
CDAVecEnv.set_order_schedule): packing rows of per-step windows, cutting a recorded episode into them, the seed window, files and the digest a checkpoint
keeps.  Nothing here touches a device."""
import numpy as np

from . import _capi as K

# cda_order_msg / cda_order_result (include/cda.h)
MSG_DTYPE = np.dtype([("price", np.int32), ("size", np.int32), ("trader", np.int16), ("type", np.int8), ("side", np.int8), ("tag", np.int32)])
RESULT_DTYPE = np.dtype([("status", np.int32), ("n_fills", np.int32), ("position_delta", np.int32), ("resting_delta", np.int32)])
assert MSG_DTYPE.itemsize == 16 and RESULT_DTYPE.itemsize == 16

T_MARKET, T_LIMIT, T_MODIFY, T_CANCEL = K.T_MARKET, K.T_LIMIT, K.T_MODIFY, K.T_CANCEL
OP_MARK = 4                                         # CDA_OP_MARK: Exchg_Helper.mark_to_mkt; carries nothing but its type
ORD_INVALID, ORD_REJECTED, ORD_DONE = 0, 1, 2       # CDA_ORD_*
CLEAR_STEP_COUNTERS = 1                             # CDA_ORDERS_CLEAR_STEP_COUNTERS
SUMMARY_FIELDS = ("done", "rejected", "invalid", "fills")
SCHEDULE_LOOP, SCHEDULE_CLEAR_STEP_COUNTERS = 1, 2  # CDA_SCHEDULE_*
SCHEDULE_FAULTS = {1: "sched_of out of range", 2: "negative start", 3: "decreasing row", 4: "end beyond n_msgs"}     # CDA_SCHEDULE_BAD_*

MARK = ("mark",)


def message(trader, type_, side, size, price=0, tag=0):
    """one message as a MSG_DTYPE scalar array (no checks: check() judges it)"""
    m = np.zeros(1, MSG_DTYPE)
    m["trader"], m["type"], m["side"], m["size"], m["price"], m["tag"] = trader, type_, side, size, price, tag
    return m


def _one(item):
    if isinstance(item, np.void) and item.dtype == MSG_DTYPE:
        return tuple(item[f] for f in ("trader", "type", "side", "size", "price", "tag"))
    t = tuple(item)
    if len(t) == 1 and t[0] == "mark":
        return (0, OP_MARK, 0, 0, 0, 0)
    if len(t) == 5:
        return t + (0,)
    if len(t) == 6:
        return t
    raise ValueError(f"a message is (trader, type, side, size, price[, tag]) or ('mark',), got {item!r}")


def pack(streams):
    """A list of N per-market sequences of (trader, type, side, size, price[, tag]) or ("mark",) -> (offsets int64 [N + 1], msgs MSG_DTYPE [total]):
    market i owns msgs[offsets[i] : offsets[i + 1]].  A sequence may also be a MSG_DTYPE array.  Values are stored as given (check() judges them); one that does
    not fit its field raises."""
    offsets = np.zeros(len(streams) + 1, np.int64)
    parts = []
    for i, st in enumerate(streams):
        if isinstance(st, np.ndarray) and st.dtype == MSG_DTYPE:
            part = np.ascontiguousarray(st).reshape(-1)
        else:
            rows = [_one(x) for x in st]
            part = np.zeros(len(rows), MSG_DTYPE)
            for j, f in enumerate(("trader", "type", "side", "size", "price", "tag")):
                col = np.array([int(r[j]) for r in rows], np.int64)
                info = np.iinfo(MSG_DTYPE[f])
                if col.size and (col.min() < info.min or col.max() > info.max):
                    raise ValueError(f"market {i}: a message's {f} does not fit {MSG_DTYPE[f]}")
                part[f] = col
        parts.append(part)
        offsets[i + 1] = offsets[i] + len(part)
    msgs = np.concatenate(parts) if parts else np.zeros(0, MSG_DTYPE)
    return offsets, np.ascontiguousarray(msgs.astype(MSG_DTYPE, copy=False))


def unpack(offsets, msgs):
    """the inverse of pack(): a list of per-market lists of 6-tuples (a mark comes back as ("mark",))"""
    out = []
    for i in range(len(offsets) - 1):
        rows = []
        for m in msgs[int(offsets[i]):int(offsets[i + 1])]:
            rows.append(MARK if int(m["type"]) == OP_MARK else tuple(int(m[f]) for f in ("trader", "type", "side", "size", "price", "tag")))
        out.append(rows)
    return out


def valid(msgs, num_agents):
    """bool [n]: which messages lie in the accepted domain (the rule of cda_place_order: trader 0 .. num_agents-1, type 0 .. 3, side 0 / 1, size >= 1, price >= 1
    for limit / modify / cancel; a mark - type 4 - is always valid, its other fields are not looked at).  The device skips the others."""
    m = np.asarray(msgs)
    typ = m["type"].astype(np.int64)
    order = ((m["trader"] >= 0) & (m["trader"].astype(np.int64) < int(num_agents)) & (typ >= 0) & (typ <= 3) & (m["side"] >= 0) & (m["side"] <= 1) & (m["size"] >= 1)
             & ((typ == 0) | (m["price"] >= 1)))
    return (typ == OP_MARK) | order


def check(msgs, num_agents):
    """index of the first invalid message, -1 = every message is valid (cda_order_msgs_check_host's answer)"""
    bad = np.flatnonzero(~valid(msgs, num_agents))
    return int(bad[0]) if bad.size else -1


def from_lob_actions(lob_actions, exec_order=None, mark_every=0):
    """The decoded orders of T steps, info["lob_actions"] rows [T, A, 4] = (side, type, size, price; side -1 = the agent passed), as one market's stream.
    exec_order: int [T, >= acting agents] - step t's acting agents in the order they executed (the step shuffles them); None = agent order.  Only a step's
    first (number of acting agents) entries are read.  mark_every = k > 0 puts a mark behind every k orders."""
    la = np.asarray(lob_actions)
    if la.ndim != 3 or la.shape[2] != 4:
        raise ValueError(f"lob_actions must be [T, A, 4], got {la.shape}")
    out, n = [], 0
    for t in range(la.shape[0]):
        acting = [a for a in range(la.shape[1]) if la[t, a, 0] >= 0]
        order = acting if exec_order is None else [int(a) for a in np.asarray(exec_order)[t][:len(acting)]]
        if sorted(order) != acting:
            raise ValueError(f"step {t}: exec_order {order} does not list the acting agents {acting}")
        for a in order:
            side, typ, size, price = (int(v) for v in la[t, a])
            out.append((a, typ, side, size, price if typ != T_MARKET else 0, t))
            n += 1
            if mark_every and n % mark_every == 0:
                out.append(MARK)
    return out


def from_book(bids, asks):
    """get_book() / book_orders() rows (price, qty, owner, order_id, timestamp) of one market, IN THE DUMP'S QUEUE ORDER, as limit messages that rebuild the
    book in an empty market: the bids, then the asks, each side best price first - same prices, quantities, owners and queue positions; order ids and
    timestamps are new.  Two things can keep a message from resting as dumped: approval (Trader._order_approved) rejects it where the target account lacks
    the cash for it, and a limit order at a price where its owner already rests on that side is an upsert, not a second order - a dump that holds such a
    pair raises here."""
    out = []
    for side, rows in ((K.S_BID, bids), (K.S_ASK, asks)):
        r = np.asarray(rows).reshape(-1, 5)
        seen = set()
        for price, qty, owner in r[:, :3].tolist():
            if (owner, price) in seen:
                raise ValueError(f"owner {owner} rests twice at price {price} on side {side}: limit messages cannot rebuild that")
            seen.add((owner, price))
            out.append((int(owner), T_LIMIT, side, int(qty), int(price), 0))
    return out


def expected_results(msgs, num_agents, states, tape_counts, book_counts):
    """The specification of cda_order_result.  msgs: one market's stream; states / tape_counts / book_counts: what get_state(), the tape's fill count and the
    market's resting-order count (both sides, tile and ring) read around the stream's VALID messages played one by one - entry j before the j-th valid message,
    entry j + 1 after it (n_valid + 1 entries each).  -> RESULT_DTYPE [len(msgs)]:
      status          ORD_INVALID outside the domain (all deltas 0); ORD_REJECTED when the trader's num_rejected_step grew; else ORD_DONE
      n_fills         fills the message caused = records the tape gained
      position_delta  the trader's net_position after - before (0 for a mark)
      resting_delta   the market's resting orders after - before"""
    ok = valid(msgs, num_agents)
    assert len(states) == len(tape_counts) == len(book_counts) == int(ok.sum()) + 1
    out = np.zeros(len(msgs), RESULT_DTYPE)
    j = 0
    for i, m in enumerate(msgs):
        if not ok[i]:
            out[i]["status"] = ORD_INVALID
            continue
        before, after = states[j], states[j + 1]
        status, dpos = ORD_DONE, 0
        if int(m["type"]) != OP_MARK:
            tr = int(m["trader"])
            if after.acc[tr].num_rejected_step != before.acc[tr].num_rejected_step:
                status = ORD_REJECTED
            dpos = after.acc[tr].net_position - before.acc[tr].net_position
        out[i] = (status, int(tape_counts[j + 1]) - int(tape_counts[j]), dpos, int(book_counts[j + 1]) - int(book_counts[j]))
        j += 1
    return out


def summary_of(results):
    """the [4] summary row (done, rejected, invalid, fills) of one market's result records"""
    r = np.asarray(results)
    return np.array([(r["status"] == ORD_DONE).sum(), (r["status"] == ORD_REJECTED).sum(), (r["status"] == ORD_INVALID).sum(), r["n_fills"].sum()], np.int32)


# ---- order schedules -------------------------------------------------------------------------------------------------------------
class PackedSchedule:
    """An order schedule in the form the device reads: step_offsets int64 [n_sched, S + 1] into msgs (MSG_DTYPE [total]); row r owns, for step t of an episode,
    msgs[step_offsets[r, t] : step_offsets[r, t + 1]]."""

    def __init__(self, step_offsets, msgs):
        self.step_offsets = np.ascontiguousarray(np.asarray(step_offsets, np.int64))
        m = np.asarray(msgs)
        self.msgs = np.ascontiguousarray(m if m.dtype == MSG_DTYPE else m.view(np.uint8).reshape(-1).view(MSG_DTYPE))
        if self.step_offsets.ndim != 2 or self.step_offsets.shape[0] < 1 or self.step_offsets.shape[1] < 2:
            raise ValueError(f"step_offsets must be [n_sched >= 1, S + 1 >= 2], got {self.step_offsets.shape}")

    def __iter__(self):                                 # step_offsets, msgs = pack_schedule(rows)
        return iter((self.step_offsets, self.msgs))

    n_sched = property(lambda self: self.step_offsets.shape[0])
    n_steps = property(lambda self: self.step_offsets.shape[1] - 1)

    def window(self, r, t):
        return self.msgs[int(self.step_offsets[r, t]):int(self.step_offsets[r, t + 1])]

    def rows(self):
        """the inverse of pack_schedule()"""
        return [unpack(self.step_offsets[r], self.msgs) for r in range(self.n_sched)]


def pack_schedule(rows):
    """rows[r][t] = the messages of step t of schedule row r (each a sequence pack() takes) -> PackedSchedule.  Every row must hold the same number S >= 1 of
    windows; a window may be empty."""
    rows = [list(r) for r in rows]
    if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("a schedule needs >= 1 rows of the same number >= 1 of windows")
    S = len(rows[0])
    off, msgs = pack([w for r in rows for w in r])
    step_offsets = np.empty((len(rows), S + 1), np.int64)
    for r in range(len(rows)):
        step_offsets[r] = off[r * S:r * S + S + 1]
    return PackedSchedule(step_offsets, msgs)


def schedule_from_lob_actions(lob_actions, exec_order=None, traders=None):
    """The per-step split of from_lob_actions(): T windows, window t = step t's decoded orders (info["lob_actions"] rows [T, A, 4]) in the order they executed,
    restricted to the slots in `traders` (None = every slot) - a recorded episode's opponents as one schedule row."""
    la = np.asarray(lob_actions)
    if la.ndim != 3 or la.shape[2] != 4:
        raise ValueError(f"lob_actions must be [T, A, 4], got {la.shape}")
    keep = None if traders is None else {int(a) for a in traders}
    out = []
    for t in range(la.shape[0]):
        step = from_lob_actions(la[t:t + 1], None if exec_order is None else np.asarray(exec_order)[t:t + 1])
        out.append([(m[0], m[1], m[2], m[3], m[4], t) for m in step if keep is None or m[0] in keep])
    return out


def schedule_with_seed(bids, asks, rows):
    """every row with from_book(bids, asks) prepended as window 0: the book every episode of a scheduled market starts from (the rows' own windows move one step back)"""
    seed = from_book(bids, asks)
    return [[list(seed)] + [list(w) for w in r] for r in rows]


def schedule_check(sched, sched_of, num_agents, n_markets=None):
    """cda_schedule_attach's rule on host data, stated here in Python (cda_schedule_check_host is the library's): None, or the name of the first fault
    (SCHEDULE_FAULTS)"""
    so = np.asarray(sched_of, np.int64).reshape(-1)
    off = sched.step_offsets
    if (so < -1).any() or (so >= sched.n_sched).any():
        return SCHEDULE_FAULTS[1]
    for r in range(sched.n_sched):
        if off[r, 0] < 0:
            return SCHEDULE_FAULTS[2]
        if (np.diff(off[r]) < 0).any():
            return SCHEDULE_FAULTS[3]
        if off[r, -1] > len(sched.msgs):
            return SCHEDULE_FAULTS[4]
    return None


def _flag_bits(loop, clear_step_counters):
    return (SCHEDULE_LOOP if loop else 0) | (SCHEDULE_CLEAR_STEP_COUNTERS if clear_step_counters else 0)


def save_schedule(path, sched, market_schedule=None, loop=False, clear_step_counters=False):
    """a PackedSchedule (+ the per-market row table and the flags, when given) as one .npz"""
    arrs = {"step_offsets": sched.step_offsets, "msgs": sched.msgs.view(np.uint8).reshape(-1, 16), "flags": np.array([_flag_bits(loop, clear_step_counters)], np.int64)}
    if market_schedule is not None:
        arrs["market_schedule"] = np.ascontiguousarray(np.asarray(market_schedule, np.int32))
    with open(path, "wb") as fh:
        np.savez(fh, **arrs)


def load_schedule(path):
    """-> (PackedSchedule, market_schedule int32 [N] or None, loop, clear_step_counters)"""
    with np.load(path) as z:
        sched = PackedSchedule(z["step_offsets"], z["msgs"].reshape(-1).view(MSG_DTYPE))
        ms = z["market_schedule"].astype(np.int32) if "market_schedule" in z.files else None
        flags = int(z["flags"][0])
    if flags & ~(SCHEDULE_LOOP | SCHEDULE_CLEAR_STEP_COUNTERS):
        raise ValueError(f"{path}: unknown schedule flag bits {flags:#x}")
    return sched, ms, bool(flags & SCHEDULE_LOOP), bool(flags & SCHEDULE_CLEAR_STEP_COUNTERS)


def schedule_digest(sched, sched_of, loop=False, clear_step_counters=False):
    """sha256 (hex) over the packed arrays, the per-market row table and the flags: what a training checkpoint keeps of the schedule it ran with"""
    import hashlib
    h = hashlib.sha256()
    for a in (np.array(sched.step_offsets.shape, np.int64), sched.step_offsets, np.array([len(sched.msgs)], np.int64), sched.msgs.view(np.uint8),
              np.ascontiguousarray(np.asarray(sched_of, np.int32)), np.array([_flag_bits(loop, clear_step_counters)], np.int64)):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
