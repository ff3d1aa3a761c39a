"""The trade tape on the host: the record layout of include/cda.h cda_tape_record as a numpy dtype, the reference's transaction_record dicts
built from it, an .npz container, and the two reductions of CDAVecEnv.tape_bars / tape_flows stated in plain numpy for tapes that are already on the host
(bars_from_records, flows_from_records), and the execution report of CDAVecEnv.tape_exec - per-agent inventory, turnover and mark-outs - with its specification
(exec_from_records), its fold over a league's modules (exec_by_module) and the ratios a person reads (exec_summary).  No device code here but flows_by_module and
exec_by_module (torch, on whatever device the tables are): CDAVecEnv.enable_tape / drain_tape / tape_last produce the int32 [K, 8] rows."""
from decimal import Decimal

import numpy as np

TAPE_WORDS = 8
# one fill = eight int32 words (cda_tape_record)
RECORD_DTYPE = np.dtype([("time", "<i4"), ("price", "<i4"), ("quantity", "<i4"), ("counter_id", "<i4"), ("counter_order_id", "<i4"),
                         ("counter_left", "<i4"), ("init_id", "<i4"), ("sides_step", "<i4")])
assert RECORD_DTYPE.itemsize == 4 * TAPE_WORDS
FIELDS = RECORD_DTYPE.names
BAR_WORDS = 12
# one bar = twelve int32 words (cda_tape_bar)
BAR_DTYPE = np.dtype([("open", "<i4"), ("high", "<i4"), ("low", "<i4"), ("close", "<i4"), ("n_trades", "<i4"), ("n_self", "<i4"),
                      ("volume", "<i8"), ("buy_volume", "<i8"), ("notional", "<i8")])
assert BAR_DTYPE.itemsize == 4 * BAR_WORDS
SIDES = ("bid", "ask")


def as_rows(rows):
    """int32 [K, 8] host array of anything that holds records (a device tensor, a structured array, a list of rows)"""
    if hasattr(rows, "detach"):
        rows = rows.detach().cpu().numpy()
    rows = np.asarray(rows)
    if rows.dtype == RECORD_DTYPE:
        rows = rows.view(np.int32).reshape(-1, TAPE_WORDS)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if rows.ndim != 2 or rows.shape[1] != TAPE_WORDS:
        raise ValueError(f"tape rows must have shape [K, {TAPE_WORDS}], got {rows.shape}")
    return rows


def as_records(rows):
    """structured view (RECORD_DTYPE) of int32 [K, 8] rows: rec['price'], rec['quantity'], ..."""
    return as_rows(rows).view(RECORD_DTYPE).reshape(-1)


def counter_side(rows):
    return as_rows(rows)[:, 7] & 1


def init_side(rows):
    return (as_rows(rows)[:, 7] >> 1) & 1


def step_index(rows):
    """the env step t of the episode in which the fill happened"""
    return as_rows(rows)[:, 7] >> 2


def is_self_trade(rows):
    r = as_rows(rows)
    return r[:, 3] == r[:, 6]


def pack_sides_step(counter_side_, init_side_, step):
    return (np.asarray(step, dtype=np.int64) << 2 | np.asarray(init_side_, dtype=np.int64) << 1 | np.asarray(counter_side_, dtype=np.int64)).astype(np.int32)


def to_reference_records(rows):
    """The reference's transaction_record dicts (orderbook.py:108-140), one per row, with its value types: the book holds prices and quantities as Decimal, a fully
    consumed resting order leaves new_book_quantity None, the initiating party has neither order id nor left-over.  Nothing is rescaled: the device holds a price
    as the book does, in price units (an integer in this build's domain), whatever the tick."""
    out = []
    for time, price, qty, cid, coid, left, iid, ss in as_rows(rows).tolist():
        out.append({"timestamp": time, "price": Decimal(price), "quantity": Decimal(qty), "time": time,
                    "counter_party": {"ID": cid, "side": SIDES[ss & 1], "order_id": coid, "new_book_quantity": None if left < 0 else Decimal(left)},
                    "init_party": {"ID": iid, "side": SIDES[(ss >> 1) & 1], "order_id": None, "new_book_quantity": None}})
    return out


def save_tape(path, records, offsets=None, dropped=None, **extra):
    """records i32 [K, 8] (+ offsets i64 [N + 1] and dropped i64 [N] as drain_tape returns them, + any further arrays: market, episode, module ids ...) -> .npz.
    `market` (i32 [K]: the market of every row) is derived from offsets when it is not given."""
    rows = as_rows(records)
    data = {"records": rows, "fields": np.array(FIELDS)}
    if offsets is not None:
        off = np.asarray(offsets.detach().cpu().numpy() if hasattr(offsets, "detach") else offsets, dtype=np.int64)
        data["offsets"] = off
        if "market" not in extra:
            data["market"] = np.repeat(np.arange(len(off) - 1, dtype=np.int32), np.diff(off))
    if dropped is not None:
        data["dropped"] = np.asarray(dropped.detach().cpu().numpy() if hasattr(dropped, "detach") else dropped, dtype=np.int64)
    for k, v in extra.items():
        data[k] = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    np.savez_compressed(path, **data)


def load_tape(path):
    """the arrays save_tape wrote, as a dict (records as int32 [K, 8]; as_records() gives the named view)"""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def as_bars(bars):
    """structured view (BAR_DTYPE) of int32 [..., 12] bars as CDAVecEnv.tape_bars returns them: bars['open'], bars['volume'], ... of shape [...]"""
    if hasattr(bars, "detach"):
        bars = bars.detach().cpu().numpy()
    bars = np.asarray(bars)
    if bars.dtype == BAR_DTYPE:
        return bars
    bars = np.ascontiguousarray(bars, dtype=np.int32)
    if bars.ndim < 1 or bars.shape[-1] != BAR_WORDS:
        raise ValueError(f"bars must have shape [..., {BAR_WORDS}], got {bars.shape}")
    return bars.view(BAR_DTYPE).reshape(bars.shape[:-1])


def bars_from_records(rows, bar_steps, n_bars):
    """Price / volume bars of ONE market's episode (rows in tape order): bar b covers the fills of env steps [b * bar_steps, (b + 1) * bar_steps); open / close are
    the first / last of them, a bar without fills is all zeros.  -> (BAR_DTYPE [n_bars], number of rows whose bar index was >= n_bars and that were left out).
    What CDAVecEnv.tape_bars computes on the device."""
    r = as_rows(rows).astype(np.int64)
    bar_steps, n_bars = int(bar_steps), int(n_bars)
    if bar_steps < 1 or n_bars < 1:
        raise ValueError("bar_steps and n_bars must be >= 1")
    b = (r[:, 7] >> 2) // bar_steps
    keep = b < n_bars
    out = np.zeros(n_bars, BAR_DTYPE)
    r, b = r[keep], b[keep]
    for k in np.unique(b):
        x = r[b == k]
        price, qty = x[:, 1], x[:, 2]
        out[k] = (price[0], price.max(), price.min(), price[-1], len(x), int((x[:, 3] == x[:, 6]).sum()), qty.sum(), qty[((x[:, 7] >> 1) & 1) == 0].sum(),
                  (price * qty).sum())
    return out, int((~keep).sum())


def flows_from_records(rows, num_agents):
    """Who traded with whom: int64 [A, A, 3], [init_id, counter_id] = (quantity, notional = price x quantity, fills) over ONE market's rows; the diagonal holds
    the self-trades.  What CDAVecEnv.tape_flows computes on the device."""
    r = as_rows(rows).astype(np.int64)
    a = int(num_agents)
    out = np.zeros((a, a, 3), np.int64)
    if len(r) and (r[:, [3, 6]].min() < 0 or r[:, [3, 6]].max() >= a):
        raise ValueError(f"an agent id of the tape is outside 0 .. {a - 1}")
    np.add.at(out, (r[:, 6], r[:, 3]), np.stack([r[:, 2], r[:, 1] * r[:, 2], np.ones(len(r), np.int64)], axis=1))
    return out


def flows_by_module(flows, slot_module, n_modules):
    """Per-market flow matrices summed into one module x module table through a league's slot -> module map: flows i64 [N, A, A, 3] (CDAVecEnv.tape_flows),
    slot_module integer [N, A] (the module that played slot a of market i, 0 .. n_modules - 1) -> i64 [n_modules, n_modules, 3], [initiator's module,
    counterparty's module].  torch tensors, on the device the flows are on (one index_add_)."""
    import torch
    n, a = flows.shape[0], flows.shape[1]
    if tuple(flows.shape) != (n, a, a, 3) or tuple(slot_module.shape) != (n, a):
        raise ValueError(f"flows must be [N, A, A, 3] and slot_module [N, A], got {tuple(flows.shape)} and {tuple(slot_module.shape)}")
    mod = slot_module.to(device=flows.device, dtype=torch.int64)
    if mod.numel() and (int(mod.min()) < 0 or int(mod.max()) >= int(n_modules)):
        raise ValueError(f"a module id is outside 0 .. {int(n_modules) - 1}")
    cell = (mod[:, :, None] * int(n_modules) + mod[:, None, :]).reshape(-1)                  # [N * A * A]: initiator's module x counterparty's module
    out = torch.zeros((int(n_modules) * int(n_modules), 3), dtype=torch.int64, device=flows.device)
    out.index_add_(0, cell, flows.reshape(-1, 3).to(torch.int64))
    return out.reshape(int(n_modules), int(n_modules), 3)


# ---------------------------------------------------------------------------------------------------------------- the execution report (cda_tape_exec)
# the sixteen int64 words per agent of CDAVecEnv.tape_exec's `stats` (include/cda.h CDA_TAPE_STAT_WORDS)
STAT_FIELDS = ("buy_qty", "sell_qty", "buy_notional", "sell_notional", "maker_qty", "maker_fills", "taker_qty", "taker_fills", "self_qty", "self_fills",
               "final_pos", "max_long", "max_short", "abs_pos_steps", "first_step", "last_step")
STAT_WORDS = len(STAT_FIELDS)
STAT = {name: i for i, name in enumerate(STAT_FIELDS)}
STAT_ADDITIVE = STAT_FIELDS[:10] + ("final_pos", "abs_pos_steps")      # what a fold over markets sums; max_long / last_step take the max, max_short / first_step the min
MARKOUT_FIELDS = ("pnl", "qty", "fills", "open_fills")                  # the four int64 words per (agent, horizon, role)
MARKOUT_ROLES = ("maker", "taker")
MAX_HORIZONS = 8


def _horizons(horizons):
    hz = [int(k) for k in (horizons if hasattr(horizons, "__iter__") else (horizons,))]
    if not 1 <= len(hz) <= MAX_HORIZONS or min(hz) < 0 or max(hz) >= 2 ** 31:
        raise ValueError(f"horizons: 1 .. {MAX_HORIZONS} step counts >= 0, got {horizons!r}")
    return hz


def exec_from_records(rows, num_agents, horizons):
    """The execution report of ONE market's episode (rows in tape order, as held): (stats int64 [A, STAT_WORDS], markouts int64 [A, H, 2, 4]).  What
    CDAVecEnv.tape_exec computes on the device, and its specification.

    A record r has a step s(r) = sides_step >> 2, a price p, a quantity q and two parties: counter_id (role 0, maker) and init_id (role 1, taker), each with a side:
    0 = bid (it bought, sign +1), 1 = ask (it sold, sign -1).  A self-trade (init_id == counter_id) moves no position and counts in self_qty / self_fills only.
    S_last = the step of the last row.
    stats (STAT_FIELDS): buy / sell quantity and notional (p x q) over both roles; quantity and fills by role; the agent's running position (0 before its first row
    here) at the end, its largest (max_long >= 0) and most negative (max_short <= 0) value; abs_pos_steps = the sum over the steps 0 .. S_last of |position at the
    end of the step|; first_step / last_step of its non-self fills (-1 without any).
    markouts[a, h, role] (MARKOUT_FIELDS): over a's non-self fills in that role with s + k_h <= S_last, the sum of sign x (mark(s + k_h) - p) x q, of q, and their
    number; then the number of fills with s + k_h > S_last (open: the episode ended, or has not run, that far).  mark(t) = the price of the last row whose step is
    <= t (the last print, the reference's mark_to_mkt)."""
    r = as_rows(rows).astype(np.int64)
    a, hz = int(num_agents), _horizons(horizons)
    stats = np.zeros((a, STAT_WORDS), np.int64)
    stats[:, STAT["first_step"]:] = -1
    marks = np.zeros((a, len(hz), 2, 4), np.int64)
    if len(r) == 0:
        return stats, marks
    if r[:, [3, 6]].min() < 0 or r[:, [3, 6]].max() >= a:
        raise ValueError(f"an agent id of the tape is outside 0 .. {a - 1}")
    step, price, qty = r[:, 7] >> 2, r[:, 1], r[:, 2]
    if (np.diff(step) < 0).any():
        raise ValueError("the step index decreases: these rows are not one episode in tape order")
    s_last = int(step[-1])
    own = r[:, 3] == r[:, 6]
    trade = ~own
    np.add.at(stats[:, STAT["self_qty"]], r[own, 6], qty[own])
    np.add.at(stats[:, STAT["self_fills"]], r[own, 6], 1)
    ones = np.ones(len(r), np.int64)
    parties = ((r[:, 3], r[:, 7] & 1, 0), (r[:, 6], (r[:, 7] >> 1) & 1, 1))              # (agent, side, role) of every row
    for who, side, role in parties:
        for sd, word in ((0, "buy"), (1, "sell")):
            k = trade & (side == sd)
            np.add.at(stats[:, STAT[word + "_qty"]], who[k], qty[k])
            np.add.at(stats[:, STAT[word + "_notional"]], who[k], (price * qty)[k])
        np.add.at(stats[:, STAT[MARKOUT_ROLES[role] + "_qty"]], who[trade], qty[trade])
        np.add.at(stats[:, STAT[MARKOUT_ROLES[role] + "_fills"]], who[trade], ones[trade])
    # the path: an agent's position is constant between its own fills, so |position after a fill| weighs the steps up to its next fill (none when that lies in
    # the same step), the last one up to and including S_last
    for i in range(a):
        k = trade & ((r[:, 3] == i) | (r[:, 6] == i))
        if not k.any():
            continue
        side = np.where(r[k, 6] == i, (r[k, 7] >> 1) & 1, r[k, 7] & 1)
        pos = np.cumsum(np.where(side == 0, qty[k], -qty[k]))
        s = step[k]
        stats[i, STAT["final_pos"]] = pos[-1]
        stats[i, STAT["max_long"]] = max(0, int(pos.max()))
        stats[i, STAT["max_short"]] = min(0, int(pos.min()))
        stats[i, STAT["abs_pos_steps"]] = int((np.abs(pos) * (np.append(s[1:], s_last + 1) - s)).sum())
        stats[i, STAT["first_step"]], stats[i, STAT["last_step"]] = s[0], s[-1]
    for h, k in enumerate(hz):
        due = step + k
        scored = trade & (due <= s_last)
        mark = price[np.searchsorted(step, due, side="right") - 1]                       # the last row with step <= s + k (the row itself at the least)
        value = (mark - price) * qty
        for who, side, role in parties:
            np.add.at(marks[:, h, role, 0], who[scored], np.where(side == 0, value, -value)[scored])
            np.add.at(marks[:, h, role, 1], who[scored], qty[scored])
            np.add.at(marks[:, h, role, 2], who[scored], ones[scored])
            np.add.at(marks[:, h, role, 3], who[trade & ~scored], ones[trade & ~scored])
    return stats, marks


def exec_by_module(stats, markouts, slot_module, n_modules):
    """Per-market execution tables folded into one row per module through a league's slot -> module map, as flows_by_module folds the flows: stats i64 [N, A,
    STAT_WORDS] and markouts i64 [N, A, H, 2, 4] (CDAVecEnv.tape_exec), slot_module integer [N, A] -> (i64 [n_modules, STAT_WORDS], i64 [n_modules, H, 2, 4]).
    The additive words (STAT_ADDITIVE, every mark-out word) are summed; max_long and last_step take the largest, max_short and first_step the smallest value of
    the module's slots (first_step over the slots that traded; -1 when none did).  torch tensors, on the device the tables are on."""
    import torch
    n, a = stats.shape[0], stats.shape[1]
    if tuple(stats.shape) != (n, a, STAT_WORDS) or markouts.dim() != 5 or tuple(markouts.shape[:2]) != (n, a) or tuple(markouts.shape[3:]) != (2, 4) or \
            tuple(slot_module.shape) != (n, a):
        raise ValueError(f"stats must be [N, A, {STAT_WORDS}], markouts [N, A, H, 2, 4] and slot_module [N, A], got {tuple(stats.shape)}, {tuple(markouts.shape)} "
                         f"and {tuple(slot_module.shape)}")
    m = int(n_modules)
    mod = slot_module.to(device=stats.device, dtype=torch.int64).reshape(-1)
    if mod.numel() and (int(mod.min()) < 0 or int(mod.max()) >= m):
        raise ValueError(f"a module id is outside 0 .. {m - 1}")
    s = stats.reshape(-1, STAT_WORDS).to(torch.int64)
    out = torch.zeros((m, STAT_WORDS), dtype=torch.int64, device=stats.device)
    add = [STAT[f] for f in STAT_ADDITIVE]
    out[:, add] = torch.zeros((m, len(add)), dtype=torch.int64, device=stats.device).index_add_(0, mod, s[:, add])
    big = torch.iinfo(torch.int64).max
    index = mod[:, None]
    out[:, STAT["max_long"]] = torch.zeros((m, 1), dtype=torch.int64, device=stats.device).scatter_reduce_(0, index, s[:, [STAT["max_long"]]], "amax")[:, 0]
    out[:, STAT["max_short"]] = torch.zeros((m, 1), dtype=torch.int64, device=stats.device).scatter_reduce_(0, index, s[:, [STAT["max_short"]]], "amin")[:, 0]
    out[:, STAT["last_step"]] = torch.full((m, 1), -1, dtype=torch.int64, device=stats.device).scatter_reduce_(0, index, s[:, [STAT["last_step"]]], "amax")[:, 0]
    first = s[:, [STAT["first_step"]]]
    first = torch.full((m, 1), big, dtype=torch.int64, device=stats.device).scatter_reduce_(0, index, torch.where(first < 0, torch.full_like(first, big), first), "amin")[:, 0]
    out[:, STAT["first_step"]] = torch.where(first == big, torch.full_like(first, -1), first)
    h = markouts.shape[2]
    marks = torch.zeros((m, h * 8), dtype=torch.int64, device=stats.device).index_add_(0, mod, markouts.reshape(-1, h * 8).to(torch.int64))
    return out, marks.reshape(m, h, 2, 4)


def _ratio(x, y):
    return float(x) / float(y) if y else None


def exec_summary(stats, markouts, horizons=None, steps=None):
    """The ratios a person reads, from the integers of ONE row: stats [STAT_WORDS] and markouts [H, 2, 4] of an agent (exec_from_records, CDAEnv.tape_exec) or of a
    module (exec_by_module) -> a dict of floats and ints.  A ratio whose denominator is 0 is None.  buy_vwap / sell_vwap = notional / quantity; turnover = bought +
    sold quantity; maker_share = maker quantity over the row's own non-self quantity; mean_abs_position = abs_pos_steps / steps (`steps`: the position-steps the row
    covers - an episode's S_last + 1 for one agent, the sum of that over a module's slots and episodes; default last_step + 1, which is exact only for a single agent
    that traded in the episode's last step); markouts: per horizon (named by `horizons` when given) and role pnl_per_share = pnl / qty over the SCORED fills, with
    the scored quantity and fills and the number of open fills beside it - open fills are reported, never hidden, and coverage = scored / (scored + open)."""
    sv = np.asarray(stats.detach().cpu().numpy() if hasattr(stats, "detach") else stats, dtype=np.int64)
    mk = np.asarray(markouts.detach().cpu().numpy() if hasattr(markouts, "detach") else markouts, dtype=np.int64)
    if sv.shape != (STAT_WORDS,) or mk.ndim != 3 or mk.shape[1:] != (2, 4):
        raise ValueError(f"exec_summary takes one row: stats [{STAT_WORDS}] and markouts [H, 2, 4], got {sv.shape} and {mk.shape}")
    s = [int(x) for x in sv]
    hz = list(range(mk.shape[0])) if horizons is None else _horizons(horizons)
    if len(hz) != mk.shape[0]:
        raise ValueError(f"{len(hz)} horizons named for {mk.shape[0]} mark-out rows")
    g = {f: s[i] for i, f in enumerate(STAT_FIELDS)}
    own = g["maker_qty"] + g["taker_qty"]
    span = g["last_step"] + 1 if steps is None else int(steps)
    out = {"buy_qty": g["buy_qty"], "sell_qty": g["sell_qty"], "buy_vwap": _ratio(g["buy_notional"], g["buy_qty"]), "sell_vwap": _ratio(g["sell_notional"], g["sell_qty"]),
           "turnover": g["buy_qty"] + g["sell_qty"], "turnover_notional": g["buy_notional"] + g["sell_notional"], "fills": g["maker_fills"] + g["taker_fills"],
           "maker_share": _ratio(g["maker_qty"], own), "self_qty": g["self_qty"], "self_fills": g["self_fills"], "final_pos": g["final_pos"],
           "max_long": g["max_long"], "max_short": g["max_short"], "abs_pos_steps": g["abs_pos_steps"], "mean_abs_position": _ratio(g["abs_pos_steps"], span if span > 0 else 0),
           "first_step": g["first_step"], "last_step": g["last_step"], "markouts": {}}
    for h, k in enumerate(hz):
        row = {}
        for role, name in enumerate(MARKOUT_ROLES):
            pnl, qty, fills, opened = (int(x) for x in mk[h, role])
            row[name] = {"pnl": pnl, "qty": qty, "fills": fills, "open_fills": opened, "pnl_per_share": _ratio(pnl, qty), "coverage": _ratio(fills, fills + opened)}
        out["markouts"][("k%d" % k) if horizons is not None else h] = row
    return out
