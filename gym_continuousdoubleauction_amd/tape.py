"""The trade tape on the host: the record layout of include/cda.h cda_tape_record as a numpy dtype, the reference's transaction_record dicts
built from it, an .npz container, and the two reductions of CDAVecEnv.tape_bars / tape_flows stated in plain numpy for tapes that are already on the host
(bars_from_records, flows_from_records).  No device code here but flows_by_module (torch, on whatever device the flows are): CDAVecEnv.enable_tape / drain_tape /
tape_last produce the int32 [K, 8] rows."""
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
