"""The trade tape on the host: the record layout of include/cda.h cda_tape_record as a numpy dtype, the reference's transaction_record dicts
built from it, and an .npz container.  No device code here: CDAVecEnv.enable_tape / drain_tape / tape_last produce the int32 [K, 8] rows."""
from decimal import Decimal

import numpy as np

TAPE_WORDS = 8
# one fill = eight int32 words (cda_tape_record)
RECORD_DTYPE = np.dtype([("time", "<i4"), ("price", "<i4"), ("quantity", "<i4"), ("counter_id", "<i4"), ("counter_order_id", "<i4"),
                         ("counter_left", "<i4"), ("init_id", "<i4"), ("sides_step", "<i4")])
assert RECORD_DTYPE.itemsize == 4 * TAPE_WORDS
FIELDS = RECORD_DTYPE.names
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
