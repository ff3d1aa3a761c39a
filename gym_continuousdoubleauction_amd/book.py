"""The book report on the host: the SPECIFICATION of CDAVecEnv.book_counts / book_levels / book_impact / book_agents (include/cda.h cda_book_*) in plain numpy,
on the rows get_book() and book_orders() return.  The device results equal these word for word.  No device code here: importable without a GPU.

One side of a book is an int32 [n, 5] array of (price, qty, owner, order_id, timestamp) rows in QUEUE ORDER - best price first, FIFO inside a price level -
which is the order a market order consumes it in.  Side 0 = bids, 1 = asks."""
import numpy as np

ORDER_WORDS = 5
ORDER_FIELDS = ("price", "qty", "owner", "order_id", "timestamp")
LEVEL_FIELDS = ("price", "volume", "orders")
IMPACT_FIELDS = ("filled", "notional", "last_price")
AGENT_FIELDS = ("orders", "quantity", "notional", "best_price", "worst_price", "ahead_qty")
MAX_LEVELS = 4096                # include/cda.h CDA_BOOK_MAX_LEVELS
MAX_SIZES = 16                   # include/cda.h CDA_BOOK_MAX_SIZES


def as_orders(rows):
    """int64 [n, 5] host array of one side's rows (a device tensor, an int32 array, a list of rows; an empty side may come as anything of size 0)"""
    if hasattr(rows, "detach"):
        rows = rows.detach().cpu().numpy()
    rows = np.asarray(rows)
    if rows.size == 0:
        return np.zeros((0, ORDER_WORDS), np.int64)
    if rows.ndim != 2 or rows.shape[1] != ORDER_WORDS:
        raise ValueError(f"book rows must have shape [n, {ORDER_WORDS}], got {rows.shape}")
    return rows.astype(np.int64)


def _max_levels(max_levels):
    L = int(max_levels)
    if not 1 <= L <= MAX_LEVELS:
        raise ValueError(f"max_levels must be in 1 .. {MAX_LEVELS}, got {max_levels}")
    return L


def _sizes(sizes):
    q = [int(x) for x in np.atleast_1d(np.asarray(sizes)).tolist()]
    if not 1 <= len(q) <= MAX_SIZES:
        raise ValueError(f"between 1 and {MAX_SIZES} sizes, got {len(q)}")
    if any(x < 1 or x >= 2 ** 63 for x in q):
        raise ValueError(f"sizes must be >= 1 (and fit 63 bits), got {q}")
    return q


def _level_starts(price):
    """index of the first order of every price level: a level boundary is a price change between neighbours"""
    return np.flatnonzero(np.r_[True, price[1:] != price[:-1]]) if len(price) else np.zeros(0, np.int64)


def counts_from_orders(rows):
    """int32 [2] = (resting orders, distinct price levels)"""
    r = as_orders(rows)
    return np.array([len(r), len(_level_starts(r[:, 0]))], np.int32)


def levels_from_orders(rows, max_levels):
    """the Level-2 ladder: int64 [max_levels, 3] = (price, volume, orders) per level, best first; rows past the side's level count are zero"""
    L = _max_levels(max_levels)
    r = as_orders(rows)
    out = np.zeros((L, 3), np.int64)
    start = _level_starts(r[:, 0])
    if len(start):
        k = min(L, len(start))
        out[:k, 0] = r[start, 0][:k]
        out[:k, 1] = np.add.reduceat(r[:, 1], start)[:k]
        out[:k, 2] = np.diff(np.r_[start, len(r)])[:k]
    return out


def impact_from_orders(rows, sizes):
    """what a market order of each size pays that consumes this side by price-time priority: int64 [K, 3] = (filled, notional, last_price).  filled =
    min(size, the side's quantity); notional = the sum of price x quantity over what is consumed, the last order partially; last_price = the price of the last
    order touched, 0 on an empty side.  The taker's own resting orders are part of the side (the matching loop does not skip them)."""
    q = _sizes(sizes)
    r = as_orders(rows)
    out = np.zeros((len(q), 3), np.int64)
    if len(r) == 0:
        return out
    cq, cn = np.cumsum(r[:, 1]), np.cumsum(r[:, 0] * r[:, 1])
    for k, size in enumerate(q):
        if size >= cq[-1]:
            out[k] = (cq[-1], cn[-1], r[-1, 0])
        else:
            i = int(np.searchsorted(cq, size, side="left"))       # the first order whose cumulative quantity reaches the size
            out[k] = (size, cn[i] - r[i, 0] * (cq[i] - size), r[i, 0])
    return out


def agents_from_orders(rows, num_agents):
    """every agent's resting orders on this side: int64 [A, 6] = (orders, quantity, notional, best_price, worst_price, ahead_qty); best / worst price = the
    prices of the agent's first / last own order in queue order, ahead_qty = the quantity resting strictly before its first own order; zeros for an agent
    with nothing on the side"""
    r = as_orders(rows)
    out = np.zeros((int(num_agents), 6), np.int64)
    before = np.cumsum(r[:, 1]) - r[:, 1]
    for a in range(int(num_agents)):
        own = np.flatnonzero(r[:, 2] == a)
        if len(own):
            out[a] = (len(own), r[own, 1].sum(), (r[own, 0] * r[own, 1]).sum(), r[own[0], 0], r[own[-1], 0], before[own[0]])
    return out


def report_from_books(books, num_agents, max_levels=10, sizes=(1,)):
    """`books`: one (bids, asks) pair of row arrays per market.  The four reductions stacked into the device's shapes: {'counts' i32 [n, 2, 2], 'levels' i64
    [n, 2, L, 3], 'impact' i64 [n, 2, K, 3], 'agents' i64 [n, 2, A, 6], 'orders' i32 [total, 5], 'offsets' i64 [2 n + 1]}"""
    books = [(as_orders(b), as_orders(a)) for b, a in books]
    sides = [s for pair in books for s in pair]
    n = len(books)
    L, K, A = _max_levels(max_levels), len(_sizes(sizes)), int(num_agents)
    out = {"counts": np.array([counts_from_orders(s) for s in sides], np.int32).reshape(n, 2, 2),
           "levels": np.array([levels_from_orders(s, L) for s in sides], np.int64).reshape(n, 2, L, 3),
           "impact": np.array([impact_from_orders(s, sizes) for s in sides], np.int64).reshape(n, 2, K, 3),
           "agents": np.array([agents_from_orders(s, A) for s in sides], np.int64).reshape(n, 2, A, 6),
           "offsets": np.r_[0, np.cumsum([len(s) for s in sides])].astype(np.int64)}
    out["orders"] = (np.concatenate(sides) if sides else np.zeros((0, ORDER_WORDS))).astype(np.int32).reshape(-1, ORDER_WORDS)
    return out


def split_orders(orders, offsets):
    """book_orders()'s (orders [total, 5], offsets [2 n + 1]) -> one (bids, asks) pair of int32 row arrays per market"""
    if hasattr(orders, "detach"):
        orders, offsets = orders.detach().cpu().numpy(), offsets.detach().cpu().numpy()
    orders, off = np.asarray(orders), np.asarray(offsets).astype(np.int64)
    n = (len(off) - 1) // 2
    return [(orders[off[2 * i]:off[2 * i + 1]], orders[off[2 * i + 1]:off[2 * i + 2]]) for i in range(n)]


def summary(levels, top_k=5):
    """What a person reads off a ladder (book_levels' [n, 2, L, 3], or one market's [2, L, 3]): {'best_bid', 'best_ask' i64 [n] (0 = that side is empty),
    'spread' f64 [n] = best_ask - best_bid, 'mid' f64 [n] = their mean (both nan unless both sides stand), 'imbalance' f64 [n] = (bid volume - ask volume) /
    (bid volume + ask volume) over the first top_k levels of each side (nan for an empty book)}"""
    if hasattr(levels, "detach"):
        levels = levels.detach().cpu().numpy()
    lv = np.asarray(levels).astype(np.int64)
    if lv.ndim == 3:
        lv = lv[None]
    if lv.ndim != 4 or lv.shape[1] != 2 or lv.shape[3] != 3:
        raise ValueError(f"a ladder has shape [n, 2, L, 3], got {lv.shape}")
    bid, ask = lv[:, 0, 0, 0], lv[:, 1, 0, 0]
    both = (lv[:, 0, 0, 2] > 0) & (lv[:, 1, 0, 2] > 0)
    k = max(1, min(int(top_k), lv.shape[2]))
    vb, va = lv[:, 0, :k, 1].sum(axis=1).astype(np.float64), lv[:, 1, :k, 1].sum(axis=1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        imb = np.where(vb + va > 0, (vb - va) / (vb + va), np.nan)
    return {"best_bid": bid, "best_ask": ask, "spread": np.where(both, (ask - bid).astype(np.float64), np.nan),
            "mid": np.where(both, (ask + bid) / 2.0, np.nan), "imbalance": imb}
