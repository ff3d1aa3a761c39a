"""The depth tape on the host: the record layout of include/cda.h cda_depth_head / cda_depth_level as a numpy dtype, and the SPECIFICATION, in plain numpy, of
what the device does with it - a record from the book's ladders (record_from_levels) and the three book-shape reductions of CDAVecEnv.depth_profile /
depth_imbalance / depth_ofi (profile_from_records, imbalance_from_records, ofi_from_records) - with the plain sum that pools them (pool), the ratios a person
reads (summary) and an .npz container.  The device results equal these word for word, int64 wrap included.  The episode rule is the quote tape's: roll, record
and span are quotes.py's own functions.  No device code here: importable without a GPU.

A record is the Level-2 ladder of one market's book as the agents' orders of step t meet it: 1 + levels words of four int32.  Word 0 = (step, flags, bid_levels,
ask_levels); word 1 + l = (bid_price, bid_volume, ask_price, ask_volume) of level l, best first.  Rows at or beyond a side's count are zero; a volume beyond
INT32_MAX stores INT32_MAX and sets the saturated bit; a side with more than `levels` levels sets its more bit."""
import numpy as np

from .quotes import CAP_MAX, INT32_MAX, META_FIELDS, PARTIAL, PREV_PARTIAL, meta_from_words, new_meta, record, roll, span  # noqa: F401  (the episode rule: ONE statement)
from .stylised import MAX_BARS, MAX_HIST_HALF, _bar_steps, _lags, n_points  # noqa: F401  (lags, bars and points are the stylised-facts report's)

MAX_LEVELS = 16                                                  # include/cda.h CDA_DEPTH_MAX_LEVELS
MAX_DIST = 256                                                   # CDA_DEPTH_MAX_DIST
MAX_DEPTHS = 4                                                   # CDA_DEPTH_MAX_DEPTHS
BID, ASK, SATURATED, BID_MORE, ASK_MORE = 1, 2, 4, 8, 16         # bits of `flags` (CDA_DEPTH_*)
PROFILE, IMBALANCE, OFI = 0, 1, 2                                # cda_depth_check_host's kinds

PROFILE_FIELDS = ("steps", "two_sided", "bid_more", "ask_more", "saturated", "bid_levels", "ask_levels", "zero")
LEVEL_FIELDS = ("steps", "volume", "distance")
IMBALANCE_FIELDS = ("steps", "two_sided", "diff", "sum")
RESPONSE_FIELDS = ("n", "r", "r2", "up", "down")
OFI_FIELDS = ("pairs", "bars_kept", "bars_excluded", "saturated")
OFI_LAG_FIELDS = ("n", "q", "r", "qr", "qq", "rr")


def _levels(levels):
    L = int(levels)
    if not 1 <= L <= MAX_LEVELS:
        raise ValueError(f"levels must be in 1 .. {MAX_LEVELS}, got {levels}")
    return L


def record_words(levels):
    """int32 words of a record of `levels` levels"""
    return 4 * (1 + _levels(levels))


def record_dtype(levels):
    """one step's record as a structured dtype: step, flags, bid_levels, ask_levels, level = [levels] of (bid_price, bid_volume, ask_price, ask_volume)"""
    level = np.dtype([("bid_price", "<i4"), ("bid_volume", "<i4"), ("ask_price", "<i4"), ("ask_volume", "<i4")])
    dt = np.dtype([("step", "<i4"), ("flags", "<i4"), ("bid_levels", "<i4"), ("ask_levels", "<i4"), ("level", level, (_levels(levels),))])
    assert dt.itemsize == 4 * record_words(levels)
    return dt


def as_rows(rows, levels):
    """int32 [K, (1 + levels) * 4] host array of anything that holds depth records (a device tensor, a structured array, a list of rows)"""
    w = record_words(levels)
    if hasattr(rows, "detach"):
        rows = rows.detach().cpu().numpy()
    rows = np.asarray(rows)
    if rows.dtype.names:
        rows = np.ascontiguousarray(rows).view(np.int32).reshape(-1, w)
    if rows.size == 0:
        return np.zeros((0, w), np.int32)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if rows.shape == (w,):                                         # (one record)
        rows = rows.reshape(1, w)
    if rows.ndim != 2 or rows.shape[1] != w:
        raise ValueError(f"depth rows of {levels} levels must have shape [K, {w}], got {rows.shape}")
    return rows


def as_depth(rows, levels):
    """structured view (record_dtype(levels)) of int32 [K, (1 + levels) * 4] rows: d['bid_levels'], d['level']['ask_volume'][:, 2], ..."""
    return as_rows(rows, levels).view(record_dtype(levels)).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- a record
def record_from_levels(step, bid_rows, ask_rows, levels):
    """One record from the ladders book.levels_from_orders returns with levels + 1 rows per side (int64 [levels + 1, 3] = price, volume, orders per level, best
    first; rows past the side's level count are zero) - the extra row decides the more bit: int32 [(1 + levels) * 4].  What the recorder stores for a market whose
    book stands like that ahead of step `step`."""
    L = _levels(levels)
    out = np.zeros((1 + L, 4), np.int64)
    out[0, 0] = int(step)
    for sd, rows in enumerate((bid_rows, ask_rows)):
        lv = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        if len(lv) < L + 1:
            raise ValueError(f"record_from_levels needs levels + 1 = {L + 1} rows per side, got {len(lv)}")
        have = int((lv[:, 2] > 0).sum())                           # (levels are dense from the best on)
        n = min(have, L)
        out[0, 2 + sd] = n
        if n:
            out[0, 1] |= BID << sd
        if have > L:
            out[0, 1] |= BID_MORE << sd
        for l in range(n):
            v = int(lv[l, 1])
            if v > INT32_MAX:
                v = INT32_MAX
                out[0, 1] |= SATURATED
            out[1 + l, 2 * sd], out[1 + l, 2 * sd + 1] = lv[l, 0], v
    return out.reshape(-1).astype(np.int32)


def record_from_orders(step, bids, asks, levels):
    """the same from the two sides' order rows (get_book(): [n, 5] in queue order)"""
    from .book import levels_from_orders
    return record_from_levels(step, levels_from_orders(bids, _levels(levels) + 1), levels_from_orders(asks, _levels(levels) + 1), levels)


def _parts(rows, levels):
    """(head int64 [K, 4], level int64 [K, L, 4], two-sided bool [K], m2 int64 [K]) of one market's held rows; the steps must be consecutive"""
    L = _levels(levels)
    r = as_rows(rows, L).astype(np.int64).reshape(-1, 1 + L, 4)
    head, lev = r[:, 0], r[:, 1:]
    if len(r) and not np.array_equal(head[:, 0], head[0, 0] + np.arange(len(r))):
        raise ValueError("the depth rows are not the consecutive steps of one episode")
    return head, lev, (head[:, 1] & 3) == 3, lev[:, 0, 0] + lev[:, 0, 2]


# ---------------------------------------------------------------------------------------------------------------- the shape of the book
def profile_from_records(rows, levels, max_dist, tick=1):
    """The average shape of ONE market's held records of an episode (rows oldest first) -> (base int64 [8], levels int64 [2, L, 3], shape int64 [2, max_dist + 1]).
    What CDAVecEnv.depth_profile computes on the device, and its specification.  base: PROFILE_FIELDS - held steps, two-sided steps, bid-more and ask-more steps,
    saturated steps, the sums of bid_levels and of ask_levels, 0.  levels[side, l]: over the records where level l of the side exists - steps, the sum of its volume,
    the sum of its distance d = |price_l - price_0| / tick from the same side's best.  shape[side, min(d, max_dist)] += volume: the last bin holds the clipped mass."""
    L, md, tick = _levels(levels), int(max_dist), int(tick)
    if not 1 <= md <= MAX_DIST:
        raise ValueError(f"max_dist must be in 1 .. {MAX_DIST}, got {max_dist}")
    head, lev, two, _ = _parts(rows, L)
    base, per, shape = np.zeros(8, np.int64), np.zeros((2, L, 3), np.int64), np.zeros((2, md + 1), np.int64)
    base[:7] = len(head), two.sum(), ((head[:, 1] & BID_MORE) != 0).sum(), ((head[:, 1] & ASK_MORE) != 0).sum(), ((head[:, 1] & SATURATED) != 0).sum(), \
        head[:, 2].sum(), head[:, 3].sum()
    for sd in range(2):
        for l in range(L):
            on = head[:, 2 + sd] > l
            d = np.abs(lev[on, l, 2 * sd] - lev[on, 0, 2 * sd]) // tick
            v = lev[on, l, 2 * sd + 1]
            per[sd, l] = on.sum(), v.sum(), d.sum()
            np.add.at(shape[sd], np.minimum(d, md), v)
    return base, per, shape


# ---------------------------------------------------------------------------------------------------------------- imbalance and the next mid move
def imbalance_bin(b, a, half):
    """the bin of bid volume b against ask volume a (b + a > 0): floor(2 b half / (b + a)) in 0 .. 2 half - 1 (b == a: bin `half`)"""
    return min(2 * int(b) * int(half) // (int(b) + int(a)), 2 * int(half) - 1)


def imbalance_from_records(rows, levels, lags, k, half):
    """The response curve of ONE market's held records -> (resp int64 [n_lags, 2 half, 5], base int64 [4]).  What CDAVecEnv.depth_imbalance computes on the device, and
    its specification.  B, A = the bid / ask volume of the first k levels (absent levels add 0); over the two-sided records the bin is imbalance_bin(B, A, half).
    resp[lag, bin]: RESPONSE_FIELDS over the steps s whose record is two-sided and whose r = m2(s + lag) - m2(s) is defined (the record of s + lag held and
    two-sided) - n, sum r, sum r^2, up, down.  base: IMBALANCE_FIELDS - held steps, two-sided steps, the sums of B - A and of B + A over the two-sided steps."""
    L, lg, k, half = _levels(levels), _lags(lags, 1), int(k), int(half)
    if not 1 <= k <= L or not 1 <= half <= MAX_HIST_HALF:
        raise ValueError(f"k must be in 1 .. {L} and half in 1 .. {MAX_HIST_HALF}, got {k}, {half}")
    head, lev, two, m2 = _parts(rows, L)
    B, A = lev[:, :k, 1].sum(axis=1), lev[:, :k, 3].sum(axis=1)
    resp, base = np.zeros((len(lg), 2 * half, 5), np.int64), np.zeros(4, np.int64)
    base[:] = len(head), two.sum(), (B - A)[two].sum(), (B + A)[two].sum()
    for s in np.flatnonzero(two):
        b = imbalance_bin(B[s], A[s], half)
        for h, lag in enumerate(lg):
            if s + lag < len(head) and two[s + lag]:
                r = m2[s + lag] - m2[s]
                resp[h, b] += np.array([1, r, r * r, r > 0, r < 0], np.int64)
    return resp, base


# ---------------------------------------------------------------------------------------------------------------- order-flow imbalance
def ofi_terms(prev, cur, levels):
    """e_m(s), m = 0 .. levels - 1, of two consecutive records (int32 rows): int64 [levels].  Per level the bid side adds +q_bid of `cur` where the bid price rose or
    stayed and -q_bid of `prev` where it fell or stayed; the ask side is the mirror.  An absent bid level reads as (0, 0), an absent ask level as (INT32_MAX, 0):
    a level that appears or vanishes contributes exactly its volume, with the right sign."""
    L = _levels(levels)
    p, c = (np.asarray(x, np.int64).reshape(1 + L, 4) for x in (prev, cur))
    m = np.arange(L)
    pb, qb, pbv, qbv = c[1:, 0], c[1:, 1], p[1:, 0], p[1:, 1]
    pa, pav = np.where(m < c[0, 3], c[1:, 2], INT32_MAX), np.where(m < p[0, 3], p[1:, 2], INT32_MAX)
    qa, qav = c[1:, 3], p[1:, 3]
    return (pb >= pbv) * qb - (pb <= pbv) * qbv - (pa <= pav) * qa + (pa >= pav) * qav


def ofi_from_records(rows, levels, lags, bar_steps, depths, head_lost=False):
    """Multi-level order-flow imbalance against returns, bar by bar, of ONE market's held records -> (lagged int64 [n_depths, n_lags, 6], base int64 [4]).  What
    CDAVecEnv.depth_ofi computes on the device, and its specification.  OFI_K(s) = the sum of ofi_terms(record s - 1, record s)[:K]; bar b covers the steps
    [b bar_steps, (b + 1) bar_steps) on the episode's absolute grid and OFI_b sums the pairs whose step s lies in it, kept as an int32 word (it wraps); point p is
    step p bar_steps and r_p = m2((p + 1) bar_steps) - m2(p bar_steps), defined iff both records are held and two-sided.  head_lost (the ring has overwritten the
    episode's head, or the episode is partial: info's words 1 and 3): every bar up to and including the bar of the first held step is excluded (no record held:
    every word is zero).  lagged[depth, lag]:
    OFI_LAG_FIELDS over the kept bars b whose r_(b + lag) is defined - n, q = sum OFI_b, r, qr, qq, rr (lag 0: the contemporaneous regression).  base: OFI_FIELDS -
    pairs in the kept complete bars, those bars, bars excluded, saturated records held."""
    L, lg, bar = _levels(levels), _lags(lags, 0), _bar_steps(bar_steps)
    dp = [int(x) for x in depths]
    if not 1 <= len(dp) <= MAX_DEPTHS or min(dp) < 1 or max(dp) > L:
        raise ValueError(f"depths: 1 .. {MAX_DEPTHS} values in 1 .. {L}, got {depths!r}")
    head, lev, two, m2 = _parts(rows, L)
    r32 = as_rows(rows, L)
    lagged, base = np.zeros((len(dp), len(lg), 6), np.int64), np.zeros(4, np.int64)
    count = len(head)
    step0 = int(head[0, 0]) if count else 0
    b_first = step0 // bar + 1 if head_lost and count else 0      # (nothing held: nothing to exclude, every word is zero)
    b_end = (step0 + count) // bar if count else 0
    base[1], base[2], base[3] = max(0, b_end - b_first), b_first, ((head[:, 1] & SATURATED) != 0).sum()
    if count == 0:
        return lagged, base
    n_bars = (step0 + count - 1) // bar + 1
    qbar = np.zeros((len(dp), n_bars), np.int64)
    for i in range(1, count):
        b = (step0 + i) // bar
        base[0] += b_first <= b < b_end
        run = np.cumsum(ofi_terms(r32[i - 1], r32[i], L))
        for j, K in enumerate(dp):
            qbar[j, b] += run[K - 1]
    qbar = qbar.astype(np.int32).astype(np.int64)                 # (a bar's word is int32 on the device: two's-complement wrap)
    lo, hi = -(-step0 // bar), (step0 + count - 1) // bar          # the held points

    def ret(p):
        if p < lo or p >= hi or not two[p * bar - step0] or not two[(p + 1) * bar - step0]:
            return None
        return int(m2[(p + 1) * bar - step0] - m2[p * bar - step0])
    for h, lag in enumerate(lg):
        for b in range(b_first, hi):
            r = ret(b + lag)
            if r is None:
                continue
            for j in range(len(dp)):
                q = np.int64(qbar[j, b])
                with np.errstate(over="ignore"):
                    lagged[j, h] += np.array([1, q, r, q * np.int64(r), q * q, np.int64(r) * np.int64(r)], np.int64)
    return lagged, base


# ---------------------------------------------------------------------------------------------------------------- folding and reading
def pool(table):
    """the sum over markets (axis 0) of any of the tables: every word is additive.  numpy arrays and torch tensors alike (a tensor stays on its device)."""
    if hasattr(table, "detach"):
        return table.sum(dim=0)
    return np.asarray(table, dtype=np.int64).sum(axis=0)


def _host(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.int64)


def _ratio(x, y):
    return float(x) / float(y) if y else None


def summary(profile=None, imbalance=None, ofi=None, lags=None, ofi_lags=None, depths=None, tick=1):
    """The ratios a person reads, from POOLED tables (pool(), or one market's rows): a dict of up to three blocks.
      profile = (base [8], levels [2, L, 3], shape [2, D + 1])  -> per side and level the mean depth (volume per step the level exists) and mean distance in ticks,
                  the normalised shape (volume share by distance; the last bin is the clipped mass) and truncation = the share of steps with a more bit.
      imbalance = (resp [n_lags, 2 half, 5], base [4])          -> per lag and bin n, the mean r (half price units) and the up / down shares; the mean imbalance.
      ofi = (lagged [n_depths, n_lags, 6], base [4])            -> per depth and lag the regression slope cov(q, r) / var(q) and its R^2, beside n.
    A ratio whose denominator is 0 is None."""
    out = {}
    if profile is not None:
        base, lev, shape = (_host(x) for x in profile)
        sides = {}
        for sd, name in enumerate(("bid", "ask")):
            tot = int(shape[sd].sum())
            sides[name] = {"mean_depth": [_ratio(v, n) for n, v, _ in lev[sd]], "mean_distance": [_ratio(d, n) for n, _, d in lev[sd]],
                           "level_share": [_ratio(n, base[0]) for n, _, _ in lev[sd]], "shape": [_ratio(v, tot) for v in shape[sd]],
                           "truncation_share": _ratio(base[2 + sd], base[0]), "mean_levels": _ratio(base[5 + sd], base[0])}
        out["profile"] = dict(sides, steps=int(base[0]), two_sided_share=_ratio(base[1], base[0]), saturated_steps=int(base[4]), tick=int(tick))
    if imbalance is not None:
        resp, base = (_host(x) for x in imbalance)
        names = list(range(resp.shape[0])) if lags is None else ["k%d" % k for k in _lags(lags, 1)]
        rows = {}
        for h, name in enumerate(names):
            rows[name] = [{"n": int(n), "mean_r": _ratio(r, n), "mean_r2": _ratio(r2, n), "up_share": _ratio(up, n), "down_share": _ratio(dn, n)}
                          for n, r, r2, up, dn in resp[h]]
        out["imbalance"] = {"steps": int(base[0]), "two_sided": int(base[1]), "mean_imbalance": _ratio(base[2], base[3]), "response": rows}
    if ofi is not None:
        lagged, base = (_host(x) for x in ofi)
        lnames = list(range(lagged.shape[1])) if ofi_lags is None else ["k%d" % k for k in _lags(ofi_lags, 0)]
        dnames = list(range(lagged.shape[0])) if depths is None else ["K%d" % int(k) for k in depths]
        rows = {}
        for j, dname in enumerate(dnames):
            rows[dname] = {}
            for h, lname in enumerate(lnames):
                n, q, r, qr, qq, rr = (float(x) for x in lagged[j, h])
                cov, vq, vr = (n * qr - q * r, n * qq - q * q, n * rr - r * r) if n else (0.0, 0.0, 0.0)
                rows[dname][lname] = {"n": int(n), "slope": _ratio(cov, vq), "r_squared": _ratio(cov * cov, vq * vr)}
        out["ofi"] = {"pairs": int(base[0]), "bars_kept": int(base[1]), "bars_excluded": int(base[2]), "saturated_records": int(base[3]), "regression": rows}
    return out


# ---------------------------------------------------------------------------------------------------------------- container
def save(path, records, levels, counts=None, **extra):
    """records i32 [N, K, (1 + levels) * 4] (or [K, ...]) as CDAVecEnv.depth_series returns them (+ counts i32 [N]: the rows of every market that are records; + any
    further arrays: info, tables, module ids ...) -> .npz"""
    rec = records.detach().cpu().numpy() if hasattr(records, "detach") else np.asarray(records)
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    if rec.ndim not in (2, 3) or rec.shape[-1] != record_words(levels):
        raise ValueError(f"depth records of {levels} levels must have shape [N, K, {record_words(levels)}] or [K, {record_words(levels)}], got {rec.shape}")
    data = {"records": rec, "levels": np.int32(levels)}
    if counts is not None:
        data["counts"] = np.asarray(counts.detach().cpu().numpy() if hasattr(counts, "detach") else counts, dtype=np.int32)
    for k, v in extra.items():
        data[k] = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    np.savez_compressed(path, **data)


def load(path):
    """the arrays save wrote, as a dict (records as int32 [..., (1 + levels) * 4]; as_depth(rows, int(z['levels'])) gives the named view of one market's rows)"""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
