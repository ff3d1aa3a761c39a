"""The quote tape on the host: the record layout of include/cda.h cda_quote_record as a numpy dtype, and the SPECIFICATION, in plain numpy, of what the device
does with it - the episode rule (roll), a record from the book's best levels (quote_from_levels), the statistics of CDAVecEnv.quote_stats (stats_from_quotes) and
the spread report of CDAVecEnv.tape_spreads (spreads_from_records) - with its fold over a league's modules (spreads_by_module), the ratios a person reads
(spread_summary) and an .npz container.  The device results equal these word for word.  No device code here but spreads_by_module (torch, on whatever device
the tables are): importable without a GPU.

A quote is the top of one market's book as the agents' orders of step t meet it: per side the best price, the summed quantity of that price level and the number
of its orders.  An absent side stores zeros; a volume or count beyond INT32_MAX stores INT32_MAX and sets the saturated bit."""
import numpy as np

from .tape import _horizons  # noqa: F401  (the spread report's horizons are the execution report's: one check, one message; MAX_HORIZONS below == tape.MAX_HORIZONS)

QUOTE_WORDS = 8
# one step's quote = eight int32 words (cda_quote_record)
QUOTE_DTYPE = np.dtype([("step", "<i4"), ("flags", "<i4"), ("bid_price", "<i4"), ("ask_price", "<i4"), ("bid_volume", "<i4"), ("ask_volume", "<i4"),
                        ("bid_orders", "<i4"), ("ask_orders", "<i4")])
assert QUOTE_DTYPE.itemsize == 4 * QUOTE_WORDS
FIELDS = QUOTE_DTYPE.names
BID, ASK, SATURATED = 1, 2, 4                                    # bits of `flags` (CDA_QUOTE_BID, CDA_QUOTE_ASK, CDA_QUOTE_SATURATED)
INT32_MAX = 2 ** 31 - 1
CAP_MAX = 1 << 20                                                # include/cda.h CDA_QUOTE_CAP_MAX

# the eight int32 words of a market's meta row (CDAVecEnv.quote_meta): n_total is the 64-bit pair of words 0 and 1
META_FIELDS = ("n_total", "n_episode", "n_prev", "first", "prev_first", "gap", "flags")
PARTIAL, PREV_PARTIAL = 1, 2                                     # bits of the meta row's flags

# the sixteen int64 words of CDAVecEnv.quote_stats (include/cda.h CDA_QUOTE_STAT_WORDS)
STAT_FIELDS = ("steps", "two_sided", "bid_only", "ask_only", "empty", "spread_sum", "spread_sq", "spread_min", "spread_max", "m2_sum", "bid_volume", "ask_volume",
               "pairs", "m2_changes", "abs_dm2", "dm2_sq")
STAT_WORDS = len(STAT_FIELDS)
STAT = {name: i for i, name in enumerate(STAT_FIELDS)}
# the six int64 words per (agent, horizon, role) of CDAVecEnv.tape_spreads
SPREAD_FIELDS = ("cost_now", "cost_later", "qty", "fills", "open", "unquoted")
SPREAD_WORDS = len(SPREAD_FIELDS)
ROLES = ("maker", "taker")
MAX_HORIZONS = 8


def as_rows(rows):
    """int32 [K, 8] host array of anything that holds quote records (a device tensor, a structured array, a list of rows)"""
    if hasattr(rows, "detach"):
        rows = rows.detach().cpu().numpy()
    rows = np.asarray(rows)
    if rows.dtype == QUOTE_DTYPE:
        rows = rows.view(np.int32).reshape(-1, QUOTE_WORDS)
    if rows.size == 0:
        return np.zeros((0, QUOTE_WORDS), np.int32)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if rows.ndim != 2 or rows.shape[1] != QUOTE_WORDS:
        raise ValueError(f"quote rows must have shape [K, {QUOTE_WORDS}], got {rows.shape}")
    return rows


def as_quotes(rows):
    """structured view (QUOTE_DTYPE) of int32 [K, 8] rows: q['bid_price'], q['ask_volume'], ..."""
    return as_rows(rows).view(QUOTE_DTYPE).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- the episode rule
def new_meta():
    return {k: 0 for k in META_FIELDS}


def roll(meta, t_step):
    """THE EPISODE RULE, a pure function of a market's meta row and its current t_step (csrc/cda_quotes.inc quote_roll): the row the recorder - and, lazily, every
    reader - works with.  The current episode holds n_episode records, of the steps first .. first + n_episode - 1.
      t_step == first + n_episode     the expected next step: nothing changes.
      t_step == 0 and n_episode > 0   the market was reset: the held episode becomes "previous", the current one starts empty.
      anything else                   a restore moved the clock: the current episode restarts at t_step, empty, partial unless t_step == 0; what it held stays in
                                      the ring as a gap between the previous episode and the new current one."""
    h, t = dict(meta), int(t_step)
    if t == h["first"] + h["n_episode"]:
        return h
    if t == 0 and h["n_episode"] > 0:
        h.update(n_prev=h["n_episode"], prev_first=h["first"], gap=0, flags=PREV_PARTIAL if h["flags"] & PARTIAL else 0, n_episode=0, first=0)
        return h
    h.update(gap=min(h["gap"] + h["n_episode"], CAP_MAX), n_episode=0, first=t, flags=(h["flags"] & PREV_PARTIAL) | (PARTIAL if t != 0 else 0))
    return h


def record(meta, t_step):
    """the meta row behind the recorder's visit at t_step (the episode not over): rolled, then one record more"""
    h = roll(meta, t_step)
    h["n_total"] += 1
    h["n_episode"] += 1
    return h


def span(meta, capacity, episode="current"):
    """What the ring of `capacity` records still holds of an episode of a ROLLED meta row, in record numbers (record j lies in slot j % capacity): a dict of start,
    count, lost (records of the episode's head that are overwritten), step0 (the step of record `start`) and partial."""
    if episode not in ("current", "previous"):
        raise ValueError(f"episode must be 'current' or 'previous', got {episode!r}")
    prev = episode == "previous"
    hi = meta["n_total"] - (meta["n_episode"] + meta["gap"] if prev else 0)
    lo = max(0, hi - (meta["n_prev"] if prev else meta["n_episode"]))
    hi = max(hi, lo)
    floor = min(max(meta["n_total"] - int(capacity), lo), hi)
    return {"start": floor, "count": hi - floor, "lost": floor - lo, "step0": (meta["prev_first"] if prev else meta["first"]) + floor - lo,
            "partial": 1 if meta["flags"] & (PREV_PARTIAL if prev else PARTIAL) else 0}


def meta_from_words(words):
    """a meta row as CDAVecEnv.quote_meta returns it (eight int32 words) -> the dict roll() and span() take"""
    w = [int(x) for x in np.asarray(words).reshape(-1)]
    if len(w) != 8:
        raise ValueError(f"a meta row has eight words, got {len(w)}")
    return {"n_total": (w[0] & 0xFFFFFFFF) | (w[1] << 32), "n_episode": w[2], "n_prev": w[3], "first": w[4], "prev_first": w[5], "gap": w[6], "flags": w[7]}


# ---------------------------------------------------------------------------------------------------------------- a record
def quote_from_levels(step, bid_levels, ask_levels):
    """One record from the ladders book.levels_from_orders returns (int64 [L, 3] = price, volume, orders per level, best first; L >= 1; an empty side is all zeros):
    int32 [8].  What the recorder stores for a market whose book stands like that ahead of step `step`."""
    out = np.zeros(QUOTE_WORDS, np.int64)
    out[0] = int(step)
    for sd, levels in enumerate((bid_levels, ask_levels)):
        lv = np.asarray(levels, dtype=np.int64).reshape(-1, 3)
        if len(lv) == 0 or lv[0, 2] <= 0:
            continue
        out[1] |= BID << sd
        out[2 + sd] = lv[0, 0]
        for word, v in ((4 + sd, int(lv[0, 1])), (6 + sd, int(lv[0, 2]))):
            if v > INT32_MAX:
                v = INT32_MAX
                out[1] |= SATURATED
            out[word] = v
    return out.astype(np.int32)


def quote_from_orders(step, bids, asks):
    """the same from the two sides' order rows (get_book(): [n, 5] in queue order)"""
    from .book import levels_from_orders
    return quote_from_levels(step, levels_from_orders(bids, 1), levels_from_orders(asks, 1))


# ---------------------------------------------------------------------------------------------------------------- statistics
def stats_from_quotes(rows):
    """The statistics of ONE market's held records of an episode (rows oldest first): int64 [STAT_WORDS].  What CDAVecEnv.quote_stats computes on the device.
    steps; two-sided, bid-only, ask-only and empty steps; over the two-sided steps the sum, sum of squares, minimum and maximum of the spread (ask - bid; 0, 0
    without any), the sum of m2 = bid + ask (twice the mid, kept integer) and the sums of both best-level volumes; over CONSECUTIVE held steps that are both
    two-sided their number (pairs), the number of m2 changes, the sum of |m2' - m2| and of (m2' - m2)^2 - the realised variance of the mid, times four."""
    r = as_rows(rows).astype(np.int64)
    out = np.zeros(STAT_WORDS, np.int64)
    side = r[:, 1] & 3
    two = side == 3
    out[STAT["steps"]] = len(r)
    out[STAT["two_sided"]], out[STAT["bid_only"]], out[STAT["ask_only"]], out[STAT["empty"]] = two.sum(), (side == 1).sum(), (side == 2).sum(), (side == 0).sum()
    spread, m2 = (r[:, 3] - r[:, 2])[two], (r[:, 2] + r[:, 3])
    if two.any():
        out[STAT["spread_sum"]], out[STAT["spread_sq"]], out[STAT["spread_min"]], out[STAT["spread_max"]] = spread.sum(), (spread * spread).sum(), spread.min(), spread.max()
        out[STAT["m2_sum"]], out[STAT["bid_volume"]], out[STAT["ask_volume"]] = m2[two].sum(), r[two, 4].sum(), r[two, 5].sum()
    pair = two[1:] & two[:-1]
    d = (m2[1:] - m2[:-1])[pair]
    out[STAT["pairs"]], out[STAT["m2_changes"]], out[STAT["abs_dm2"]], out[STAT["dm2_sq"]] = pair.sum(), (d != 0).sum(), np.abs(d).sum(), (d * d).sum()
    return out


def stats_summary(stats):
    """the ratios a person reads off one row of quote_stats: a dict; a ratio whose denominator is 0 is None"""
    s = {f: int(x) for f, x in zip(STAT_FIELDS, np.asarray(stats.detach().cpu().numpy() if hasattr(stats, "detach") else stats, dtype=np.int64).reshape(-1))}
    n = s["two_sided"]
    return {"steps": s["steps"], "two_sided_share": _ratio(n, s["steps"]), "mean_spread": _ratio(s["spread_sum"], n), "min_spread": s["spread_min"] if n else None,
            "max_spread": s["spread_max"] if n else None, "mean_mid": _ratio(s["m2_sum"], 2 * n), "mean_bid_volume": _ratio(s["bid_volume"], n),
            "mean_ask_volume": _ratio(s["ask_volume"], n), "mid_change_share": _ratio(s["m2_changes"], s["pairs"]),
            "realised_variance_per_step": _ratio(s["dm2_sq"], 4 * s["pairs"])}


# ---------------------------------------------------------------------------------------------------------------- spread reports
# (the horizons' check is tape.py's _horizons, imported above: MAX_HORIZONS == tape.MAX_HORIZONS)


def spreads_from_records(tape_rows, quote_rows, horizons, num_agents):
    """The spread report of ONE market's episode: its tape rows (tape.RECORD_DTYPE rows, tape order, as held) joined by step to its HELD quote rows (oldest first:
    consecutive steps) -> int64 [A, H, 2, 6].  What CDAVecEnv.tape_spreads computes on the device, and its specification.

    A fill has a step s, a price p, a quantity q and two parties: counter_id (role 0, maker) and init_id (role 1, taker), each with side = +1 if it bought (its
    side bit is 0 = bid), -1 if it sold; a self-trade is skipped.  m2(t) = bid + ask of the quote of step t (twice the mid).  For horizon k, with Q0 .. Q1 the steps
    of the first and last held quote (no quote held: every fill is open):
      s + k > Q1                                                        open += 1          (the episode has not run, or did not run, that far: never extrapolated)
      else s < Q0, or quote(s) or quote(s + k) not two-sided            unquoted += 1      (s < Q0: overwritten in the ring, or never recorded)
      else   cost_now += side (2p - m2(s)) q;  cost_later += side (2p - m2(s + k)) q;  qty += q;  fills += 1
    per (agent, horizon, role), SPREAD_FIELDS order.  Effective half-spread per share = cost_now / (2 qty) for a taker; see spread_summary."""
    from .tape import as_rows as tape_rows_of
    t = tape_rows_of(tape_rows).astype(np.int64) if np.size(tape_rows) else np.zeros((0, 8), np.int64)
    q = as_rows(quote_rows).astype(np.int64)
    a, hz = int(num_agents), _horizons(horizons)
    out = np.zeros((a, len(hz), 2, SPREAD_WORDS), np.int64)
    if len(t) == 0:
        return out
    if t[:, [3, 6]].min() < 0 or t[:, [3, 6]].max() >= a:
        raise ValueError(f"an agent id of the tape is outside 0 .. {a - 1}")
    if len(q) and not np.array_equal(q[:, 0], q[0, 0] + np.arange(len(q))):
        raise ValueError("the quote rows are not the consecutive steps of one episode")
    q0, q1 = (int(q[0, 0]), int(q[-1, 0])) if len(q) else (0, -1)
    two = (q[:, 1] & 3) == 3
    m2 = q[:, 2] + q[:, 3]
    for cid, iid, p, n, ss in zip(t[:, 3], t[:, 6], t[:, 1], t[:, 2], t[:, 7]):
        if cid == iid:
            continue
        s = int(ss >> 2)
        parties = ((int(cid), 1 if ss & 1 == 0 else -1, 0), (int(iid), 1 if (ss >> 1) & 1 == 0 else -1, 1))
        for h, k in enumerate(hz):
            if s + k > q1:
                word = "open"
            elif s < q0 or not two[s - q0] or not two[s + k - q0]:
                word = "unquoted"
            else:
                word = None
            for who, side, role in parties:
                cell = out[who, h, role]
                if word is not None:
                    cell[SPREAD_FIELDS.index(word)] += 1
                else:
                    cell[0] += side * (2 * p - m2[s - q0]) * n
                    cell[1] += side * (2 * p - m2[s + k - q0]) * n
                    cell[2] += n
                    cell[3] += 1
    return out


def spreads_by_module(spreads, slot_module, n_modules):
    """Per-market spread tables summed into one per module through a league's slot -> module map, as tape.exec_by_module folds the execution report: spreads i64
    [N, A, H, 2, 6] (CDAVecEnv.tape_spreads), slot_module integer [N, A] -> i64 [n_modules, H, 2, 6].  Every word is additive.  torch tensors, on the device the
    table is on (one index_add_)."""
    import torch
    n, a = spreads.shape[0], spreads.shape[1]
    if spreads.dim() != 5 or tuple(spreads.shape[3:]) != (2, SPREAD_WORDS) or tuple(slot_module.shape) != (n, a):
        raise ValueError(f"spreads must be [N, A, H, 2, {SPREAD_WORDS}] and slot_module [N, A], got {tuple(spreads.shape)} and {tuple(slot_module.shape)}")
    m, h = int(n_modules), spreads.shape[2]
    mod = slot_module.to(device=spreads.device, dtype=torch.int64).reshape(-1)
    if mod.numel() and (int(mod.min()) < 0 or int(mod.max()) >= m):
        raise ValueError(f"a module id is outside 0 .. {m - 1}")
    out = torch.zeros((m, h * 2 * SPREAD_WORDS), dtype=torch.int64, device=spreads.device)
    out.index_add_(0, mod, spreads.reshape(-1, h * 2 * SPREAD_WORDS).to(torch.int64))
    return out.reshape(m, h, 2, SPREAD_WORDS)


def _ratio(x, y):
    return float(x) / float(y) if y else None


def spread_summary(spreads, horizons=None):
    """The ratios a person reads, from the integers of ONE row: spreads [H, 2, 6] of an agent (spreads_from_records, CDAVecEnv.tape_spreads) or of a module
    (spreads_by_module) -> {horizon: {role: {...}}}.  Per share, in price units, signed so that a COST is positive: a taker that lifts the ask pays
    effective_half_spread = cost_now / (2 qty) > 0 and a maker earns it (its number is negative); realised_half_spread = cost_later / (2 qty) is what is left of
    that k steps later, at the mid then; impact = effective - realised = how far the mid moved with the trade.  Beside them the scored quantity and fills, and
    the fills left out - open, unquoted - which are reported, never hidden; coverage = scored / all.  A ratio whose denominator is 0 is None."""
    sp = np.asarray(spreads.detach().cpu().numpy() if hasattr(spreads, "detach") else spreads, dtype=np.int64)
    if sp.ndim != 3 or sp.shape[1:] != (2, SPREAD_WORDS):
        raise ValueError(f"spread_summary takes one row: spreads [H, 2, {SPREAD_WORDS}], got {sp.shape}")
    hz = list(range(sp.shape[0])) if horizons is None else _horizons(horizons)
    if len(hz) != sp.shape[0]:
        raise ValueError(f"{len(hz)} horizons named for {sp.shape[0]} rows")
    out = {}
    for h, k in enumerate(hz):
        row = {}
        for role, name in enumerate(ROLES):
            now, later, qty, fills, opened, unq = (int(x) for x in sp[h, role])
            row[name] = {"effective_half_spread": _ratio(now, 2 * qty), "realised_half_spread": _ratio(later, 2 * qty), "impact": _ratio(now - later, 2 * qty),
                         "qty": qty, "fills": fills, "open_fills": opened, "unquoted_fills": unq, "coverage": _ratio(fills, fills + opened + unq)}
        out[("k%d" % k) if horizons is not None else h] = row
    return out


# ---------------------------------------------------------------------------------------------------------------- container
def save(path, records, counts=None, **extra):
    """records i32 [N, K, 8] (or [K, 8]) as CDAVecEnv.quote_series returns them (+ counts i32 [N]: the rows of every market that are records; + any further arrays:
    info, market, episode, module ids ...) -> .npz"""
    rec = records.detach().cpu().numpy() if hasattr(records, "detach") else np.asarray(records)
    if rec.dtype == QUOTE_DTYPE:
        rec = rec.view(np.int32).reshape(rec.shape + (QUOTE_WORDS,))
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    if rec.ndim not in (2, 3) or rec.shape[-1] != QUOTE_WORDS:
        raise ValueError(f"quote records must have shape [N, K, {QUOTE_WORDS}] or [K, {QUOTE_WORDS}], got {rec.shape}")
    data = {"records": rec, "fields": np.array(FIELDS)}
    if counts is not None:
        data["counts"] = np.asarray(counts.detach().cpu().numpy() if hasattr(counts, "detach") else counts, dtype=np.int32)
    for k, v in extra.items():
        data[k] = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    np.savez_compressed(path, **data)


def load(path):
    """the arrays save wrote, as a dict (records as int32 [..., 8]; as_quotes() gives the named view of one market's rows)"""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
