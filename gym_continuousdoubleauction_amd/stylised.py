"""The stylised-facts report on the host: the SPECIFICATION, in plain numpy, of the three reductions of include/cda.h cda_quote_returns, cda_tape_signs and
cda_tape_flow_returns (CDAVecEnv.quote_returns / tape_signs / tape_flow_returns) - the time-series statistics an agent-based market is validated against: are
mid-price returns uncorrelated while their magnitudes cluster, how fat are their tails, how persistent is the sign of order flow, how much does signed volume
move the price - with the field names, the fold over markets (pool) and the figures a person reads (summary).  The device results equal the specifications word
for word.  No device code here (pool is a plain sum, on whatever device the tables are): importable without a GPU.

Common definitions.  m2(s) = bid_price + ask_price of the quote record of episode step s (twice the mid, kept integer), defined iff that record is held and
two-sided.  The bar points are the steps s with s % bar_steps == 0, on the episode's absolute step grid (a lost head does not shift the grid); point p is step
p * bar_steps.  The return at point p is r_p = m2((p + 1) bar_steps) - m2(p bar_steps), defined iff both are; it is in half price units, like quote_stats' dm2.
The sign of a fill is +1 where the initiator bought (init side 0 = bid), -1 where it sold; self-trades are fills like any other.  Every word is an int64 sum
with two's-complement wrap (numpy's): a fold over markets, episodes or ranks is a plain sum - there are no min / max words."""
import numpy as np

from .quotes import as_rows as _quote_rows

MAX_BARS = 4096                                                  # include/cda.h CDA_STYL_MAX_BARS: bar points of the longest episode a launch takes
MAX_LAGS = 8                                                     # CDA_STYL_MAX_LAGS
MAX_LAG = 1 << 20                                                # CDA_STYL_MAX_LAG: the largest single lag (the trade tape's largest ring)
MAX_HIST_HALF = 64                                               # CDA_STYL_MAX_HIST_HALF

RETURN_FIELDS = ("bars", "returns", "missing", "sum_r", "sum_abs", "sum_r2", "up", "down")
RETURN_LAG_FIELDS = ("n", "rr", "aa", "ra")
SIGN_FIELDS = ("fills", "buys", "sells", "buy_qty", "sell_qty", "self_fills", "runs", "steps_with_fills")
SIGN_LAG_FIELDS = ("n", "ss", "qq", "same_step")
FLOW_FIELDS = ("fills", "bars_with_fills", "bars_excluded", "qty")
FLOW_LAG_FIELDS = ("n", "q", "r", "qr", "qq", "rr")
RET, RLAG, SGN, SLAG, FLW, FLAG = ({name: i for i, name in enumerate(f)} for f in
                                   (RETURN_FIELDS, RETURN_LAG_FIELDS, SIGN_FIELDS, SIGN_LAG_FIELDS, FLOW_FIELDS, FLOW_LAG_FIELDS))


def _lags(lags, lowest):
    lg = [int(k) for k in (lags if hasattr(lags, "__iter__") else (lags,))]
    if not 1 <= len(lg) <= MAX_LAGS or min(lg) < lowest or max(lg) > MAX_LAG:
        raise ValueError(f"lags: 1 .. {MAX_LAGS} values in {lowest} .. {MAX_LAG}, got {lags!r}")
    return lg


def _bar_steps(bar_steps):
    if int(bar_steps) < 1:
        raise ValueError(f"bar_steps must be >= 1, got {bar_steps}")
    return int(bar_steps)


def n_points(max_step, bar_steps):
    """the bar points of an episode of max_step steps: ceil(max_step / bar_steps); a launch takes at most MAX_BARS of them"""
    return -(-int(max_step) // int(bar_steps))


def _tape_rows(rows):
    from .tape import as_rows
    return as_rows(rows).astype(np.int64) if np.size(rows) else np.zeros((0, 8), np.int64)


def _points(quote_rows, bar):
    """(first held point p0, m2 int64 [P] of the held points p0 .. p0 + P - 1 with 0 = not two-sided) of one market's held quote rows (consecutive steps)"""
    q = _quote_rows(quote_rows).astype(np.int64)
    if len(q) and not np.array_equal(q[:, 0], q[0, 0] + np.arange(len(q))):
        raise ValueError("the quote rows are not the consecutive steps of one episode")
    if len(q) == 0:
        return 0, np.zeros(0, np.int64)
    p0 = -(-int(q[0, 0]) // bar)
    at = q[p0 * bar - int(q[0, 0])::bar]
    return p0, np.where((at[:, 1] & 3) == 3, at[:, 2] + at[:, 3], 0)


def _returns(m2):
    """(r int64 [P], defined bool [P]) of the points' m2: r_i = m2[i + 1] - m2[i]; the last point has no return"""
    nxt = np.concatenate([m2[1:], np.zeros(min(1, len(m2)), np.int64)])
    ok = (m2 != 0) & (nxt != 0)
    return np.where(ok, nxt - m2, 0), ok


def returns_from_quotes(quote_rows, lags, bar_steps=1, hist_half=16, tick=1):
    """The return statistics of ONE market's held quote rows of an episode (oldest first: consecutive steps) -> (base int64 [8], lagged int64 [L, 4], hist int64
    [2 hist_half + 1]).  What CDAVecEnv.quote_returns computes on the device, and its specification.
      base    RETURN_FIELDS: bars = the bar points held; returns = the returns that are defined; missing = adjacent held point pairs with an endpoint that is
              not two-sided; sum_r, sum_abs, sum_r2 over the defined returns; up / down = the returns > 0 / < 0.
      lagged  per lag l >= 1, over the points p where r_p and r_(p + l) are both defined, RETURN_LAG_FIELDS: n, rr = sum r r', aa = sum |r| |r'| (volatility
              clustering), ra = sum r |r'| (the leverage term: today's return against the later magnitude).
      hist    bin clamp(r / tick, -hist_half, hist_half) + hist_half of every defined return; tick = the market's tick_size (prices are multiples of it: the
              division is exact; it truncates toward zero otherwise).  The end bins hold the clipped mass.
    At bar_steps = 1: returns == quote_stats' pairs, sum_r2 == dm2_sq, sum_abs == abs_dm2."""
    bar, lg, hh, tick = _bar_steps(bar_steps), _lags(lags, 1), int(hist_half), int(tick)
    if not 1 <= hh <= MAX_HIST_HALF or tick < 1:
        raise ValueError(f"hist_half must be in 1 .. {MAX_HIST_HALF} and tick >= 1, got {hist_half} and {tick}")
    _, m2 = _points(quote_rows, bar)
    r, ok = _returns(m2)
    a = np.abs(r)
    base = np.zeros(len(RETURN_FIELDS), np.int64)
    base[:] = (len(m2), ok.sum(), max(len(m2) - 1, 0) - ok.sum(), r.sum(), a.sum(), (r * r).sum(), (r > 0).sum(), (r < 0).sum())
    lagged = np.zeros((len(lg), len(RETURN_LAG_FIELDS)), np.int64)
    for h, l in enumerate(lg):
        if l < len(r):
            both = ok[:-l] & ok[l:]
            x, y = r[:-l][both], r[l:][both]
            lagged[h] = (both.sum(), (x * y).sum(), (np.abs(x) * np.abs(y)).sum(), (x * np.abs(y)).sum())
    bins = np.clip(np.sign(r[ok]) * (a[ok] // tick), -hh, hh) + hh
    return base, lagged, np.bincount(bins, minlength=2 * hh + 1).astype(np.int64)


def signs_from_records(tape_rows, lags):
    """The order-flow sign statistics of ONE market's held tape rows of an episode (tape.RECORD_DTYPE rows, tape order) -> (base int64 [8], lagged int64 [L, 4]).
    What CDAVecEnv.tape_signs computes on the device, and its specification.  Fill i has sign s_i, quantity q_i and env step t_i.
      base    SIGN_FIELDS: fills; buys, sells (s = +1 / -1); buy_qty, sell_qty; self_fills (counter_id == init_id); runs = the maximal runs of equal sign;
              steps_with_fills = the fills whose step differs from the fill before them, the first one included (steps never decrease within an episode).
      lagged  per lag l >= 1 in TRADE time, over the pairs of fills i and i + l, SIGN_LAG_FIELDS: n, ss = sum s s', qq = sum (s q)(s' q'), same_step = the
              pairs whose two fills carry the same env step - one sweep prints many same-sign fills in one step: the mechanical part of the persistence."""
    lg = _lags(lags, 1)
    t = _tape_rows(tape_rows)
    s = np.where((t[:, 7] >> 1) & 1 == 0, 1, -1).astype(np.int64)
    q, step = t[:, 2], t[:, 7] >> 2
    base = np.zeros(len(SIGN_FIELDS), np.int64)
    if len(t):
        base[:] = (len(t), (s > 0).sum(), (s < 0).sum(), q[s > 0].sum(), q[s < 0].sum(), (t[:, 3] == t[:, 6]).sum(), 1 + (s[1:] != s[:-1]).sum(),
                   1 + (step[1:] != step[:-1]).sum())
    lagged = np.zeros((len(lg), len(SIGN_LAG_FIELDS)), np.int64)
    for h, l in enumerate(lg):
        if l < len(t):
            lagged[h] = (len(t) - l, (s[:-l] * s[l:]).sum(), (s[:-l] * q[:-l] * s[l:] * q[l:]).sum(), (step[:-l] == step[l:]).sum())
    return base, lagged


def flow_returns_from_records(tape_rows, quote_rows, lags, bar_steps=1, tape_lost=0):
    """Signed volume joined to returns, bar by bar, of ONE market's episode: its held tape rows (tape order) and its held quote rows (consecutive steps) ->
    (lagged int64 [L, 6], base int64 [4]).  What CDAVecEnv.tape_flow_returns computes on the device, and its specification.
    Bar b covers the steps [b bar_steps, (b + 1) bar_steps); Q_b = the sum of sign x quantity over its held fills, kept as an int32 word (it wraps beyond 2^31;
    a bar without fills has Q_b = 0 and counts); r_b = the return at point b.  tape_lost > 0 (the ring has lost the episode's head: info's second word): every
    bar up to and including the bar of the first held fill is excluded - all bars, where no fill is held at all - and bars_excluded says how many: that bar's
    index + 1, or, with no fill held, the bars that begin at or before the last held quote step.
      lagged  per lag l >= 0, over the kept bars b whose r_(b + l) is defined, FLOW_LAG_FIELDS: n, q = sum Q_b, r = sum r_(b + l), qr, qq, rr.  Lag 0 is the
              contemporaneous impact regression (Kyle's lambda = cov / var, and its R^2); lags >= 1 say whether flow predicts returns.
      base    FLOW_FIELDS: the fills of the kept bars, the kept bars that have fills, bars_excluded, the quantity of the kept bars' fills."""
    bar, lg = _bar_steps(bar_steps), _lags(lags, 0)
    t = _tape_rows(tape_rows)
    p0, m2 = _points(quote_rows, bar)
    r, ok = _returns(m2)
    fb = (t[:, 7] >> 2) // bar                                   # every fill's bar
    first = 0
    if int(tape_lost) > 0:
        first = int(fb[0]) + 1 if len(t) else p0 + len(m2)
    kept = fb >= first
    base = np.array([kept.sum(), len(np.unique(fb[kept])), first, t[kept, 2].sum()], np.int64)
    lagged = np.zeros((len(lg), len(FLOW_LAG_FIELDS)), np.int64)
    n_bars = max(p0 + len(m2), int(fb.max()) + 1 if len(t) else 0)
    Q = np.zeros(n_bars, np.int64)
    np.add.at(Q, fb, np.where((t[:, 7] >> 1) & 1 == 0, t[:, 2], -t[:, 2]))
    Q = Q.astype(np.int32).astype(np.int64)
    for h, l in enumerate(lg):
        b = np.arange(max(first, p0 - l), p0 + len(m2) - l)       # the bars whose point b + l is held
        if len(b) == 0:
            continue
        b = b[ok[b + l - p0]]
        x, y = Q[b], r[b + l - p0]
        lagged[h] = (len(b), x.sum(), y.sum(), (x * y).sum(), (x * x).sum(), (y * y).sum())
    return lagged, base


# ---------------------------------------------------------------------------------------------------------------- the fold and the figures
def pool(table):
    """the sum over markets (axis 0) of any of the tables: every word is additive.  numpy arrays and torch tensors alike (a tensor stays on its device)."""
    if hasattr(table, "detach"):
        return table.sum(dim=0)
    return np.asarray(table, dtype=np.int64).sum(axis=0)


def _host(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.int64)


def _ratio(x, y):
    return float(x) / float(y) if y else None


def _corr(n, sxy, sx, sy, sxx, syy):
    """the correlation of n pairs from their sums; None where a variance is 0"""
    if not n:
        return None
    cov, vx, vy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    return cov / (vx * vy) ** 0.5 if vx > 0 and vy > 0 else None


def returns_summary(base, lagged, hist, lags, tick=1):
    """The figures of one POOLED quote_returns result (base [8], lagged [L, 4], hist [B]; `tick`: the tick the histogram's bins are in - pool markets of one tick).
    mean, variance and mean magnitude of a return (half price units); per lag the autocorrelation of returns acf = (rr / n - mean^2) / variance, of their
    magnitudes acf_abs = (aa / n - mean_abs^2) / variance_abs and the leverage correlation (ra / n - mean mean_abs) / (sd sd_abs) - all with the whole sample's
    moments; from the histogram (bin centres, in ticks) the excess kurtosis and the share of the mass in the two end bins (clipped: the tails the bins cut)."""
    b, lg, h = [int(x) for x in _host(base)], _host(lagged), _host(hist)
    s = dict(zip(RETURN_FIELDS, b))
    n = s["returns"]
    mean, mean_abs = _ratio(s["sum_r"], n), _ratio(s["sum_abs"], n)
    var = None if not n else s["sum_r2"] / n - mean * mean
    var_abs = None if not n else s["sum_r2"] / n - mean_abs * mean_abs
    out = {"bars": s["bars"], "returns": n, "missing": s["missing"], "mean": mean, "variance": var, "mean_abs": mean_abs, "up_share": _ratio(s["up"], n),
           "down_share": _ratio(s["down"], n), "lags": {}}
    for row, l in zip(lg, _lags(lags, 1)):
        k, rr, aa, ra = (int(x) for x in row)
        out["lags"]["k%d" % l] = {"n": k, "acf": _ratio(rr / k - mean * mean, var) if k and var else None,
                                  "acf_abs": _ratio(aa / k - mean_abs * mean_abs, var_abs) if k and var_abs else None,
                                  "leverage": (ra / k - mean * mean_abs) / (var * var_abs) ** 0.5 if k and var and var_abs and var > 0 and var_abs > 0 else None}
    half, tot = (len(h) - 1) // 2, int(h.sum())
    x = (np.arange(len(h)) - half).astype(np.float64) * float(tick)
    kurt = None
    if tot:
        mu = float((h * x).sum()) / tot
        m2, m4 = float((h * (x - mu) ** 2).sum()) / tot, float((h * (x - mu) ** 4).sum()) / tot
        kurt = m4 / (m2 * m2) - 3.0 if m2 > 0 else None
    out["excess_kurtosis"], out["clipped_share"] = kurt, _ratio(int(h[0]) + int(h[-1]), tot)
    return out


def variance_ratio(base_1, base_k, k):
    """The variance ratio from two POOLED quote_returns results, at bar sizes 1 and k: Var(r over k steps) / (k Var(r over 1 step)); 1 for a random walk, below 1
    where returns mean-revert (bid-ask bounce), above 1 where they trend.  None where a variance is 0."""
    v = []
    for b in (base_1, base_k):
        s = dict(zip(RETURN_FIELDS, (int(x) for x in _host(b))))
        n = s["returns"]
        v.append(None if not n else s["sum_r2"] / n - (s["sum_r"] / n) ** 2)
    return _ratio(v[1], int(k) * v[0]) if v[0] and v[1] is not None else None


def signs_summary(base, lagged, lags):
    """The figures of one POOLED tape_signs result: buy share, mean run length, fills per step that has any; per lag the sign autocorrelation acf = (ss / n -
    mean^2) / (1 - mean^2), mean = (buys - sells) / fills, the share of the pairs that lie within one step (same_step_share) and the same autocorrelation over
    the pairs that do NOT (acf_across_steps: a same-step pair counted as it almost always is - one sweep, equal signs, s s' = +1).  A tape of one sign only has
    no variance to divide by: its acf is reported as 1.0 (every pair agrees), the one ratio here that is not None on a zero denominator."""
    s = dict(zip(SIGN_FIELDS, (int(x) for x in _host(base))))
    n = s["fills"]
    mean = _ratio(s["buys"] - s["sells"], n)
    var = None if mean is None else 1.0 - mean * mean
    out = {"fills": n, "buy_share": _ratio(s["buys"], n), "buy_qty_share": _ratio(s["buy_qty"], s["buy_qty"] + s["sell_qty"]), "self_share": _ratio(s["self_fills"], n),
           "mean_run": _ratio(n, s["runs"]), "fills_per_step": _ratio(n, s["steps_with_fills"]), "lags": {}}
    for row, l in zip(_host(lagged), _lags(lags, 1)):
        k, ss, qq, same = (int(x) for x in row)
        across = k - same
        out["lags"]["k%d" % l] = {"n": k, "acf": _ratio(ss / k - mean * mean, var) if k and var else (1.0 if k and var == 0 else None), "same_step_share": _ratio(same, k),
                                  "acf_across_steps": _ratio((ss - same) / across - mean * mean, var) if across and var else None,
                                  "qq_mean": _ratio(qq, k)}
    return out


def flow_summary(lagged, base, lags):
    """The figures of one POOLED tape_flow_returns result: per lag the regression of r_(b + l) on Q_b - lambda = cov / var(Q) (half price units per unit of signed
    volume; lag 0: Kyle's lambda), its R^2 = corr^2 and the correlation itself."""
    s = dict(zip(FLOW_FIELDS, (int(x) for x in _host(base))))
    out = dict(s, lags={})
    for row, l in zip(_host(lagged), _lags(lags, 0)):
        n, q, r, qr, qq, rr = (int(x) for x in row)
        corr = _corr(n, qr, q, r, qq, rr)
        out["lags"]["k%d" % l] = {"n": n, "lambda": _ratio(n * qr - q * r, n * qq - q * q) if n else None, "corr": corr, "r2": None if corr is None else corr * corr}
    return out


def summary(returns=None, returns_k=None, signs=None, flows=None, lags=None, flow_lags=None, bar_steps=1, k=None, tick=1):
    """Pooled tables -> the figures a person reads, one block per table given: returns = (base, lagged, hist) of quote_returns at `bar_steps`; returns_k = the
    same at bar size k x bar_steps (adds variance_ratio to the returns block); signs = (base, lagged) of tape_signs; flows = (lagged, base) of tape_flow_returns.
    lags name the rows of returns and signs, flow_lags (default: lags) those of flows.  Tables of several markets ([n, ...]) are pooled first.  A ratio with a
    zero denominator is None."""
    def pooled(t, dims):
        t = _host(t)
        return t.sum(axis=0) if t.ndim == dims + 1 else t
    out = {"bar_steps": int(bar_steps)}
    if returns is not None:
        b, lg, h = pooled(returns[0], 1), pooled(returns[1], 2), pooled(returns[2], 1)
        out["returns"] = returns_summary(b, lg, h, lags, tick)
        if returns_k is not None:
            out["returns"]["variance_ratio"] = {"k": int(k), "value": variance_ratio(b, pooled(returns_k[0], 1), k)}
    if signs is not None:
        out["signs"] = signs_summary(pooled(signs[0], 1), pooled(signs[1], 2), lags)
    if flows is not None:
        out["flows"] = flow_summary(pooled(flows[0], 2), pooled(flows[1], 1), lags if flow_lags is None else flow_lags)
    return out
