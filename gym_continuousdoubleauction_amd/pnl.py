"""The P&L report on the host: the SPECIFICATION, in plain numpy, of include/cda.h cda_tape_pnl (CDAVecEnv.tape_pnl) - what every agent's mark-to-mid P&L did
over one remembered episode: its equity curve on the bar points, the drawdown, the moments of the per-bar P&L, the time under water, and the market-making split
of the P&L into what the carried inventory gained or lost on the mid's moves and what the trades themselves earned against each bar's closing mid - with the
field names, the fold over markets, episodes and modules (fold, pnl_by_module) and the figures a person reads (pnl_summary).  The device result equals the
specification word for word.  No device code here (pnl_by_module is torch, on whatever device the table is): importable without a GPU.

Definitions (the conventions of stylised.py hold).  m2(s) = bid_price + ask_price of the held, two-sided quote record of step s.  Point p is step p * bar_steps on
the episode's absolute grid; it is HELD iff its quote record is.  The MARK m(p) is m2 of the latest held point p' <= p whose quote is two-sided: it carries forward
over points, not over the steps between them.  A held point is MARKED if such a p' exists (the held points before the first two-sided one are unmarked) and STALE
if it is marked and its own quote is not two-sided.  An agent's fills are the non-self fills (counter_id != init_id) it is a party of, with the signed quantity
sq = +quantity where it bought (its side bit is 0), -quantity where it sold.  A fill of step s is INSIDE point p iff s < p * bar_steps (a step's quote is taken
ahead of its orders).  pos(p) = the sum of sq and C(p) = the sum of -sq * price over the held fills inside p; the equity, in half price units (twice the money, as
m2 is twice the mid), is E(p) = 2 C(p) + pos(p) m(p) at the marked points.  For adjacent marked points d_p = E(p + 1) - E(p) = inv_p + trd_p EXACTLY:
inv_p = pos(p) (m(p + 1) - m(p)), trd_p = the sum over the agent's fills of bar p (steps [p bar, (p + 1) bar)) of sq (m(p + 1) - 2 price).  Nothing is
extrapolated: where the tape ring has lost the episode's head pos and C start from the first held fill; where the quote ring has, the points start at the first
held quote.  Fills at steps >= (the last marked point) * bar_steps - every fill, where no point is marked - are in no equity point: OPEN, counted, never marked.
Products are int64 and sums wrap in two's complement (numpy's); a bar's signed quantity is kept as an int32 word, as stylised.py's Q_b."""
import numpy as np

from .stylised import MAX_BARS, _bar_steps, _points, _tape_rows, n_points  # noqa: F401  (MAX_BARS, n_points: what a caller sizes a series by)

PNL_FIELDS = ("points", "stale", "unmarked", "bars", "equity_first", "equity_last", "inventory", "trading", "sum_d2", "up", "down", "under_water", "max_drawdown",
              "equity_max", "equity_min", "open_fills")
PNL_WORDS = len(PNL_FIELDS)                                      # include/cda.h CDA_PNL_WORDS
PNL = {name: i for i, name in enumerate(PNL_FIELDS)}
# what a fold over markets, episodes or slots sums; max_drawdown and equity_max take the max, equity_min the min - over the rows with points > 0
PNL_ADDITIVE = tuple(f for f in PNL_FIELDS if f not in ("max_drawdown", "equity_max", "equity_min"))
PNL_MAX, PNL_MIN = ("max_drawdown", "equity_max"), ("equity_min",)


def pnl_from_records(tape_rows, quote_rows, num_agents, bar_steps=1, n_points=None):
    """The P&L report of ONE market's episode: its held tape rows (tape.RECORD_DTYPE rows, tape order) joined to its HELD quote rows (oldest first: consecutive
    steps) -> (stats int64 [A, 16] - PNL_FIELDS -, equity int64 [A, P], position int32 [A, P], marks int32 [P]).  What CDAVecEnv.tape_pnl computes on the device,
    and its specification.  The series are on the absolute grid of points 0 .. P - 1: E(p), 0 where p is not marked; pos(p), 0 where p is not held; m(p), 0 where
    p is not marked.  P = n_points, or, where it is None, the last held point + 1; an n_points below that is an error.
      points, stale, unmarked   the marked points, those of them that are stale, and the held points that are not marked.
      bars                      the defined increments: max(points - 1, 0) - held points are consecutive, so every point behind a marked one is marked.
      equity_first / _last      E at the first / last marked point;  inventory, trading = the sums of inv_p and trd_p: inventory + trading == equity_last -
                                equity_first;  sum_d2 = the sum of d_p^2;  up, down = the bars with d_p > 0 / < 0.
      under_water               the marked points with E below its running maximum (which starts at equity_first);  max_drawdown = the largest running
                                maximum - E, >= 0;  equity_max, equity_min over the marked points (0 where there is none).
      open_fills                the agent's fills at steps >= (last marked point) * bar_steps; all of them where no point is marked."""
    bar, a = _bar_steps(bar_steps), int(num_agents)
    t = _tape_rows(tape_rows)
    if len(t) and (t[:, [3, 6]].min() < 0 or t[:, [3, 6]].max() >= a):
        raise ValueError(f"an agent id of the tape is outside 0 .. {a - 1}")
    p0, m2 = _points(quote_rows, bar)                                # (raises where the quote rows are not consecutive steps)
    hi = p0 + len(m2) - 1                                            # the last held point (p0 - 1: none)
    P = hi + 1 if n_points is None else int(n_points)
    if P < hi + 1:
        raise ValueError(f"n_points = {P} is below the episode's {hi + 1} points")
    two = m2 != 0
    last = np.maximum.accumulate(np.where(two, np.arange(len(m2)), -1)) if len(m2) else np.zeros(0, np.int64)
    marked = last >= 0
    mark = np.where(marked, m2[np.maximum(last, 0)], 0) if len(m2) else np.zeros(0, np.int64)
    n_marked = int(marked.sum())
    stats = np.zeros((a, PNL_WORDS), np.int64)
    equity, position, marks = np.zeros((a, P), np.int64), np.zeros((a, P), np.int32), np.zeros(P, np.int32)
    marks[p0:hi + 1] = mark
    stats[:, PNL["points"]], stats[:, PNL["stale"]], stats[:, PNL["unmarked"]] = n_marked, int((marked & ~two).sum()), len(m2) - n_marked
    stats[:, PNL["bars"]] = max(n_marked - 1, 0)
    fb = (t[:, 7] >> 2) // bar                                       # every fill's bar
    real = t[:, 3] != t[:, 6]
    n_bars = max(hi + 1, int(fb.max()) + 1 if len(t) else 0)
    for who in range(a):
        mine = real & ((t[:, 3] == who) | (t[:, 6] == who))
        side = np.where(t[mine, 6] == who, (t[mine, 7] >> 1) & 1, t[mine, 7] & 1)
        sq, price, b = np.where(side == 0, t[mine, 2], -t[mine, 2]), t[mine, 1], fb[mine]
        stats[who, PNL["open_fills"]] = int((b >= hi).sum()) if n_marked else int(mine.sum())
        Q, dC = np.zeros(n_bars, np.int64), np.zeros(n_bars, np.int64)
        np.add.at(Q, b, sq)
        np.add.at(dC, b, -sq * price)
        Q = Q.astype(np.int32).astype(np.int64)
        pos = np.concatenate([[0], np.cumsum(Q)])[p0:hi + 1]         # ahead of the held points: the bars below each
        C = np.concatenate([[0], np.cumsum(dC)])[p0:hi + 1]
        position[who, p0:hi + 1] = pos.astype(np.int32)
        if not n_marked:
            continue
        E = (2 * C + pos * mark)[marked]
        pm, mm = pos[marked], mark[marked]
        f = p0 + int(np.argmax(marked))                              # the first marked point
        equity[who, f:hi + 1] = E
        d = E[1:] - E[:-1]
        inv = pm[:-1] * (mm[1:] - mm[:-1])
        trd = Q[f:hi] * mm[1:] + 2 * dC[f:hi]                        # bar p's fills against m(p + 1)
        top = np.maximum.accumulate(E)
        stats[who, PNL["equity_first"]:PNL["open_fills"]] = (E[0], E[-1], inv.sum(), trd.sum(), (d * d).sum(), (d > 0).sum(), (d < 0).sum(), (E < top).sum(),
                                                             (top - E).max(), E.max(), E.min())
    return stats, equity, position, marks


# ---------------------------------------------------------------------------------------------------------------- the fold and the figures
def fold(tables):
    """Rows of PNL_FIELDS ([..., 16]: markets, agents, episodes, ranks - or a list of such tables) -> one row [16]: the PNL_ADDITIVE words are summed (int64, wrapping),
    max_drawdown and equity_max take the largest and equity_min the smallest value over the rows with points > 0 (0 where there is none).  numpy arrays and torch
    tensors alike (a tensor stays on its device)."""
    if isinstance(tables, (list, tuple)):
        if len(tables) and hasattr(tables[0], "detach"):
            import torch
            tables = torch.cat([t.reshape(-1, PNL_WORDS) for t in tables])
        else:
            tables = np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1, PNL_WORDS) for t in tables]) if len(tables) else np.zeros((0, PNL_WORDS), np.int64)
    if hasattr(tables, "detach"):
        import torch
        rows = tables.reshape(-1, PNL_WORDS).to(torch.int64)
        return pnl_by_module(rows[:, None, :], torch.zeros((rows.shape[0], 1), dtype=torch.int64, device=rows.device), 1)[0]
    rows = np.asarray(tables, dtype=np.int64).reshape(-1, PNL_WORDS)
    out = np.zeros(PNL_WORDS, np.int64)
    add = [PNL[f] for f in PNL_ADDITIVE]
    out[add] = rows[:, add].sum(axis=0)
    some = rows[rows[:, PNL["points"]] > 0]
    if len(some):
        for f in PNL_MAX:
            out[PNL[f]] = some[:, PNL[f]].max()
        for f in PNL_MIN:
            out[PNL[f]] = some[:, PNL[f]].min()
    return out


pool = fold


def pnl_by_module(stats, slot_module, n_modules):
    """Per-market P&L tables folded into one row per module through a league's slot -> module map, as tape.exec_by_module folds the execution report: stats i64
    [N, A, 16] (CDAVecEnv.tape_pnl), slot_module integer [N, A] -> i64 [n_modules, 16], by the rule of fold: the PNL_ADDITIVE words summed, max_drawdown and
    equity_max the largest, equity_min the smallest value of the module's slots that have points (0 where none has).  torch tensors, on the device the table is on."""
    import torch
    n, a = stats.shape[0], stats.shape[1]
    if tuple(stats.shape) != (n, a, PNL_WORDS) or tuple(slot_module.shape) != (n, a):
        raise ValueError(f"stats must be [N, A, {PNL_WORDS}] and slot_module [N, A], got {tuple(stats.shape)} and {tuple(slot_module.shape)}")
    m = int(n_modules)
    mod = slot_module.to(device=stats.device, dtype=torch.int64).reshape(-1)
    if mod.numel() and (int(mod.min()) < 0 or int(mod.max()) >= m):
        raise ValueError(f"a module id is outside 0 .. {m - 1}")
    s = stats.reshape(-1, PNL_WORDS).to(torch.int64)
    out = torch.zeros((m, PNL_WORDS), dtype=torch.int64, device=stats.device)
    add = [PNL[f] for f in PNL_ADDITIVE]
    out[:, add] = torch.zeros((m, len(add)), dtype=torch.int64, device=stats.device).index_add_(0, mod, s[:, add])
    info = torch.iinfo(torch.int64)
    some = s[:, PNL["points"]] > 0
    index = mod[:, None]
    for names, how, neutral in ((PNL_MAX, "amax", info.min), (PNL_MIN, "amin", info.max)):
        for f in names:
            col = torch.where(some, s[:, PNL[f]], torch.full_like(s[:, PNL[f]], neutral))[:, None]
            v = torch.full((m, 1), neutral, dtype=torch.int64, device=stats.device).scatter_reduce_(0, index, col, how)[:, 0]
            out[:, PNL[f]] = torch.where(v == neutral, torch.zeros_like(v), v)
    return out


def _ratio(x, y):
    return float(x) / float(y) if y else None


def pnl_summary(row, bar_steps=1):
    """The figures a person reads, from the integers of ONE row [16]: an agent's (pnl_from_records, CDAVecEnv.tape_pnl) or a folded one (fold, pnl_by_module).
    Money is in price units (the words are in half price units: halved here): pnl = (equity_last - equity_first) / 2 and its split into inventory and trading,
    max_drawdown, equity_max / equity_min; bar_pnl_mean and bar_pnl_std = the mean and the (population) standard deviation of the per-bar P&L, from equity_last -
    equity_first, sum_d2 and bars; sharpe_per_bar = mean / std and sharpe_episode = that x sqrt(bars); hit_ratio = up / (up + down); under_water_share = the share
    of the marked points below the running maximum; calmar = pnl / max_drawdown.  A ratio whose denominator is 0 is None."""
    r = np.asarray(row.detach().cpu().numpy() if hasattr(row, "detach") else row, dtype=np.int64)
    if r.shape != (PNL_WORDS,):
        raise ValueError(f"pnl_summary takes one row [{PNL_WORDS}], got {r.shape}")
    s = dict(zip(PNL_FIELDS, (int(x) for x in r)))
    total, bars = s["equity_last"] - s["equity_first"], s["bars"]
    mean = _ratio(total, 2 * bars)
    var = None if not bars else max(s["sum_d2"] / (4.0 * bars) - mean * mean, 0.0)
    std = None if var is None else var ** 0.5
    sharpe = _ratio(mean, std) if std else None
    return {"bar_steps": int(bar_steps), "points": s["points"], "stale_points": s["stale"], "unmarked_points": s["unmarked"], "bars": bars, "open_fills": s["open_fills"],
            "pnl": total / 2.0, "inventory_pnl": s["inventory"] / 2.0, "trading_pnl": s["trading"] / 2.0, "max_drawdown": s["max_drawdown"] / 2.0,
            "equity_max": s["equity_max"] / 2.0, "equity_min": s["equity_min"] / 2.0, "bar_pnl_mean": mean, "bar_pnl_std": std, "sharpe_per_bar": sharpe,
            "sharpe_episode": None if sharpe is None else sharpe * bars ** 0.5, "hit_ratio": _ratio(s["up"], s["up"] + s["down"]),
            "under_water_share": _ratio(s["under_water"], s["points"]), "calmar": _ratio(total, s["max_drawdown"])}
