"""Evaluate a trained policy: play it (greedy by default) against chosen opponents and read per-module episode results off the device.

Placement (`slot_modules`): slots 0 .. trained_slots - 1 of every market play the policy (module 0); every other slot of market m plays opponent
opponents[m % P] (module 1 + m % P).  Without opponents the policy plays every slot through the shared-policy chain (self-play).  With opponents the
markets run on a PolicyBank: row 0 is the policy, the frozen rows behind it the network opponents, LEAGUE_RANDOM marks the uniform random module.

The loop resets every market from `seed`, switches the env's episode metrics on BEFORE the chains are built (a toggle after graph capture would not reach
the captured kernels), runs episodes * max_step steps, and reads the episodes that ENDED in that window with module_of = the placement
(episode_metrics.summarise; check_nav_conservation strict).  Episodes still running at the end of the horizon are not counted: `episodes` and each module's
`agent_episodes` say how many completed.  mode="greedy" plays the mode of every network slot's distribution (RLlib's explore=False: mlp.FusedPolicy.act,
the greedy chains); mode="sample" runs the same loop on the sampling kernels.

CLI: python -m gym_continuousdoubleauction_amd.evaluate --policy P [--opponent random|FILE ...] --markets --agents --max-step --episodes --trained-slots
     (a scripted opponent: pass | maker | taker | imbalance | NAME:key=value,...; one with memory: trend | value | execution | NAME:key=value,...)
     [--sample] --seed --out JSON [--tape FILE.npz [--exec-report K[,K...]] [--spread-report K[,K...]]] [--quotes FILE.npz]
     [--stylised-facts L[,L...] [--bar-steps K]] [--pnl-report [--bar-steps K]] [--depth FILE.npz --depth-levels L] [--book-shape-report [--bar-steps K]]
     [--orders FILE.npz] [--order-flow-report]
"""
import argparse
import dataclasses
import json
import time

import numpy as np
import torch

from . import _capi as K
from .episode_metrics import REWARD_TERMS, check_nav_conservation, summarise

RANDOM = "random"


def slot_modules(n_markets, num_agents, trained_slots, n_opponents):
    """the documented placement: int32 [N, A] module per (market, slot) - 0 = the policy, 1 + p = opponent p.  n_opponents = 0: the policy everywhere."""
    N, A, k, P = int(n_markets), int(num_agents), int(trained_slots), int(n_opponents)
    if not 1 <= k <= A:
        raise ValueError(f"trained_slots must be in 1 .. {A} (got {trained_slots})")
    m = np.zeros((N, A), dtype=np.int32)
    if P > 0:
        m[:, k:] = (1 + np.arange(N) % P)[:, None]
    return m


def _as_policy(x, device):
    from .mlp import FusedPolicy, load_policy
    if isinstance(x, FusedPolicy):
        return x
    return load_policy(x, device)


def _describe(x):
    from .mlp import FusedPolicy
    if isinstance(x, str):
        return x
    if dataclasses.is_dataclass(x):
        return repr(x)
    return "FusedPolicy" if isinstance(x, FusedPolicy) else str(x)


def _horizon(total, cap=128):
    """the rollout length: the largest divisor of the step count up to `cap` (the chains' buffers are [T, N, ...])"""
    for h in range(min(cap, total), 0, -1):
        if total % h == 0:
            return h
    return 1


def _tape_episodes(rows, offsets, before, after):
    """The episode counter value (CDAVecEnv.tape_counts()["episode"]) of every record drained after a rollout chunk (nothing dropped); before / after: the
    counters {episode, n_episode} read around the chunk.  A market whose counter did not move: that episode.  Otherwise its last n_episode rows are the current
    episode's (exact: that is what the counter counts); if the counter moved by one, the rows before them are the episode that ended (exact as well); if it
    moved by more (a chunk that spans several episodes) a new episode begins, going backwards, wherever the step index drops - exact unless an episode in
    between had no fill at all."""
    ep = np.zeros(len(rows), np.int32)
    t = rows[:, 7] >> 2
    for m in range(len(offsets) - 1):
        a, b = int(offsets[m]), int(offsets[m + 1])
        e0, e1 = int(before["episode"][m]), int(after["episode"][m])
        if a == b:
            continue
        if e1 == e0:
            ep[a:b] = e0
            continue
        k = min(int(after["n_episode"][m]), b - a)
        ep[b - k:b] = e1
        if b - k > a:
            drops = np.diff(t[a:b - k]) < 0 if e1 > e0 + 1 else np.zeros(b - k - a - 1, bool)
            ep[a:b - k] = (e1 - 1) - np.concatenate([np.cumsum(drops[::-1])[::-1], [0]])
    return ep


def _execution_report(env, horizons, module_of, names, episode0, keep):
    """evaluate(exec_horizons=...): the device tables of every market's previous episode, folded per module.  A market counts when its tape completed an episode
    since `episode0` (its counter at the start of the evaluation); the others' slots are mapped to no module."""
    from .tape import MARKOUT_FIELDS, STAT, exec_by_module, exec_summary
    stats, marks, info = env.tape_exec(horizons, episode="previous")
    counted = env.tape_counts()["episode"].to(torch.int64) > torch.from_numpy(np.asarray(episode0)).to(env.device, torch.int64)
    n_mod = len(names)
    slot_module = torch.where(counted[:, None], module_of.to(torch.int64), torch.full_like(module_of, n_mod, dtype=torch.int64))      # row n_mod: not counted
    st, mk = exec_by_module(stats, marks, slot_module, n_mod + 1)
    # position-steps per module: every counted slot over the steps 0 .. the market's last non-self fill
    span = (stats[:, :, STAT["last_step"]].max(dim=1).values + 1)[:, None].expand(-1, stats.shape[1]).reshape(-1)
    steps = torch.zeros(n_mod + 1, dtype=torch.int64, device=stats.device).index_add_(0, slot_module.reshape(-1), span)
    st_h, mk_h, steps_h, info_h = st.cpu().numpy(), mk.cpu().numpy(), steps.cpu().numpy(), info.cpu().numpy()
    sel = counted.cpu().numpy()
    out = {"about": {"horizons": list(horizons), "episode": "previous", "markets": int(sel.sum()), "records": int(info_h[sel, 0].sum()),
                     "records_lost": int(info_h[sel, 1].sum()), "partial_markets": int(info_h[sel, 3].sum()), "markout_words": list(MARKOUT_FIELDS)},
           "modules": {}}
    for i, name in enumerate(names):
        block = exec_summary(st_h[i], mk_h[i], horizons=horizons, steps=int(steps_h[i]))
        block["position_steps"] = int(steps_h[i])
        block["stats"] = [int(x) for x in st_h[i]]
        block["markout_rows"] = mk_h[i].tolist()
        out["modules"][name] = block
    if keep is not None:
        keep["execution_tables"] = {"stats": stats.cpu().numpy(), "markouts": marks.cpu().numpy(), "info": info_h, "counted": sel}
    return out


def _spread_report(env, horizons, module_of, names, episode0, keep):
    """evaluate(spread_horizons=...): the spread tables (CDAVecEnv.tape_spreads) of every market's previous episode, folded per module; a market counts as in
    _execution_report."""
    from .quotes import SPREAD_FIELDS, spread_summary, spreads_by_module
    spreads, info = env.tape_spreads(horizons, episode="previous")
    counted = env.tape_counts()["episode"].to(torch.int64) > torch.from_numpy(np.asarray(episode0)).to(env.device, torch.int64)
    n_mod = len(names)
    slot_module = torch.where(counted[:, None], module_of.to(torch.int64), torch.full_like(module_of, n_mod, dtype=torch.int64))      # row n_mod: not counted
    sp_h, info_h, sel = spreads_by_module(spreads, slot_module, n_mod + 1).cpu().numpy(), info.cpu().numpy(), counted.cpu().numpy()
    out = {"about": {"horizons": list(horizons), "episode": "previous", "markets": int(sel.sum()), "tape_records": int(info_h[sel, 0].sum()),
                     "tape_records_lost": int(info_h[sel, 1].sum()), "quotes_lost": int(info_h[sel, 2].sum()), "partial_markets": int((info_h[sel, 3] != 0).sum()),
                     "spread_words": list(SPREAD_FIELDS)},
           "modules": {}}
    for i, name in enumerate(names):
        block = spread_summary(sp_h[i], horizons=horizons)
        block["rows"] = sp_h[i].tolist()
        out["modules"][name] = block
    if keep is not None:
        keep["spread_tables"] = {"spreads": spreads.cpu().numpy(), "info": info_h, "counted": sel}
    return out


def _pnl_report(env, bar_steps, module_of, names, episode0, keep):
    """evaluate(pnl_report=True): the P&L tables (CDAVecEnv.tape_pnl) of every market's previous episode, folded per module by pnl.pnl_by_module; a market counts
    as in _execution_report."""
    from .pnl import PNL_FIELDS, pnl_by_module, pnl_summary
    stats, info = env.tape_pnl(bar_steps, episode="previous")
    counted = env.tape_counts()["episode"].to(torch.int64) > torch.from_numpy(np.asarray(episode0)).to(env.device, torch.int64)
    n_mod = len(names)
    slot_module = torch.where(counted[:, None], module_of.to(torch.int64), torch.full_like(module_of, n_mod, dtype=torch.int64))      # row n_mod: not counted
    st_h, info_h, sel = pnl_by_module(stats, slot_module, n_mod + 1).cpu().numpy(), info.cpu().numpy(), counted.cpu().numpy()
    out = {"about": {"bar_steps": int(bar_steps), "episode": "previous", "markets": int(sel.sum()), "tape_records": int(info_h[sel, 0].sum()),
                     "tape_records_lost": int(info_h[sel, 1].sum()), "quotes_lost": int(info_h[sel, 2].sum()), "partial_markets": int((info_h[sel, 3] != 0).sum()),
                     "pnl_words": list(PNL_FIELDS)},
           "modules": {}}
    for i, name in enumerate(names):
        block = pnl_summary(st_h[i], bar_steps=bar_steps)
        block["row"] = [int(x) for x in st_h[i]]
        out["modules"][name] = block
    if keep is not None:
        keep["pnl_tables"] = {"stats": stats.cpu().numpy(), "info": info_h, "counted": sel}
    return out


STYLISED_HIST_HALF = 16                                              # the return histogram of evaluate(stylised_facts=...): -16 .. 16 ticks, the ends clipped
VARIANCE_RATIO_BARS = 5                                              # ... and, at one-step bars, the longer bar its variance ratio compares against


def _stylised_report(env, lags, bar_steps, episode0, keep):
    """evaluate(stylised_facts=...): the three stylised-facts reductions (CDAVecEnv.quote_returns / tape_signs / tape_flow_returns) of every market's previous
    episode, pooled over the markets that count (as in _execution_report) and read through stylised.summary.  The joined table takes lag 0 and the first seven
    lags; where bar_steps is 1 the variance ratio compares against bars of VARIANCE_RATIO_BARS steps, else bars of one step against bars of bar_steps."""
    from . import stylised as SF
    flow_lags = [0] + list(lags)[:SF.MAX_LAGS - 1]
    top = int(env.market_rows()["max_step"].max()) if env.per_market else int(env.max_step)
    ret = env.quote_returns(lags, bar_steps, hist_half=STYLISED_HIST_HALF, episode="previous")
    other = VARIANCE_RATIO_BARS if int(bar_steps) == 1 else 1
    ret_other = env.quote_returns(lags, other, hist_half=STYLISED_HIST_HALF, episode="previous") if SF.n_points(top, other) <= SF.MAX_BARS else None
    sig = env.tape_signs(lags, episode="previous")
    flo = env.tape_flow_returns(flow_lags, bar_steps, episode="previous")
    counted = env.tape_counts()["episode"].to(torch.int64) > torch.from_numpy(np.asarray(episode0)).to(env.device, torch.int64)

    def pooled(t):                                                   # the sum over the markets that count, on the device; a few hundred words come to the host
        return SF.pool(t[counted]).cpu().numpy()
    r1, rk = (ret, ret_other) if int(bar_steps) == 1 else (ret_other, ret)
    block = SF.summary(returns=[pooled(t) for t in ret[:3]], signs=[pooled(t) for t in sig[:2]], flows=[pooled(t) for t in flo[:2]], lags=lags, flow_lags=flow_lags,
                       bar_steps=bar_steps)
    if ret_other is not None:
        k = max(int(bar_steps), other)
        block["returns"]["variance_ratio"] = {"k": k, "value": SF.variance_ratio(pooled(r1[0]), pooled(rk[0]), k)}
    sel = counted.cpu().numpy()
    qi, ti, fi = ret[3].cpu().numpy(), sig[2].cpu().numpy(), flo[2].cpu().numpy()
    block["about"] = {"lags": list(lags), "flow_lags": flow_lags, "bar_steps": int(bar_steps), "hist_half": STYLISED_HIST_HALF, "episode": "previous",
                      "markets": int(sel.sum()), "quotes": int(qi[sel, 0].sum()), "quotes_lost": int(qi[sel, 1].sum()), "tape_records": int(ti[sel, 0].sum()),
                      "tape_records_lost": int(ti[sel, 1].sum()), "partial_markets": int((fi[sel, 3] != 0).sum())}
    block["rows"] = {"returns": pooled(ret[0]).tolist(), "returns_lagged": pooled(ret[1]).tolist(), "returns_hist": pooled(ret[2]).tolist(),
                     "signs": pooled(sig[0]).tolist(), "signs_lagged": pooled(sig[1]).tolist(), "flows_lagged": pooled(flo[0]).tolist(), "flows": pooled(flo[1]).tolist()}
    if keep is not None:
        keep["stylised_tables"] = {"returns": [t.cpu().numpy() for t in ret], "signs": [t.cpu().numpy() for t in sig], "flows": [t.cpu().numpy() for t in flo],
                                   "counted": sel, "flow_lags": flow_lags}
    return block


BOOK_SHAPE_MAX_DIST, BOOK_SHAPE_HALF = 32, 8                         # evaluate(book_shape_report=True): the shape's distance bins (ticks, the last clipped) and 2 x 8 imbalance bins
BOOK_SHAPE_LAGS, BOOK_SHAPE_OFI_LAGS = (1, 2, 5, 10), (0, 1, 2, 5)   # ... the response curve's lags (steps) and the OFI regression's (bars)


def _book_shape_report(env, bar_steps, keep):
    """evaluate(book_shape_report=True): the three depth reductions (CDAVecEnv.depth_profile / depth_imbalance / depth_ofi) of every market's previous episode,
    pooled over the markets that have one (a book belongs to no module: ONE block) and read through depth.summary, the pooled integer rows beside the figures."""
    from . import depth as D
    L = env.depth_levels
    depths = sorted({1, min(5, L), L})
    prof = env.depth_profile(BOOK_SHAPE_MAX_DIST, episode="previous")
    imb = env.depth_imbalance(BOOK_SHAPE_LAGS, L, BOOK_SHAPE_HALF, episode="previous")
    ofi = env.depth_ofi(BOOK_SHAPE_OFI_LAGS, bar_steps, depths, episode="previous")
    counted = prof[3][:, 0] > 0                                      # the markets whose ring holds something of a finished episode

    def pooled(t):
        return D.pool(t[counted]).cpu().numpy()
    tick = int(env.market_rows()["tick_size"].max()) if env.per_market else int(env.config.get("tick_size", 1))
    block = D.summary(profile=[pooled(t) for t in prof[:3]], imbalance=[pooled(t) for t in imb[:2]], ofi=[pooled(t) for t in ofi[:2]], lags=BOOK_SHAPE_LAGS,
                      ofi_lags=BOOK_SHAPE_OFI_LAGS, depths=depths, tick=tick)
    sel, info = counted.cpu().numpy(), prof[3].cpu().numpy()
    block["about"] = {"levels": L, "max_dist": BOOK_SHAPE_MAX_DIST, "half": BOOK_SHAPE_HALF, "lags": list(BOOK_SHAPE_LAGS), "ofi_lags": list(BOOK_SHAPE_OFI_LAGS),
                      "depths": depths, "bar_steps": int(bar_steps), "episode": "previous", "markets": int(sel.sum()), "records": int(info[sel, 0].sum()),
                      "records_lost": int(info[sel, 1].sum()), "partial_markets": int((info[sel, 3] != 0).sum())}
    block["rows"] = {"profile": pooled(prof[0]).tolist(), "levels": pooled(prof[1]).tolist(), "shape": pooled(prof[2]).tolist(), "response": pooled(imb[0]).tolist(),
                     "imbalance": pooled(imb[1]).tolist(), "ofi_lagged": pooled(ofi[0]).tolist(), "ofi": pooled(ofi[1]).tolist()}
    if keep is not None:
        keep["depth_tables"] = {"profile": [t.cpu().numpy() for t in prof], "imbalance": [t.cpu().numpy() for t in imb], "ofi": [t.cpu().numpy() for t in ofi],
                                "counted": sel, "depths": depths}
    return block


def _order_flow_report(env, module_of, names, with_fills, keep):
    """evaluate(order_flow_report=True): the order-flow table (CDAVecEnv.order_flow) - and, with the trade tape, the fills-against-orders table
    (CDAVecEnv.order_fills) - of every market's previous episode, folded per module through the slot map as tape.exec_by_module folds the execution report (every
    word is additive: one index_add_) and read through order_tape.summary, the integer rows beside the ratios.  A market counts when its ring holds something of a
    finished episode; the others' slots are mapped to no module."""
    from . import order_tape as OT
    flow, info = env.order_flow(episode="previous")
    fills = env.order_fills(episode="previous")[0] if with_fills else None
    counted = info[:, 0] > 0
    n_mod = len(names)
    slot_module = torch.where(counted[:, None], module_of.to(torch.int64), torch.full_like(module_of, n_mod, dtype=torch.int64)).reshape(-1)      # row n_mod: not counted

    def fold(t):
        return torch.zeros((n_mod + 1, t.shape[2]), dtype=torch.int64, device=t.device).index_add_(0, slot_module, t.reshape(-1, t.shape[2])).cpu().numpy()
    fl_h, fi_h, info_h, sel = fold(flow), fold(fills) if with_fills else None, info.cpu().numpy(), counted.cpu().numpy()
    out = {"about": {"episode": "previous", "markets": int(sel.sum()), "records": int(info_h[sel, 0].sum()), "records_lost": int(info_h[sel, 1].sum()),
                     "partial_markets": int((info_h[sel, 3] != 0).sum()), "flow_words": list(OT.FLOW_FIELDS), "fill_words": list(OT.FILL_FIELDS) if with_fills else None},
           "modules": {}}
    for i, name in enumerate(names):
        block = OT.summary(fl_h[i], fi_h[i] if with_fills else None)
        block["flow"] = [int(x) for x in fl_h[i]]
        if with_fills:
            block["fills"] = [int(x) for x in fi_h[i]]
        out["modules"][name] = block
    if keep is not None:
        keep["order_tables"] = {"flow": flow.cpu().numpy(), "fills": fills.cpu().numpy() if with_fills else None, "info": info_h, "counted": sel}
    return out


def evaluate(env, policy, opponents=None, trained_slots=None, episodes=1, mode="greedy", seed=0, groups=None, keep=None, tape=None, tape_capacity=4096,
             exec_horizons=None, quotes=None, spread_horizons=None, stylised_facts=None, bar_steps=1, pnl_report=False, depth=None, depth_levels=10,
             book_shape_report=False, orders=None, order_flow_report=False):
    """Play `policy` (a FusedPolicy or a policy file) on `env` (a CDAVecEnv with auto_reset) for episodes * max_step steps; return per-module results.
    opponents: None = self-play; else a list of "random", FusedPolicy objects, policy files or scripted opponents - "pass", "maker", "taker", "imbalance",
    "NAME:key=value,..." or a scripted.Profile (rule-based agents on the device: their slots carry LEAGUE_RANDOM in slot_net and their profile in the env's slot_script,
    attached for the evaluation and detached afterwards) - or stateful ones - "trend", "value", "execution", "NAME:key=value,..." or a stateful.Profile (opponents
    with memory: attached likewise through set_stateful, on a zeroed state tensor; the result names them in "stateful_modules" and in their module's "module") -,
    placed by slot_modules.  trained_slots: the policy's slots per
    market when there are opponents (default 1).  groups: rollout chains (default 4).  keep (a dict, optional): receives the RolloutChains object, the
    placement, the collected metric tables (agent table, env row) and host copies of every step's env actions (`actions`: category, size_mean, size_sigma,
    price, price_offset as [steps, N, A]) - what a replay needs.
    Every network opponent must have the policy's hidden activation and vf_share_layers setting (the bank's rows are launched by one object's kernels): ValueError
    otherwise, raised before the opponent is loaded and before anything runs.
    tape (a path, optional): record every fill of the evaluated episodes on the device (CDAVecEnv.enable_tape, `tape_capacity` records per market, drained after every
    rollout) and save them as an .npz (tape.save_tape): records i32 [K, 8] with, per record, `market`, `episode` (0 = the first evaluated) and the modules of both
    parties (`init_module`, `counter_module`: indices into `module_names`, the keys of the result's "modules"), plus `dropped` per market (0 unless a market filled
    more than tape_capacity times within one rollout: that raises RuntimeError instead of saving a tape with holes).  The env's tape must be OFF (ValueError
    otherwise: enabling it here would wipe the caller's rings, counters and cursor, and stale every graph captured on the env); it is off again afterwards.
    exec_horizons (step counts, optional; needs `tape`): add an "execution" block to every module of the result - inventory, turnover and mark-outs at these
    horizons (CDAVecEnv.tape_exec on the device, folded per module by tape.exec_by_module, read through tape.exec_summary, the integer rows beside the ratios) -
    and result["execution"], which says what it covers: the PREVIOUS episode on the tape of every market that completed one, i.e. each market's last finished
    episode, with the records lost to the ring (a tape_capacity below an episode's fills) and the open fills reported, not hidden.  Without it the result is
    unchanged, key for key.
    quotes (a path, optional): record the top of the book ahead of every step of the evaluated episodes on the device (CDAVecEnv.enable_quotes, two episodes of
    capacity) and save every market's last finished episode as an .npz (quotes.save): records i32 [N, max_step, 8] with `counts`, `info` (quote_series' rows), the
    slot -> module map `modules` and `module_names`.  The env's quote tape must be OFF (ValueError otherwise); it is off again afterwards.
    spread_horizons (step counts, optional; needs `tape`; the quotes are recorded whether or not `quotes` names a file): add a "spreads" block to every module -
    effective and realised half-spread and impact per share, by role (CDAVecEnv.tape_spreads, folded by quotes.spreads_by_module, read through
    quotes.spread_summary, the integer rows beside the ratios) - and result["spreads"], which says what it covers, as the execution report does.
    stylised_facts (lags, optional; bar_steps: the bar size, in env steps): switch BOTH tapes on for the evaluated episodes - with or without a `tape` / `quotes`
    file - and add result["stylised_facts"]: the return, order-flow-sign and flow-return statistics of every market's last finished episode (CDAVecEnv.quote_returns,
    tape_signs, tape_flow_returns on the device), pooled over the markets (stylised.pool) and read through stylised.summary - autocorrelations of returns and of
    their magnitudes, the leverage correlation, variance ratio, excess kurtosis, sign autocorrelation, Kyle's lambda and R^2 per lag - with the pooled integer rows
    beside the figures and what they cover ("about"), records lost to a ring reported, not hidden.
    pnl_report (needs `tape`; the quotes are recorded whether or not `quotes` names a file; bar_steps: the bar size): add a "pnl" block to every module - what its
    slots' mark-to-mid P&L did over every market's last finished episode: P&L and its split into inventory and trading, drawdown, bar P&L mean / std, Sharpe, hit
    ratio, time under water (CDAVecEnv.tape_pnl on the device, folded by pnl.pnl_by_module, read through pnl.pnl_summary, the integer row beside the figures) -
    and result["pnl"], which says what it covers, as the spread report does.
    depth (a path, optional; depth_levels: the levels per side, 1 .. 16): record the Level-2 ladder ahead of every step of the evaluated episodes on the device
    (CDAVecEnv.enable_depth, two episodes of capacity; neither other tape is needed) and save every market's last finished episode as an .npz (depth.save): records
    i32 [N, max_step, (1 + levels) * 4] with `levels`, `counts`, `info`, `modules` and `module_names`.  The env's depth tape must be OFF; it is off again afterwards.
    book_shape_report (the ladders are recorded whether or not `depth` names a file; bar_steps: the OFI's bar size): add result["depth"] - the average shape of the
    book, the future mid move given the depth imbalance and the multi-level order-flow-imbalance regression of every market's last finished episode
    (CDAVecEnv.depth_profile, depth_imbalance, depth_ofi on the device), pooled over the markets (a book belongs to no module) and read through depth.summary,
    with the pooled integer rows and what they cover ("about").
    orders (a path, optional): record every decoded order and its execution rank ahead of every step of the evaluated episodes on the device
    (CDAVecEnv.enable_order_tape, two episodes of capacity) and save every market's last finished episode as an .npz (order_tape.save): records i32 [N, max_step,
    (1 + A) * 4] with `counts`, `info`, `modules` and `module_names`.  The env's order tape must be OFF; it is off again afterwards.
    order_flow_report (the orders are recorded whether or not `orders` names a file): add result["orders"] and one "orders" block per module - what the module's slots
    sent, how they priced it against the touch and, with tape=..., how much of it found liquidity at once (CDAVecEnv.order_flow / order_fills on the device, folded
    through the slot map, read through order_tape.summary)."""
    from .mlp import LEAGUE_RANDOM, FusedPolicy, PolicyBank, RolloutChains, read_policy
    if mode not in ("greedy", "sample"):
        raise ValueError(f"mode must be 'greedy' or 'sample' (got {mode!r})")
    if not bool(env.config.get("auto_reset", False)):
        raise ValueError("evaluate needs an auto_reset env")
    if exec_horizons is not None:
        from .tape import _horizons
        exec_horizons = _horizons(exec_horizons)
        if tape is None:
            raise ValueError("evaluate(exec_horizons=...) reads the trade tape of the evaluated episodes: pass tape=FILE.npz as well (the tape is off by default)")
    if spread_horizons is not None:
        from .quotes import _horizons as _spread_hz
        spread_horizons = _spread_hz(spread_horizons)
        if tape is None:
            raise ValueError("evaluate(spread_horizons=...) joins the trade tape of the evaluated episodes to their quotes: pass tape=FILE.npz as well")
    if pnl_report:
        from .stylised import MAX_BARS, _bar_steps, n_points
        if tape is None:
            raise ValueError("evaluate(pnl_report=True) joins the trade tape of the evaluated episodes to their quotes: pass tape=FILE.npz as well")
        bar_steps = _bar_steps(bar_steps)
        top = int(env.market_rows()["max_step"].max()) if env.per_market else int(env.max_step)
        if n_points(top, bar_steps) > MAX_BARS:
            raise ValueError(f"evaluate(pnl_report=True): an episode of {top} steps has more than {MAX_BARS} bars of {bar_steps} steps: raise bar_steps")
    if stylised_facts is not None:
        from .stylised import MAX_BARS, _bar_steps, _lags, n_points
        stylised_facts, bar_steps = _lags(stylised_facts, 1), _bar_steps(bar_steps)
        top = int(env.market_rows()["max_step"].max()) if env.per_market else int(env.max_step)
        if n_points(top, bar_steps) > MAX_BARS:
            raise ValueError(f"evaluate(stylised_facts=...): an episode of {top} steps has more than {MAX_BARS} bars of {bar_steps} steps: raise bar_steps")
    with_depth = depth is not None or bool(book_shape_report)
    if with_depth:
        from .depth import _levels as _depth_levels
        from .stylised import MAX_BARS, _bar_steps, n_points
        depth_levels, bar_steps = _depth_levels(depth_levels), _bar_steps(bar_steps)
        top = int(env.market_rows()["max_step"].max()) if env.per_market else int(env.max_step)
        if book_shape_report and n_points(top, bar_steps) > MAX_BARS:
            raise ValueError(f"evaluate(book_shape_report=True): an episode of {top} steps has more than {MAX_BARS} bars of {bar_steps} steps: raise bar_steps")
        if env.depth_enabled:
            raise ValueError("evaluate(depth=... / book_shape_report=True) needs an env whose depth tape is off: it enables one of its own for the evaluated episodes "
                             "(disable_depth() first)")
    with_orders = orders is not None or bool(order_flow_report)
    if with_orders and env.order_tape_enabled:
        raise ValueError("evaluate(orders=... / order_flow_report=True) needs an env whose order tape is off: it enables one of its own for the evaluated episodes "
                         "(disable_order_tape() first)")
    with_tape = tape is not None or stylised_facts is not None
    with_quotes = quotes is not None or spread_horizons is not None or stylised_facts is not None or bool(pnl_report)
    if with_quotes and env.quotes_enabled:
        raise ValueError("evaluate(quotes=... / spread_horizons=... / stylised_facts=...) needs an env whose quote tape is off: it enables one of its own for the evaluated episodes "
                         "(disable_quotes() first)")
    dev, N, A = env.device, env.n_markets, env.num_agents
    pol = _as_policy(policy, dev)
    opp = None if opponents is None else list(opponents)
    if opp is not None and len(opp) == 0:
        raise ValueError("opponents: None (self-play) or a non-empty list")
    nets = []                                                           # (opponent index, FusedPolicy) of the network opponents
    from .scripted import is_scripted_spec, parse_profile
    scripts = {p: parse_profile(o) for p, o in enumerate(opp or []) if is_scripted_spec(o)}      # opponent index -> Profile (a bad 'NAME:key=value' raises here)
    if scripts and env.scripted:
        raise ValueError("evaluate() with scripted opponents needs an env without scripts attached: it attaches its own for the evaluated episodes (clear_scripted() first)")
    from . import stateful as SF
    statefuls = {p: SF.parse_profile(o) for p, o in enumerate(opp or []) if SF.is_stateful_spec(o)}      # opponent index -> stateful.Profile
    if statefuls and env.stateful:
        raise ValueError("evaluate() with stateful opponents needs an env without stateful opponents attached: it attaches its own for the evaluated episodes "
                         "(clear_stateful() first)")
    for p, o in enumerate(opp or []):
        if (isinstance(o, str) and o == RANDOM) or p in scripts or p in statefuls:
            continue
        act, vfs = (o.activation, o.vf_share_layers) if isinstance(o, FusedPolicy) else read_policy(o, with_activation=True, with_vf_share_layers=True)[1:]
        if act != pol.activation:
            raise ValueError(f"opponent {p} is a {act} network, the policy a {pol.activation} one: a bank holds networks of one activation")
        if vfs != pol.vf_share_layers:
            raise ValueError(f"opponent {p} has vf_share_layers = {vfs}, the policy {pol.vf_share_layers}: a bank holds networks of one setting")
        op = _as_policy(o, dev)
        if op.L.hist != pol.L.hist:
            raise ValueError(f"opponent {p} is laid out for n_hist = {op.L.hist}, the policy for {pol.L.hist}")
        nets.append((p, op))
    k = (A if opp is None else 1) if trained_slots is None else int(trained_slots)
    modules = slot_modules(N, A, k, 0 if opp is None else len(opp))
    names = ["policy"] + [f"opponent_{p}" for p in range(len(opp or []))]

    total = int(episodes) * int(env.max_step)
    if total < 1:
        raise ValueError("episodes * max_step must be at least 1")
    T = _horizon(total)
    prev_metrics = bool(getattr(env, "episode_metrics_on", False))       # the caller's setting, tolerance included: put back as it was afterwards
    prev_tolerance = float(getattr(env, "episode_metrics_tolerance", 1e-6))
    env.enable_episode_metrics(True)                                    # before the chains are captured
    if with_tape and env.tape_enabled:
        raise ValueError("evaluate(tape=... / stylised_facts=...) needs an env whose trade tape is off: it enables a tape of its own for the evaluated episodes (disable_tape() first, or "
                         "drain the running tape yourself with drain_tape(cursor=...))")
    if with_tape:
        env.enable_tape(tape_capacity)                                  # (likewise: the chains' graphs hold the tape-writing step instances)
    if with_quotes:
        env.enable_quotes(min(1 << 20, 2 * max(1, int(env.max_step))))  # (likewise: the recorder's launch; the finished episode and the running one both fit)
    if with_depth:
        env.enable_depth(min(1 << 20, 2 * max(1, int(env.max_step))), depth_levels)      # (likewise)
    if with_orders:
        env.enable_order_tape(min(1 << 20, 1 << (2 * max(1, int(env.max_step)) - 1).bit_length()))      # (likewise; a power of two that holds two episodes)
    tape_parts, tape_dropped = [], np.zeros(N, np.int64)
    try:
        if opp is None:
            driver = pol
        else:
            bank = PolicyBank(dev, N, A, n_trainable=1, max_frozen=max(1, len(nets)), random_seed=seed, n_hist=pol.L.hist,
                              activation=pol.activation, vf_share_layers=pol.vf_share_layers)
            bank.theta[0].copy_(pol.theta)
            bank.wb[0].copy_(pol.wb)
            row_of = {}
            for p, op in nets:
                row = bank.n_trainable + bank.n_frozen
                bank.n_frozen += 1
                bank.theta[row].copy_(op.theta)
                bank.wb[row].copy_(op.wb)
                row_of[p] = row
            bank._refresh()
            slot_net = np.zeros((N, A), dtype=np.int32)
            for p in range(len(opp)):
                slot_net[modules == 1 + p] = row_of.get(p, LEAGUE_RANDOM)
            bank.set_slots(torch.from_numpy(slot_net))
            driver = bank
            if scripts:                                                  # the scripted modules' slots: the random module in slot_net, their profile in slot_script
                order = sorted(scripts)
                slot_script = np.zeros((N, A), dtype=np.int32)
                for j, p in enumerate(order):
                    slot_script[modules == 1 + p] = 1 + j
                env.set_scripted(slot_script, [scripts[p] for p in order], seed=seed)      # before the chains are captured
            if statefuls:                                                # likewise the stateful modules': the random module in slot_net, their profile in the stateful table
                order = sorted(statefuls)
                slot_stateful = np.zeros((N, A), dtype=np.int32)
                for j, p in enumerate(order):
                    slot_stateful[modules == 1 + p] = 1 + j
                env.set_stateful(slot_stateful, [statefuls[p] for p in order], seed=seed)   # (a zeroed state tensor: every slot starts fresh)
        seeds = (np.uint64(int(seed) & (2 ** 63 - 1)) * np.uint64(N) + np.arange(N, dtype=np.uint64))
        env.reset(seed=seeds)
        env.collect_episode_metrics(clear=True)                          # nothing that ended before the reset counts
        chains = RolloutChains(env, driver, T, groups=4 if groups is None else int(groups), seed=seed, greedy=mode == "greedy")
        acts = [] if keep is not None else None
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for c in range(total // T):
            before = {k: v.cpu().numpy() for k, v in env.tape_counts().items()} if with_tape else None
            if with_tape and c == 0:
                tape_ep0 = before["episode"].copy()                      # the first evaluated episode of every market
            buf = chains.run()
            if tape is not None:
                rows, off, dropped = (x.cpu().numpy() for x in env.drain_tape())
                after = {k: v.cpu().numpy() for k, v in env.tape_counts().items()}
                market = np.repeat(np.arange(N, dtype=np.int32), np.diff(off))
                tape_parts.append((rows, market, _tape_episodes(rows, off, before, after) - tape_ep0[market]))
                if int(dropped.sum()) > 0:                            # (rows are missing: neither the tape nor the ids derived from the counters could be trusted)
                    raise RuntimeError(f"evaluate(tape=...): {int(dropped.sum())} fills were overwritten before they were drained - tape_capacity {tape_capacity} is "
                                       f"too small for a rollout of {T} steps")
            if acts is not None:
                acts.append({key: buf[key].cpu() for key in ("category", "size_mean", "size_sigma", "price", "price_offset")})
        torch.cuda.synchronize(dev)
        wall = time.perf_counter() - t0
        module_of = torch.from_numpy(modules).to(dev).contiguous()
        table, env_row = env.collect_episode_metrics(module_of=module_of, n_modules=len(names), clear=True)
        execution = None
        if exec_horizons is not None:
            execution = _execution_report(env, exec_horizons, module_of, names, tape_ep0, keep)
        spread_rep = None
        if spread_horizons is not None:
            spread_rep = _spread_report(env, spread_horizons, module_of, names, tape_ep0, keep)
        stylised_rep = None
        if stylised_facts is not None:
            stylised_rep = _stylised_report(env, stylised_facts, bar_steps, tape_ep0, keep)
        pnl_rep = None
        if pnl_report:
            pnl_rep = _pnl_report(env, bar_steps, module_of, names, tape_ep0, keep)
        depth_rep = None
        if book_shape_report:
            depth_rep = _book_shape_report(env, bar_steps, keep)
        order_rep = None
        if order_flow_report:
            order_rep = _order_flow_report(env, module_of, names, tape is not None, keep)
        if orders is not None:
            from .order_tape import save as save_orders
            rec, cnt, oinfo = env.order_tape_series(int(env.max_step), episode="previous")
            save_orders(orders, rec, counts=cnt, info=oinfo, modules=modules.astype(np.int32), module_names=np.array(names))
        if depth is not None:
            from .depth import save as save_depth
            rec, cnt, dinfo = env.depth_series(int(env.max_step), episode="previous")
            save_depth(depth, rec, depth_levels, counts=cnt, info=dinfo, modules=modules.astype(np.int32), module_names=np.array(names))
        if quotes is not None:
            from .quotes import save as save_quotes
            rec, cnt, qinfo = env.quote_series(int(env.max_step), episode="previous")
            save_quotes(quotes, rec, counts=cnt, info=qinfo, modules=modules.astype(np.int32), module_names=np.array(names))
        if tape is not None:
            from .tape import save_tape
            rows = np.concatenate([p[0] for p in tape_parts]) if tape_parts else np.zeros((0, 8), np.int32)
            market = np.concatenate([p[1] for p in tape_parts]) if tape_parts else np.zeros(0, np.int32)
            save_tape(tape, rows, dropped=tape_dropped, market=market, episode=np.concatenate([p[2] for p in tape_parts]) if tape_parts else np.zeros(0, np.int32),
                      init_module=modules[market, rows[:, 6]].astype(np.int32), counter_module=modules[market, rows[:, 3]].astype(np.int32),
                      module_names=np.array(names), modules=modules.astype(np.int32))
    finally:
        env.enable_episode_metrics(prev_metrics, nav_tolerance=prev_tolerance)
        if with_tape:
            env.disable_tape()
        if with_quotes and env.quotes_enabled:
            env.disable_quotes()
        if with_depth and env.depth_enabled:
            env.disable_depth()
        if with_orders and env.order_tape_enabled:
            env.disable_order_tape()
        if scripts and env.scripted:
            env.clear_scripted()
        if statefuls and env.stateful:
            env.clear_stateful()
    table_h, env_h = table.cpu().numpy(), env_row.cpu().numpy()
    summary = summarise(table_h, env_h, module_names=names)
    check_nav_conservation(0, summary, strict=True)
    mods = {}
    for i, name in enumerate(names):
        r = table_h[i]
        s = summary["modules"].get(name, {"agent_episodes": 0.0})
        mods[name] = {"agent_episodes": s["agent_episodes"], "episode_return_mean": s.get("episode_return_mean"), "episode_return_std": s.get("episode_return_std"),
                      "episode_nav_mean": s.get("episode_nav_mean"), "trades": float(r[K.EM_TRADES]), "rejections": float(r[K.EM_REJECTIONS]),
                      "maker_fill_ratio_mean": s.get("maker_fill_ratio_mean"),
                      "reward_term_sums": {t: float(r[K.EM_TERM_SUM + j]) for j, t in enumerate(REWARD_TERMS)},
                      "slots": int((modules == i).sum())}
    result = {"mode": mode, "episodes": summary["episodes"], "nav_conservation_violations": summary["nav_conservation_violations"], "modules": mods,
              "config": {"markets": N, "agents": A, "max_step": int(env.max_step), "episodes": int(episodes), "steps": total, "horizon": T, "seed": int(seed),
                         "trained_slots": k, "opponents": None if opp is None else [_describe(o) for o in opp], "n_hist": pol.L.hist,
                         "activation": pol.activation},
              "agent_steps_per_s": N * A * total / wall if wall > 0 else None,
              "summary": summary}
    if statefuls:                                                        # the stateful modules by name: stateful_<index among them>_<law>
        result["stateful_modules"] = {}
        for j, p in enumerate(sorted(statefuls)):
            mods[f"opponent_{p}"]["module"] = result["stateful_modules"][f"opponent_{p}"] = SF.module_id(j, statefuls[p])
    if execution is not None:
        result["execution"] = execution["about"]
        for name in names:
            mods[name]["execution"] = execution["modules"][name]
    if spread_rep is not None:
        result["spreads"] = spread_rep["about"]
        for name in names:
            mods[name]["spreads"] = spread_rep["modules"][name]
    if stylised_rep is not None:
        result["stylised_facts"] = stylised_rep
    if pnl_rep is not None:
        result["pnl"] = pnl_rep["about"]
        for name in names:
            mods[name]["pnl"] = pnl_rep["modules"][name]
    if depth_rep is not None:
        result["depth"] = depth_rep
    if order_rep is not None:
        result["orders"] = order_rep["about"]
        for name in names:
            mods[name]["orders"] = order_rep["modules"][name]
    if keep is not None:
        keep["chains"], keep["modules"], keep["tables"] = chains, modules, (table_h, env_h)
        keep["actions"] = {key: torch.cat([a[key] for a in acts]) for key in acts[0]}
    return result


def main(argv=None):
    p = argparse.ArgumentParser(description="evaluate a saved policy (greedy by default) against opponents on the HIP env")
    p.add_argument("--policy", required=True, help="a policy file (ppo --save, league_train --save-dir)")
    p.add_argument("--opponent", action="append", default=None, help="'random', a scripted opponent ('pass', 'maker', 'taker', 'imbalance', 'NAME:key=value,...'), one with memory ('trend', 'value', 'execution', 'NAME:key=value,...') or a policy file; repeat for several (market m plays opponent m mod P); none = self-play")
    p.add_argument("--markets", type=int, default=1024)
    p.add_argument("--agents", type=int, default=4)
    p.add_argument("--max-step", type=int, default=256)
    p.add_argument("--episodes", type=int, default=1)
    p.add_argument("--trained-slots", type=int, default=None, help="slots per market the policy plays when there are opponents (default 1)")
    p.add_argument("--sample", action="store_true", help="sample actions (the training kernels) instead of the greedy mode")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=None, help="also write the JSON result to this file")
    p.add_argument("--tape", default=None, metavar="FILE.npz", help="record every fill of the evaluated episodes (the trade tape) and save the records with their market, episode and module ids")
    p.add_argument("--exec-report", default=None, metavar="K[,K...]", help="with --tape: add per-module inventory, turnover and mark-outs at these step horizons, reduced "
                   "on the device from every market's last finished episode")
    p.add_argument("--quotes", default=None, metavar="FILE.npz", help="record the top of the book ahead of every step (the quote tape) and save every market's last finished episode")
    p.add_argument("--spread-report", default=None, metavar="K[,K...]", help="with --tape: add per-module effective spread, realised spread and impact per share at these step "
                   "horizons, by role - the trade tape joined to the quotes on the device")
    p.add_argument("--stylised-facts", default=None, metavar="L[,L...]", help="add the stylised-facts block - return autocorrelations, volatility clustering, tails, order-flow "
                   "sign persistence, price impact of signed volume - at these lags, reduced on the device from every market's last finished episode (switches the trade "
                   "tape and the quote tape on)")
    p.add_argument("--bar-steps", type=int, default=1, metavar="K", help="with --stylised-facts / --pnl-report / --book-shape-report: the bar size in env steps (default 1)")
    p.add_argument("--pnl-report", action="store_true", help="with --tape: add per-module P&L, its inventory / trading split, drawdown, bar P&L moments, Sharpe and hit "
                   "ratio - every agent's mark-to-mid equity curve, reduced on the device from every market's last finished episode (switches the quote tape on)")
    p.add_argument("--depth", default=None, metavar="FILE.npz", help="record the Level-2 ladder ahead of every step (the depth tape) and save every market's last finished episode")
    p.add_argument("--depth-levels", type=int, default=10, metavar="L", help="with --depth / --book-shape-report: price levels per side, 1 .. 16 (default 10)")
    p.add_argument("--book-shape-report", action="store_true", help="add the pooled depth block - the average shape of the book, the mid's response to depth imbalance and "
                   "the multi-level order-flow-imbalance regression (bars of --bar-steps), reduced on the device from every market's last finished episode (switches the "
                   "depth tape on)")
    p.add_argument("--orders", default=None, metavar="FILE.npz", help="record every decoded order and its execution rank ahead of every step (the order tape) and save every "
                   "market's last finished episode")
    p.add_argument("--order-flow-report", action="store_true", help="add one orders block per module - what it sent, how it priced it against the touch and, with --tape, how "
                   "much of it filled at once - reduced on the device from every market's last finished episode (switches the order tape on)")
    p.add_argument("--order-schedule", default=None, metavar="FILE.npz", help="attach this order schedule (orders.save_schedule) to the env: per-step order flow played ahead "
                   "of every step of the evaluated episodes")
    args = p.parse_args(argv)
    exec_horizons = None
    if args.exec_report is not None:
        if args.tape is None:
            p.error("--exec-report reads the trade tape: give --tape FILE.npz as well")
        try:
            exec_horizons = [int(k) for k in args.exec_report.split(",")]
        except ValueError:
            p.error(f"--exec-report takes step counts separated by commas, got {args.exec_report!r}")
    spread_horizons = None
    if args.spread_report is not None:
        if args.tape is None:
            p.error("--spread-report joins the trade tape to the quotes: give --tape FILE.npz as well")
        try:
            spread_horizons = [int(k) for k in args.spread_report.split(",")]
        except ValueError:
            p.error(f"--spread-report takes step counts separated by commas, got {args.spread_report!r}")
    if args.pnl_report and args.tape is None:
        p.error("--pnl-report joins the trade tape to the quotes: give --tape FILE.npz as well")
    stylised_facts = None
    if args.stylised_facts is not None:
        try:
            stylised_facts = [int(k) for k in args.stylised_facts.split(",")]
        except ValueError:
            p.error(f"--stylised-facts takes lags separated by commas, got {args.stylised_facts!r}")
    from .mlp import layout_of_params, read_policy
    from .vec_env import CDAVecEnv
    n_hist = layout_of_params(read_policy(args.policy).numel()).hist             # (the hidden activation comes with the file: load_policy)
    env = CDAVecEnv({"num_of_agents": args.agents, "init_cash": 1000000, "max_step": args.max_step, "is_render": False, "auto_reset": True, "n_hist": n_hist},
                    n_markets=args.markets, device="cuda:0", with_info=False)
    try:
        if args.order_schedule:
            env.load_order_schedule(args.order_schedule)
        res = evaluate(env, args.policy, opponents=args.opponent, trained_slots=args.trained_slots, episodes=args.episodes,
                       mode="sample" if args.sample else "greedy", seed=args.seed, tape=args.tape, exec_horizons=exec_horizons,
                       quotes=args.quotes, spread_horizons=spread_horizons, stylised_facts=stylised_facts, bar_steps=args.bar_steps, pnl_report=args.pnl_report,
                       depth=args.depth, depth_levels=args.depth_levels, book_shape_report=args.book_shape_report,
                       orders=args.orders, order_flow_report=args.order_flow_report)
    finally:
        env.close()
    res.pop("summary")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
