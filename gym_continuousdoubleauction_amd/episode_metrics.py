"""What the reference's callback reports around an episode, from the device-side accumulators (include/cda.h cda_episode_metrics_*).

Reference: train/callbk/league_based_self_play_callback.py - `_log_activity` :295-342 (pass / rejection fractions), `_log_maker_ratio` :344-372,
`_log_reward_terms` :374-416 (mean and variance share of the five reward terms), `_log_episode_account` :418-470 (NAV mean / min / max, drawdown, inventory,
trades at the episode's last step), `on_episode_end` :627-755 (sum of NAV == num_agents x init_cash, `nav_conservation_violations`), and the driver's half of
the check, train/train.py:1109-1164 (`_check_nav_conservation`: a violation stops a `strict_nav_check` run with NavConservationError).

The reference logs one value per EPISODE and lets RLlib's MetricsLogger average a window of ten; a batch of N markets ends N episodes at once, so the figures
here are the means over the episodes that ended since the last collection (sums of the per-episode numerators and denominators where the reference's own
statistic is a ratio of sums, e.g. the fractions of one episode)."""
import json

import numpy as np

from . import _capi as K

REWARD_TERMS = ("nav", "order", "trade", "drawdown", "passive")      # reward_helper.py:75-81, the order of info["reward_terms"]


class NavConservationError(AssertionError):
    """A run stopped because the NAV conservation invariant broke (train/train.py:1100-1107)."""


def _row(r, terms=REWARD_TERMS):
    n = float(r[K.EM_EPISODES])
    if n <= 0:
        return None
    steps = float(r[K.EM_AGENT_STEPS])
    out = {"agent_episodes": n, "agent_steps": steps}
    if steps > 0:
        out["pass_action_fraction"] = float(r[K.EM_PASSES]) / steps
        out["order_rejection_fraction"] = float(r[K.EM_REJECTIONS]) / steps
        out["orders_placed_fraction"] = float(r[K.EM_PLACED]) / steps
        var = {}
        for j, t in enumerate(terms):
            mean = float(r[K.EM_TERM_SUM + j]) / steps
            var[t] = max(0.0, float(r[K.EM_TERM_SQ + j]) / steps - mean * mean)          # E[x^2] - E[x]^2, clamped (:399-404)
            out[f"reward_term_mean_{t}"] = mean
        total = sum(var.values())
        if total > 0.0:
            for t in terms:
                out[f"reward_term_var_share_{t}"] = var[t] / total
    trades = float(r[K.EM_TRADES])
    out["trades"], out["passive_fills"] = trades, float(r[K.EM_PASSIVE])
    mean_ret = float(r[K.EM_RETURN_SUM]) / n
    out["episode_return_mean"] = mean_ret
    out["episode_return_std"] = max(0.0, float(r[K.EM_RETURN_SQ]) / n - mean_ret * mean_ret) ** 0.5
    out["episode_nav_mean"], out["episode_nav_min"], out["episode_nav_max"] = float(r[K.EM_NAV_SUM]) / n, float(r[K.EM_NAV_MIN]), float(r[K.EM_NAV_MAX])
    out["mean_agent_drawdown"] = float(r[K.EM_DRAWDOWN_SUM]) / n
    out["mean_abs_net_position"] = float(r[K.EM_ABS_POSITION_SUM]) / n
    out["mean_num_trades"] = float(r[K.EM_NUM_TRADES_SUM]) / n
    if r[K.EM_MAKER_RATIO_N] > 0:
        out["maker_fill_ratio_mean"] = float(r[K.EM_MAKER_RATIO_SUM]) / float(r[K.EM_MAKER_RATIO_N])
        out["maker_fill_ratio_best"] = float(r[K.EM_MAKER_RATIO_MAX])
    out["bankrupt_fraction"] = float(r[K.EM_BANKRUPT]) / n
    return out


def summarise(agent_table, env_row, module_names=None):
    """agent_table f64 [n_modules, EM_AGENT_FIELDS], env_row f64 [EM_ENV_FIELDS] (device or host) -> {"episodes", "nav_conservation_violations",
    "nav_conservation_error", ..., "all": {...the callback's per-episode metrics over every agent...}, "modules": {name: {...}}}"""
    t = agent_table.detach().cpu().numpy() if hasattr(agent_table, "detach") else np.asarray(agent_table)
    e = env_row.detach().cpu().numpy() if hasattr(env_row, "detach") else np.asarray(env_row)
    out = {"episodes": float(e[K.EM_ENV_EPISODES]), "nav_conservation_violations": float(e[K.EM_ENV_NAV_VIOLATIONS]),
           "nav_conservation_error": float(e[K.EM_ENV_NAV_ERROR_MAX]), "nav_conservation_error_sum": float(e[K.EM_ENV_NAV_ERROR_SUM])}
    if e[K.EM_ENV_EPISODES] > 0:
        out["episode_len_mean"] = float(e[K.EM_ENV_STEPS]) / float(e[K.EM_ENV_EPISODES])
        out["terminated_fraction"] = float(e[K.EM_ENV_TERMINATED]) / float(e[K.EM_ENV_EPISODES])
    if e[K.EM_ENV_MAKER_MAX_N] > 0:
        out["maker_fill_ratio_max"] = float(e[K.EM_ENV_MAKER_MAX_SUM]) / float(e[K.EM_ENV_MAKER_MAX_N])      # mean over the episodes of their most maker-like agent (:344-372)
    allr = _row(_merge_agent_rows([t[i:i + 1] for i in range(t.shape[0])])[0]) if t.shape[0] else None      # every module folded into one row, by the one merge rule
    if allr is not None:
        out["all"] = allr
    names = list(module_names) if module_names is not None else [f"module_{i}" for i in range(t.shape[0])]
    mods = {}
    for i in range(min(t.shape[0], len(names))):
        r = _row(t[i])
        if r is not None:
            mods[names[i]] = r
    out["modules"] = mods
    return out


# ---- one merge rule: how two tables of cda_episode_metrics_collect become one (the device's em_combine / em_identity and the env row's fmax, restated by column) ----
AGENT_MIN_COLUMNS = (K.EM_NAV_MIN,)                                  # identity +inf
AGENT_MAX_COLUMNS = (K.EM_NAV_MAX, K.EM_MAKER_RATIO_MAX)             # identity -inf
ENV_MAX_COLUMNS = (K.EM_ENV_NAV_ERROR_MAX,)                          # identity 0 (an absolute error)
AGENT_SUM_COLUMNS = tuple(f for f in range(K.EM_AGENT_FIELDS) if f not in AGENT_MIN_COLUMNS + AGENT_MAX_COLUMNS)
ENV_SUM_COLUMNS = tuple(f for f in range(K.EM_ENV_FIELDS) if f not in ENV_MAX_COLUMNS)


def _host(x):
    return np.array(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def _with_identities(a):
    """a copy of an agent table in which a module that played nothing (EM_EPISODES == 0: k_em_final reports zeros for it) holds the identities of MIN and MAX;
    works on numpy arrays and torch tensors alike"""
    a = a.clone() if hasattr(a, "clone") else a.copy()
    idle = ~(a[:, K.EM_EPISODES] > 0)
    for f in AGENT_MIN_COLUMNS:
        a[idle, f] = float("inf")
    for f in AGENT_MAX_COLUMNS:
        a[idle, f] = float("-inf")
    return a


def _merge_agent_rows(tables):
    """agent tables f64 [M, EM_AGENT_FIELDS] (numpy) -> their merge [M, EM_AGENT_FIELDS]: MIN / MAX over the tables in which the module played, SUM elsewhere.  A
    module that played in none keeps the first table's words in the MIN / MAX columns (k_em_final's zeros - or the raw identities, untouched)"""
    stack = np.stack([_with_identities(a) for a in tables])
    out = stack.sum(axis=0)
    for f in AGENT_MIN_COLUMNS:
        out[:, f] = stack[:, :, f].min(axis=0)
    for f in AGENT_MAX_COLUMNS:
        out[:, f] = stack[:, :, f].max(axis=0)
    idle = ~(out[:, K.EM_EPISODES] > 0)
    for f in AGENT_MIN_COLUMNS + AGENT_MAX_COLUMNS:
        out[idle, f] = tables[0][idle, f]
    return out


def merge_tables(tables):
    """[(agent_table [M, EM_AGENT_FIELDS], env_row [EM_ENV_FIELDS]), ...] of the same modules (device or host) -> the one (agent_table, env_row), f64 numpy, that a
    collection over the union of their markets gives: em_combine by column - MIN for EM_NAV_MIN, MAX for EM_NAV_MAX, EM_MAKER_RATIO_MAX and EM_ENV_NAV_ERROR_MAX, SUM for
    every other column (the sums in list order).  A table in which a module played nothing (zeros) does not touch that module's MIN / MAX; infinities pass through."""
    tables = [(_host(a), _host(e)) for a, e in tables]
    if not tables:
        raise ValueError("merge_tables needs at least one (agent_table, env_row)")
    if any(a.shape != tables[0][0].shape or e.shape != tables[0][1].shape for a, e in tables):
        raise ValueError("merge_tables: the tables must cover the same modules (equal shapes)")
    env = np.stack([e for _, e in tables])
    out_env = env.sum(axis=0)
    for f in ENV_MAX_COLUMNS:
        out_env[f] = env[:, f].max()
    return _merge_agent_rows([a for a, _ in tables]), out_env


def check_allreduce(allreduce):
    """TypeError unless `allreduce` takes op= ("sum" / "min" / "max": parallel.make_grad_allreduce's callable): the tables' MIN and MAX columns must not be summed"""
    import inspect
    try:
        params = inspect.signature(allreduce).parameters
    except (TypeError, ValueError):
        params = {}
    if "op" not in params and not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values()):
        raise TypeError("episode metrics over data-parallel ranks need an all-reduce that can take the minimum and the maximum: a callable(tensor, op='sum' | 'min' | "
                        "'max') such as parallel.make_grad_allreduce's. This one takes no `op`; summing the min / max columns would report wrong figures "
                        "(or pass episode_metrics=False)")


def allreduce_tables(em, allreduce):
    """merge_tables over the ranks of a data-parallel run: em = this rank's (agent_table, env_row), allreduce(tensor, op=) reduces in place over the ranks.  Three
    collectives (the SUM, MIN and MAX columns packed into one tensor each); returns new torch tensors on em's device, equal on every rank."""
    import torch
    check_allreduce(allreduce)
    agent, env = torch.as_tensor(em[0]), torch.as_tensor(em[1])
    a = _with_identities(agent)
    M = a.shape[0]
    packs = {"sum": torch.cat([a[:, list(AGENT_SUM_COLUMNS)].reshape(-1), env[list(ENV_SUM_COLUMNS)]]),
             "min": a[:, list(AGENT_MIN_COLUMNS)].reshape(-1).clone(),
             "max": torch.cat([a[:, list(AGENT_MAX_COLUMNS)].reshape(-1), env[list(ENV_MAX_COLUMNS)]])}
    for op in ("sum", "min", "max"):                        # (one fixed order on every rank)
        allreduce(packs[op], op=op)
    out_a, out_e = torch.empty_like(a), torch.empty_like(env)
    ns, nx = M * len(AGENT_SUM_COLUMNS), M * len(AGENT_MAX_COLUMNS)
    out_a[:, list(AGENT_SUM_COLUMNS)] = packs["sum"][:ns].view(M, -1)
    out_e[list(ENV_SUM_COLUMNS)] = packs["sum"][ns:]
    out_a[:, list(AGENT_MIN_COLUMNS)] = packs["min"].view(M, -1)
    out_a[:, list(AGENT_MAX_COLUMNS)] = packs["max"][:nx].view(M, -1)
    out_e[list(ENV_MAX_COLUMNS)] = packs["max"][nx:]
    idle = ~(out_a[:, K.EM_EPISODES] > 0)
    for f in AGENT_MIN_COLUMNS + AGENT_MAX_COLUMNS:         # a module that played on no rank: this rank's own words (k_em_final's zeros)
        out_a[idle, f] = agent[idle, f]
    return out_a, out_e


def check_nav_conservation(iteration, summary, strict=True, log=None):
    """train.py:1125-1164 `_check_nav_conservation`: a violated episode stops a strict run, wherever (and whenever inside the rollout) it ended."""
    v = summary.get("nav_conservation_violations", 0.0)
    if v <= 0:
        return
    msg = (f"NAV conservation was violated in {v:.0f} episode(s) during iteration {iteration} (largest |sum(NAV) - A * init_cash| = "
           f"{summary.get('nav_conservation_error', float('nan')):g}). The ledger has created or destroyed cash, so every reward computed from NAV after this point is "
           f"meaningless. The markets concerned carry CDA_FLAG_NAV_CONSERVATION (CDAVecEnv.flags()).")
    if not strict:
        if log is not None:
            log(msg + " Continuing: strict_nav_check is off.")
        return
    raise NavConservationError(msg)


def log_iteration(it, stats, em, module_names, history, log, strict=True, shape=None, allreduce=None):
    """The end of a fused loop's iteration, outside its timed region: em, collected inside it (CDAVecEnv.collect_episode_metrics; None: metrics off), is summarised into
    stats["episode_metrics"] (as shape(summary), if given), the iteration goes to `history` and the log, then NAV conservation is checked.  allreduce: a data-parallel run
    first merges the ranks' tables by the device's own rule (allreduce_tables: the additive columns summed, EM_NAV_MIN by MIN, the *_MAX columns by MAX), so every rank
    summarises, logs and checks the GLOBAL figures - and a violation on any shard raises on every rank in the same iteration.  A callable without an `op` keyword is
    refused (TypeError), never summed."""
    summ = None
    if em is not None:
        if allreduce is not None:
            em = allreduce_tables(em, allreduce)
        summ = summarise(*em, module_names=module_names)
        stats["episode_metrics"] = summ if shape is None else shape(summ)
    history.append(stats)
    log(json.dumps(stats))
    if summ is not None:
        check_nav_conservation(it, summ, strict=strict, log=log)
