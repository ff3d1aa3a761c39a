"""Per-market environment parameters: many configurations in one batch (include/cda.h cda_market_params).

Every market of a CDAVecEnv reads the PER_MARKET_KEYS from a row of its own; the SHAPE_KEYS set shapes, memory or kernel choice and hold for the
whole env.  A market's config is an override dict in the reference's key spelling: missing keys come from the env's config.  Everything here is host
code and runs without a GPU: a row is validated (the config with the row merged in passes the env's own checks, and its max_step is within the env's)
before anything reaches the device."""
import ctypes as C
import json

import numpy as np

from . import _capi as K

# reference key -> cda_market_params field
PER_MARKET_KEYS = {
    "max_step": "max_step", "tick_size": "tick_size", "init_cash": "init_cash",
    "initial_price_min": "initial_price_min", "initial_price_max": "initial_price_max",
    "min_size": "min_size", "mkt_max_size": "mkt_max_size", "limit_size_multiple": "limit_size_multiple",
    "order_penalty": "order_penalty", "trade_penalty": "trade_penalty", "drawdown_penalty": "drawdown_penalty",
    "passive_bonus": "passive_bonus", "loss_multiplier": "loss_multiplier",
}
SHAPE_KEYS = ("num_of_agents", "n_hist", "book_capacity", "book_spill", "auto_reset")

ROW_DTYPE = np.dtype(K.MarketParams)          # a row as numpy sees it (snapshots keep the rows of their markets in this form)


def market_config(base, override):
    """The effective config dict of a market: `base` (an env config dict) with `override` merged in.  ValueError when the override changes a shape
    key, KeyError for a key the env does not know; the values themselves are checked by validate_rows."""
    override = dict(override or {})
    for k, v in override.items():
        if k in SHAPE_KEYS:
            if v != base.get(k):
                raise ValueError(f"market config key {k!r} = {v!r} differs from the env's {base.get(k)!r}: it sets shapes, memory or kernel choice "
                                 f"and holds for the whole env (per-market keys: {sorted(PER_MARKET_KEYS)})")
        elif k not in PER_MARKET_KEYS and k not in base:
            raise KeyError(f"unknown env config key {k!r}; per-market keys: {sorted(PER_MARKET_KEYS)}")
    out = dict(base)
    out.update(override)
    return out


def row_of(cfg):
    """an effective config dict -> MarketParams (make_config's conversions: integer ticks, integer init_cash)"""
    c, _ = K.make_config(cfg)
    r = K.MarketParams()
    for key, field in PER_MARKET_KEYS.items():
        setattr(r, field, getattr(c, key))
    return r


def rows_of(base, overrides):
    """base config dict + a list of override dicts -> ctypes array of rows, validated (ValueError before any device is touched)"""
    rows = (K.MarketParams * len(overrides))()
    for i, o in enumerate(overrides):
        try:
            rows[i] = row_of(market_config(base, o))
        except (ValueError, KeyError) as e:
            raise type(e)(f"market config {i}: {e.args[0] if e.args else e}") from None
    validate_rows(base, rows)
    return rows


def validate_rows(base, rows):
    """the library's check (cda_check_market_params: the env's cfg_ok on the config with each row merged in, max_step within the env's)"""
    from ._lib import lib
    cfg, _ = K.make_config(base)
    n = len(rows)
    for i in range(n):
        rc = lib().cda_check_market_params(C.byref(cfg), 1, C.byref(rows[i]))
        if rc != 0:
            why = "tick_size outside 1 .. 65536" if rc == K.ERR_UNSUPPORTED else "outside the supported domain, or max_step above the env's"
            raise ValueError(f"market row {i} refused ({why}): {row_dict(rows[i])}")


def row_dict(r):
    """a row -> {reference key: value}"""
    return {key: getattr(r, field) for key, field in PER_MARKET_KEYS.items()}


def rows_to_numpy(rows):
    return np.frombuffer(bytes(memoryview(rows)), dtype=ROW_DTYPE).copy() if len(rows) else np.zeros(0, dtype=ROW_DTYPE)


def rows_from_numpy(arr):
    arr = np.ascontiguousarray(arr, dtype=ROW_DTYPE)
    rows = (K.MarketParams * len(arr))()
    C.memmove(rows, arr.ctypes.data, arr.nbytes)
    return rows


def load_market_configs(path):
    """a --market-configs file: a JSON list of override dicts"""
    with open(path) as fh:
        configs = json.load(fh)
    if not isinstance(configs, list) or not configs or not all(isinstance(c, dict) for c in configs):
        raise ValueError(f"{path}: a market-configs file holds a non-empty JSON list of override dicts")
    return configs


def round_robin(configs, n_markets):
    """market m gets configs[m % len(configs)]"""
    return [configs[m % len(configs)] for m in range(int(n_markets))]
