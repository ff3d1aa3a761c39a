"""Scripted opponents WITH MEMORY: the profiles, and the SPECIFICATION of the stateful laws in Python integers (include/cda_stateful_agents.h states them in C;
the device kernel k_stateful_actions and cda_stateful_advance_host equal this word for word).  No device code here: importable without a GPU.

The sibling family of scripted.py.  A law reads the same VIEW (scripted.VIEW_DTYPE; vol is not read) and STATE_WORDS int64 words of state per (market, slot):
word 0 the header (low 32 bits last_t, high 32 bits the tag 1 + profile index, 0 = never written), words 1 .. 3 the law's own.  One update rule serves every law
(advance below): fresh (t_step == 0, tag 0, or another profile's tag) -> zero the words and take the law's step; the same t_step again -> nothing; else the
law's step once.  x = best_bid + best_ask (twice the mid) exists on a quoted step (both sides non-empty).
    trend       words: fast EMA, slow EMA of x << 16, count of quoted steps - trades the sign of direction * (fast - slow) beyond a band, after a warm-up
    value       words: the private value V (units of x), initialised flag - V starts at x, random-walks by 2 * tick, trades a touch that is cheap / dear against V
    execution   words: consecutive steps behind schedule - works target over duration steps from start_step: a resting order at the touch while it has been behind
                for at most `patience` steps, a market order beyond; max_position does not bind it
It answers the env's Dict action: (category, size_mean, size_sigma, price, price_offset); a pass is (0, 0.0, 0.0, 0, 1)."""
import contextlib
import dataclasses

import numpy as np

from .scripted import VIEW_DTYPE, mix, views_from_report  # noqa: F401  (the view is the stateless family's, as it is)

LAW_TREND, LAW_VALUE, LAW_EXECUTION = 1, 2, 3
LAWS = {"trend": LAW_TREND, "value": LAW_VALUE, "execution": LAW_EXECUTION}
LAW_NAMES = {v: k for k, v in LAWS.items()}
MAX_PROFILES = 16
STATE_WORDS = 4
MAX_SHIFT = 12
MAX_BAND = 4096
DOMAIN = 0x082efa98ec4e6c89                  # include/cda_stateful_agents.h CDA_STATEFUL_DOMAIN
_M64 = (1 << 64) - 1

PROFILE_DTYPE = np.dtype([("law", "<i4"), ("size_mean", "<f4"), ("size_sigma", "<f4"), ("max_position", "<i4"), ("fast_shift", "<i4"), ("slow_shift", "<i4"),
                          ("band_ticks", "<i4"), ("direction", "<i4"), ("warmup", "<i4"), ("patience", "<i4"), ("p_move_q32", "<u8"), ("target", "<i4"),
                          ("start_step", "<i4"), ("duration", "<i4"), ("pad0", "<i4")])
STATE_DTYPE = np.dtype("<i8")
assert PROFILE_DTYPE.itemsize == 64

# every branch name advance() can answer
BRANCHES = ("trend_warmup", "trend_buy", "trend_buy_capped", "trend_sell", "trend_sell_capped", "trend_flat",
            "value_uninitialised", "value_buy", "value_buy_capped", "value_sell", "value_sell_capped", "value_hold",
            "exec_waiting", "exec_done", "exec_ahead", "exec_passive_limit", "exec_passive_modify", "exec_market")


@dataclasses.dataclass(frozen=True)
class Profile:
    """One stateful module (cda_stateful_profile).  Every bound of every law holds for every profile, whatever its own law (the defaults satisfy them).
    trend: EMAs of the mid with weights 2^-fast_shift and 2^-slow_shift, direction +1 follows / -1 fades, trades once it has seen more than `warmup` quoted steps and
    the EMAs differ by more than band_ticks ticks of the mid.  value: V moves by one tick of the mid with probability p_move_q32 / 2^32 per step, trades when the
    touch lies more than band_ticks ticks beyond it.  execution: target units of position (> 0 buys) over `duration` steps from start_step, passive for `patience`
    steps behind schedule."""
    law: int = LAW_TREND
    size_mean: float = 0.0
    size_sigma: float = 0.0
    max_position: int = 0
    fast_shift: int = 2
    slow_shift: int = 5
    band_ticks: int = 0
    direction: int = 1
    warmup: int = 0
    patience: int = 0
    p_move_q32: int = 0
    target: int = 1
    start_step: int = 0
    duration: int = 1

    def problems(self):
        """why the profile is invalid, as a list of strings (empty: valid) - the checks of cda_stateful_profile_valid"""
        out = []
        if self.law not in (1, 2, 3):
            out.append(f"law {self.law} is none of 1 .. 3")
        sm, ss = np.float32(self.size_mean), np.float32(self.size_sigma)
        if not (sm >= -1 and sm <= 1):
            out.append(f"size_mean {self.size_mean} outside [-1, 1]")
        if not (ss >= 0 and ss <= 1):
            out.append(f"size_sigma {self.size_sigma} outside [0, 1]")
        if self.max_position < 0:
            out.append("max_position < 0")
        if not 0 <= self.fast_shift < self.slow_shift <= MAX_SHIFT:
            out.append(f"need 0 <= fast_shift < slow_shift <= {MAX_SHIFT}")
        if not 0 <= self.band_ticks <= MAX_BAND:
            out.append(f"band_ticks outside 0 .. {MAX_BAND}")
        if self.direction not in (-1, 1):
            out.append("direction is neither -1 nor +1")
        if self.warmup < 0:
            out.append("warmup < 0")
        if not 0 <= self.p_move_q32 <= 1 << 32:
            out.append("p_move_q32 outside 0 .. 2^32")
        if self.target == 0:
            out.append("target == 0")
        if self.start_step < 0:
            out.append("start_step < 0")
        if self.duration < 1:
            out.append("duration < 1")
        if self.patience < 0:
            out.append("patience < 0")
        return out


NAMED = {
    "trend": Profile(law=LAW_TREND, size_mean=0.05, size_sigma=0.02, max_position=200, fast_shift=2, slow_shift=5, band_ticks=1, direction=1, warmup=8),
    "value": Profile(law=LAW_VALUE, size_mean=0.05, size_sigma=0.02, max_position=200, band_ticks=2, p_move_q32=1 << 29),
    "execution": Profile(law=LAW_EXECUTION, size_mean=0.02, size_sigma=0.0, target=100, start_step=0, duration=64, patience=3),
}
_FLOAT_FIELDS = ("size_mean", "size_sigma")


def parse_profile(spec):
    """A Profile from a Profile, a name ('trend', 'value', 'execution') or 'NAME:key=value,...' (the named defaults with fields replaced)."""
    if isinstance(spec, Profile):
        p = spec
    else:
        name, _, rest = str(spec).partition(":")
        if name not in NAMED:
            raise ValueError(f"unknown stateful opponent {name!r}: one of {sorted(NAMED)}")
        kw = {}
        for item in filter(None, (x.strip() for x in rest.split(","))):
            k, eq, val = item.partition("=")
            k = k.strip()
            if not eq or k not in {f.name for f in dataclasses.fields(Profile)} or k == "law":
                raise ValueError(f"bad field {item!r} in stateful opponent {spec!r}")
            kw[k] = float(val) if k in _FLOAT_FIELDS else int(val, 0)
        p = dataclasses.replace(NAMED[name], **kw)
    bad = p.problems()
    if bad:
        raise ValueError(f"invalid stateful profile {p}: " + "; ".join(bad))
    return p


def is_stateful_spec(spec):
    return isinstance(spec, Profile) or (isinstance(spec, str) and spec.partition(":")[0] in NAMED)


def module_id(index, profile):
    """the module id of stateful opponent `index`: stateful_<index>_<law>"""
    return f"stateful_{int(index)}_{LAW_NAMES[int(profile.law)]}"


def profiles_array(profiles, validate=True):
    """numpy PROFILE_DTYPE [n] (the 64-byte device layout) of a list of Profiles"""
    out = np.zeros(len(profiles), PROFILE_DTYPE)
    for k, p in enumerate(profiles):
        if validate and p.problems():
            raise ValueError(f"invalid stateful profile {p}: " + "; ".join(p.problems()))
        for f in dataclasses.fields(Profile):
            out[f.name][k] = getattr(p, f.name)
    return out


@contextlib.contextmanager
def attached(env, slot_table, profiles, seed=0, market_index_base=0):
    """stateful opponents attached to `env` (CDAVecEnv.set_stateful's arguments) for a `with` block; detached on any exit, if still attached then"""
    env.set_stateful(slot_table, profiles, seed=seed, market_index_base=market_index_base)
    try:
        yield
    finally:
        if env.stateful:
            env.clear_stateful()


def value_draw(seed, counter, market, draw, agent):
    """the value law's draw (cda_stateful_draw): scripted.taker_draw's construction under DOMAIN"""
    h0 = mix(((int(seed) ^ DOMAIN) + int(counter) * 0x9e3779b97f4a7c15 + int(market) * 0xd1342543de82ef95) & _M64)
    return mix((h0 + (((int(draw) & 0xffffffff) << 32) | (int(agent) & 0xffffffff))) & _M64)


def _behind(p, t, pos):
    el = min(max(t - int(p.start_step), 0), int(p.duration))
    n = int(p.target) * el
    due = abs(n) // int(p.duration) * (1 if n >= 0 else -1)          # truncated toward zero, as C's /
    gap = due - pos
    return gap > 0 if p.target > 0 else gap < 0


def advance(p, view, state, keys=(0, 0, 0, 0, 0), profile_index=0):
    """One slot, one call: ((category, size_mean f32, size_sigma f32, price, price_offset), new_state, branch).  `view`: a mapping / VIEW_DTYPE record; `state`:
    STATE_WORDS integers (not modified); keys = (seed, counter, market, draw, agent) of the value law's draw; profile_index: the slot's index in the attached
    profile list (its tag is 1 + that); `branch` names the decision path (the tests' tally).  cda_stateful_advance, then cda_stateful_decide."""
    t, pos, tick = int(view["t_step"]), int(view["net_position"]), int(view["tick"])
    bb, ba = int(view["best_bid"]), int(view["best_ask"])
    hdr = int(state[0]) & _M64
    tag, last_t, want = hdr >> 32, hdr & 0xffffffff, int(profile_index) + 1
    fresh = t == 0 or tag == 0 or tag != want
    w = [int(state[0]), int(state[1]), int(state[2]), int(state[3])]
    if fresh or last_t != (t & 0xffffffff):
        if fresh:
            w[1] = w[2] = w[3] = 0
        quoted = bb != 0 and ba != 0
        x = bb + ba
        if p.law == LAW_TREND:
            if quoted:
                y = x << 16
                if w[3] == 0:
                    w[1] = w[2] = y
                else:
                    w[1] += (y - w[1]) >> int(p.fast_shift)         # (Python's >> floors, as cda_stateful_floor_shift does)
                    w[2] += (y - w[2]) >> int(p.slow_shift)
                w[3] += 1
        elif p.law == LAW_VALUE:
            if w[2] == 0:
                if quoted:
                    w[1], w[2] = x, 1
            else:
                d = value_draw(*keys)
                if (d & 0xffffffff) < int(p.p_move_q32):
                    if (d >> 32) & 1 == 0:
                        w[1] += 2 * tick
                    else:
                        w[1] = max(w[1] - 2 * tick, 2 * tick)
        elif p.law == LAW_EXECUTION:
            w[1] = w[1] + 1 if _behind(p, t, pos) else 0
        hdr = (want << 32) | (t & 0xffffffff)
        w[0] = hdr - (1 << 64) if hdr >= 1 << 63 else hdr
    cap = int(p.max_position)
    cat, why = 0, "pass"
    if p.law == LAW_TREND:
        d, thr = int(p.direction) * (w[1] - w[2]), (2 * int(p.band_ticks) * tick) << 16
        if w[3] <= int(p.warmup):
            why = "trend_warmup"
        elif d > thr:
            cat, why = (1, "trend_buy") if pos < cap else (0, "trend_buy_capped")
        elif d < -thr:
            cat, why = (5, "trend_sell") if pos > -cap else (0, "trend_sell_capped")
        else:
            why = "trend_flat"
    elif p.law == LAW_VALUE:
        V, b = w[1], 2 * int(p.band_ticks) * tick
        if w[2] == 0:
            why = "value_uninitialised"
        elif ba != 0 and 2 * ba < V - b:
            cat, why = (1, "value_buy") if pos < cap else (0, "value_buy_capped")
        elif bb != 0 and 2 * bb > V + b:
            cat, why = (5, "value_sell") if pos > -cap else (0, "value_sell_capped")
        else:
            why = "value_hold"
    elif p.law == LAW_EXECUTION:
        buy = p.target > 0
        left = int(p.target) - pos
        if t < int(p.start_step):
            why = "exec_waiting"
        elif not (left > 0 if buy else left < 0):
            why = "exec_done"
        elif not _behind(p, t, pos):
            why = "exec_ahead"
        elif w[1] <= int(p.patience):
            resting = int(view["own_orders"][0 if buy else 1])
            cat, why = ((2, "exec_passive_limit") if resting == 0 else (3, "exec_passive_modify"))
            cat += 0 if buy else 4
        else:
            cat, why = (1 if buy else 5), "exec_market"
    sm = np.float32(p.size_mean) if cat else np.float32(0.0)
    ss = np.float32(p.size_sigma) if cat else np.float32(0.0)
    return (cat, sm, ss, 0, 1), w, why


def play(profiles, profile_index, views, states, seed=0, counter=0, market=0, draw=0, agent=0, branches=None):
    """The specification on arrays: item i plays profiles[profile_index[i]] on views[i] (VIEW_DTYPE) with states[i] (int64 [..., STATE_WORDS], not modified), keyed
    (seed, counter, market[i], draw[i], agent[i]); market / draw / agent broadcast.  Returns (the five action arrays (i32, f32, f32, i32, i32) shaped like `views`,
    the new states int64 shaped like `states`).  `branches`: a dict that, if given, counts the decision paths."""
    views = np.asarray(views)
    shape = views.shape
    flat = views.reshape(-1)
    n = len(flat)
    st = np.ascontiguousarray(np.asarray(states, np.int64)).reshape(n, STATE_WORDS)
    new = st.copy()
    pix = np.broadcast_to(np.asarray(profile_index), shape).reshape(-1)
    mk, dr, ag = (np.broadcast_to(np.asarray(x), shape).reshape(-1) for x in (market, draw, agent))
    cat, price, off = (np.zeros(n, np.int32) for _ in range(3))
    mean, sigma = (np.zeros(n, np.float32) for _ in range(2))
    for i in range(n):
        k = int(pix[i])
        (c, sm, ss, pr, o), w, why = advance(profiles[k], flat[i], st[i], (seed, counter, int(mk[i]), int(dr[i]), int(ag[i])), k)
        cat[i], mean[i], sigma[i], price[i], off[i] = c, sm, ss, pr, o
        new[i] = w
        if branches is not None:
            branches[why] = branches.get(why, 0) + 1
    return tuple(x.reshape(shape) for x in (cat, mean, sigma, price, off)), new.reshape(np.asarray(states).shape)
