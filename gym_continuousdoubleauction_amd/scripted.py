"""Scripted opponents: the profiles, and the SPECIFICATION of the laws in plain numpy / Python integers (include/cda_scripted_agents.h states them in C; the
device kernel k_script_actions and cda_scripted_decide_host equal this word for word).  No device code here: importable without a GPU.

A law reads a VIEW of one (market, agent) pair - integers only - and, for the taker, one counter-based 64-bit draw:
    t_step, net_position, tick, best_bid, best_ask (0 = that side is empty), own_orders[2] and own_best[2] (book_agents' `orders` and `best_price` columns),
    vol[2] (the volume of the first depth_levels levels of each side).
Prices are what the book stores: multiples of the market's tick_size, so a spread of "one tick" is best_ask - best_bid == tick.
It answers the env's Dict action: (category, size_mean, size_sigma, price, price_offset); a pass is (0, 0.0, 0.0, 0, 1)."""
import contextlib
import dataclasses

import numpy as np

LAW_PASS, LAW_TAKER, LAW_MAKER, LAW_IMBALANCE = 1, 2, 3, 4
LAWS = {"pass": LAW_PASS, "taker": LAW_TAKER, "maker": LAW_MAKER, "imbalance": LAW_IMBALANCE}
MAX_PROFILES = 16
MAX_DEPTH = 10
DOMAIN = 0x13198a2e03707344                  # include/cda_scripted_agents.h CDA_SCRIPT_DOMAIN
_M64 = (1 << 64) - 1

PROFILE_DTYPE = np.dtype([("law", "<i4"), ("size_mean", "<f4"), ("size_sigma", "<f4"), ("max_position", "<i4"), ("skew_position", "<i4"), ("max_orders", "<i4"),
                          ("depth_levels", "<i4"), ("imb_num", "<i4"), ("imb_den", "<i4"), ("pad0", "<i4"), ("p_trade_q32", "<u8"), ("pad1", "<i4", (4,))])
VIEW_DTYPE = np.dtype([("t_step", "<i4"), ("net_position", "<i4"), ("tick", "<i4"), ("best_bid", "<i4"), ("best_ask", "<i4"), ("own_orders", "<i4", (2,)),
                       ("own_best", "<i4", (2,)), ("pad", "<i4"), ("vol", "<i8", (2,))])
assert PROFILE_DTYPE.itemsize == 64 and VIEW_DTYPE.itemsize == 56


@dataclasses.dataclass(frozen=True)
class Profile:
    """One scripted module (cda_script_profile).  size_mean / size_sigma are the action's size components of every order the law sends; max_position caps the
    inventory; the maker quotes the reducing side only beyond skew_position and modifies its oldest order once it has max_orders resting on a side; the imbalance
    trader sums depth_levels levels per side and trades when one side's volume exceeds imb_num / imb_den times the other's; the taker trades with probability
    p_trade_q32 / 2^32 per step."""
    law: int = LAW_PASS
    size_mean: float = 0.0
    size_sigma: float = 0.0
    max_position: int = 0
    skew_position: int = 0
    max_orders: int = 1
    depth_levels: int = 1
    imb_num: int = 1
    imb_den: int = 1
    p_trade_q32: int = 0

    def problems(self):
        """why the profile is invalid, as a list of strings (empty: valid) - the checks of cda_script_profile_valid"""
        out = []
        if self.law not in (1, 2, 3, 4):
            out.append(f"law {self.law} is none of 1 .. 4")
        sm, ss = np.float32(self.size_mean), np.float32(self.size_sigma)
        if not (sm >= -1 and sm <= 1):
            out.append(f"size_mean {self.size_mean} outside [-1, 1]")
        if not (ss >= 0 and ss <= 1):
            out.append(f"size_sigma {self.size_sigma} outside [0, 1]")
        if self.max_position < 0:
            out.append("max_position < 0")
        if not 0 <= self.skew_position <= self.max_position:
            out.append("skew_position outside 0 .. max_position")
        if self.max_orders < 1:
            out.append("max_orders < 1")
        if not 1 <= self.depth_levels <= MAX_DEPTH:
            out.append(f"depth_levels outside 1 .. {MAX_DEPTH}")
        if self.imb_den < 1 or self.imb_num < self.imb_den:
            out.append("need imb_num >= imb_den >= 1")
        if not 0 <= self.p_trade_q32 <= 1 << 32:
            out.append("p_trade_q32 outside 0 .. 2^32")
        return out


NAMED = {
    "pass": Profile(law=LAW_PASS),
    "maker": Profile(law=LAW_MAKER, size_mean=0.05, size_sigma=0.02, max_position=200, skew_position=60, max_orders=3),
    "taker": Profile(law=LAW_TAKER, size_mean=0.1, size_sigma=0.05, max_position=500, p_trade_q32=1 << 30),
    "imbalance": Profile(law=LAW_IMBALANCE, size_mean=0.1, size_sigma=0.05, max_position=300, depth_levels=5, imb_num=2, imb_den=1),
}
_INT_FIELDS = ("law", "max_position", "skew_position", "max_orders", "depth_levels", "imb_num", "imb_den", "p_trade_q32")


def parse_profile(spec):
    """A Profile from a Profile, a name ('pass', 'maker', 'taker', 'imbalance') or 'NAME:key=value,...' (the named defaults with fields replaced)."""
    if isinstance(spec, Profile):
        p = spec
    else:
        name, _, rest = str(spec).partition(":")
        if name not in NAMED:
            raise ValueError(f"unknown scripted opponent {name!r}: one of {sorted(NAMED)}")
        kw = {}
        for item in filter(None, (x.strip() for x in rest.split(","))):
            k, eq, val = item.partition("=")
            k = k.strip()
            if not eq or k not in {f.name for f in dataclasses.fields(Profile)} or k == "law":
                raise ValueError(f"bad field {item!r} in scripted opponent {spec!r}")
            kw[k] = int(val, 0) if k in _INT_FIELDS else float(val)
        p = dataclasses.replace(NAMED[name], **kw)
    bad = p.problems()
    if bad:
        raise ValueError(f"invalid scripted profile {p}: " + "; ".join(bad))
    return p


def is_scripted_spec(spec):
    return isinstance(spec, Profile) or (isinstance(spec, str) and spec.partition(":")[0] in NAMED)


LAW_NAMES = {v: k for k, v in LAWS.items()}


def module_id(index, profile):
    """the module id of scripted opponent `index` of a training run: scripted_<index>_<law> (what episode metrics, module returns and league.json name it by)"""
    return f"scripted_{int(index)}_{LAW_NAMES[int(profile.law)]}"


def profile_record(profile):
    """the canonical fields of a profile as plain Python numbers (the floats as the float32 the device reads): what a checkpoint's `args` and league.json hold -
    two specs that parse to the same profile give the same record"""
    p = parse_profile(profile)
    return {f.name: (int(getattr(p, f.name)) if f.name in _INT_FIELDS else float(np.float32(getattr(p, f.name)))) for f in dataclasses.fields(Profile)}


def opponent_slots(n_markets, num_agents, trained_slots, n_opponents):
    """the placement ppo.train_fused(opponents=[...]) attaches: i32 [N, A], 0 in slots < trained_slots, slot trained_slots + j of market m plays
    opponents[(m + j) % P] (the value 1 + that index)"""
    N, A, k, P = int(n_markets), int(num_agents), int(trained_slots), int(n_opponents)
    if not 1 <= k <= A - 1:
        raise ValueError(f"trained_slots must lie in 1 .. num_agents - 1 = {A - 1}, got {k}")
    if not 1 <= P <= MAX_PROFILES:
        raise ValueError(f"between 1 and {MAX_PROFILES} scripted opponents, got {P}")
    out = np.zeros((N, A), np.int32)
    m, j = np.meshgrid(np.arange(N), np.arange(A - k), indexing="ij")
    out[:, k:] = 1 + (m + j) % P
    return out


@contextlib.contextmanager
def attached(env, slot_script, profiles, seed=0, market_index_base=0):
    """scripted opponents attached to `env` (CDAVecEnv.set_scripted's arguments) for a `with` block - a training run; detached on any exit, if still attached then"""
    env.set_scripted(slot_script, profiles, seed=seed, market_index_base=market_index_base)
    try:
        yield
    finally:
        if env.scripted:
            env.clear_scripted()


def profiles_array(profiles, validate=True):
    """numpy PROFILE_DTYPE [n] (the 64-byte device layout) of a list of Profiles"""
    out = np.zeros(len(profiles), PROFILE_DTYPE)
    for k, p in enumerate(profiles):
        if validate and p.problems():
            raise ValueError(f"invalid scripted profile {p}: " + "; ".join(p.problems()))
        for f in dataclasses.fields(Profile):
            out[f.name][k] = getattr(p, f.name)
    return out


def mix(z):
    """splitmix64's finaliser on Python integers (include/cda_random_agents.h cda_ra_mix), every step wrapped to 64 bits"""
    z = (z + 0x9e3779b97f4a7c15) & _M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & _M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & _M64
    return z ^ (z >> 31)


def taker_draw(seed, counter, market, draw, agent):
    h0 = mix(((int(seed) ^ DOMAIN) + int(counter) * 0x9e3779b97f4a7c15 + int(market) * 0xd1342543de82ef95) & _M64)
    return mix((h0 + (((int(draw) & 0xffffffff) << 32) | (int(agent) & 0xffffffff))) & _M64)


MIX_DOMAIN = 0xa4093822299f31d0              # include/cda_scripted_agents.h CDA_SCRIPT_MIX_DOMAIN


def mix_draw(seed, counter, market, draw, agent):
    """the label tap's mixing draw (cda_script_mix_draw): taker_draw's construction under MIX_DOMAIN"""
    h0 = mix(((int(seed) ^ MIX_DOMAIN) + int(counter) * 0x9e3779b97f4a7c15 + int(market) * 0xd1342543de82ef95) & _M64)
    return mix((h0 + (((int(draw) & 0xffffffff) << 32) | (int(agent) & 0xffffffff))) & _M64)


def mix_played(seed, counter, market, draw, agent, mix_q32):
    """the mix decision on arrays (cda_label_mix_host): i32, 1 where the low 32 bits of mix_draw lie below mix_q32 (0 .. 2^32); market / draw / agent broadcast"""
    if not 0 <= int(mix_q32) <= 1 << 32:
        raise ValueError("mix_q32 outside 0 .. 2^32")
    mk, dr, ag = np.broadcast_arrays(np.asarray(market), np.asarray(draw), np.asarray(agent))
    out = np.zeros(mk.shape, np.int32)
    of, mf, df, af = out.reshape(-1), mk.reshape(-1), dr.reshape(-1), ag.reshape(-1)
    for i in range(of.size):
        of[i] = (mix_draw(seed, counter, int(mf[i]), int(df[i]), int(af[i])) & 0xffffffff) < int(mix_q32)
    return out


def mix_q32_of(beta):
    """beta in [0, 1] as the device's mix word: round(beta * 2^32), 0 = never, 2^32 = always"""
    b = float(beta)
    if not 0.0 <= b <= 1.0:
        raise ValueError(f"the mixing probability must lie in [0, 1], got {beta}")
    return int(round(b * (1 << 32)))


def label_spec(profiles, slot_label, views, seed=0, counter=0, market=0, draw=0, agent=0, mix_q32=0, slot_script=None):
    """k_script_label's label side, stated over actions_from_views: slot_label (0 = not labelled, 1 + k = labelled by profiles[k]) and views (VIEW_DTYPE, each view's
    vol summed over ITS label profile's depth_levels) of one shape, keyed (seed, counter, market, draw, agent) - the LABEL table's keys.  Returns (the five label
    arrays, labelled bool, played i32): the labels are meaningful where `labelled`; played = mix_played(...) where the slot is labelled and not attached
    (slot_script, same shape, nonzero = an attached slot; None = none is), 0 elsewhere."""
    sl = np.asarray(slot_label)
    labelled = (sl >= 1) & (sl <= len(profiles))
    acts = actions_from_views(profiles, np.where(labelled, sl - 1, 0), views, seed, counter, market, draw, agent)
    mixable = labelled if slot_script is None else labelled & (np.asarray(slot_script) == 0)
    played = np.where(mixable, mix_played(seed, counter, np.broadcast_to(np.asarray(market), sl.shape), np.broadcast_to(np.asarray(draw), sl.shape),
                                          np.broadcast_to(np.asarray(agent), sl.shape), mix_q32), 0).astype(np.int32)
    return acts, labelled, played


def decide(p, view, seed=0, counter=0, market=0, draw=0, agent=0):
    """One action: (category, size_mean f32, size_sigma f32, price, price_offset, branch).  `view`: a mapping / VIEW_DTYPE record; `branch` names the rule that
    fired (the tests' tally)."""
    pos, cap = int(view["net_position"]), int(p.max_position)
    cat, off, why = 0, 1, "pass"
    if p.law == LAW_TAKER:
        w = taker_draw(seed, counter, market, draw, agent)
        if (w & 0xffffffff) < int(p.p_trade_q32):
            buy = (w >> 32) & 1 == 0
            if buy:
                cat, why = (1, "taker_buy") if pos < cap else (0, "taker_buy_capped")
            else:
                cat, why = (5, "taker_sell") if pos > -cap else (0, "taker_sell_capped")
        else:
            why = "taker_idle"
    elif p.law == LAW_MAKER:
        if pos > cap:
            cat, why = 5, "maker_stop_sell"
        elif pos < -cap:
            cat, why = 1, "maker_stop_buy"
        else:
            if pos > p.skew_position:
                side, why = 1, "maker_skew_ask"
            elif pos < -p.skew_position:
                side, why = 0, "maker_skew_bid"
            else:
                side = (int(view["t_step"]) + int(agent)) & 1
                why = "maker_alt_ask" if side else "maker_alt_bid"
            modify = int(view["own_orders"][side]) >= p.max_orders
            cat = (3 if modify else 2) + 4 * side
            bb, ba = int(view["best_bid"]), int(view["best_ask"])
            best = ba if side else bb
            if bb != 0 and ba != 0 and ba - bb > int(view["tick"]) and int(view["own_best"][side]) != best:
                off = 2
            why += ("_modify" if modify else "_limit") + ("_inside" if off == 2 else "_join")
    elif p.law == LAW_IMBALANCE:
        B, S = int(view["vol"][0]), int(view["vol"][1])
        if B * p.imb_den > S * p.imb_num and pos < cap:
            cat, why = 1, "imb_buy"
        elif S * p.imb_den > B * p.imb_num and pos > -cap:
            cat, why = 5, "imb_sell"
        elif B * p.imb_den > S * p.imb_num:
            why = "imb_buy_capped"
        elif S * p.imb_den > B * p.imb_num:
            why = "imb_sell_capped"
        else:
            why = "imb_balanced"
    else:
        why = "law_pass"
    sm = np.float32(p.size_mean) if cat else np.float32(0.0)
    ss = np.float32(p.size_sigma) if cat else np.float32(0.0)
    return cat, sm, ss, 0, off, why


def actions_from_views(profiles, profile_index, views, seed=0, counter=0, market=0, draw=0, agent=0, branches=None):
    """The specification on arrays: item i plays profiles[profile_index[i]] on views[i] (VIEW_DTYPE) keyed (seed, counter, market[i], draw[i], agent[i]);
    market / draw / agent broadcast.  Returns the five action arrays (i32, f32, f32, i32, i32), shaped like `views`.  `branches`: a dict that, if given,
    counts the rules that fired."""
    views = np.asarray(views)
    shape = views.shape
    flat = views.reshape(-1)
    n = len(flat)
    pix = np.broadcast_to(np.asarray(profile_index), shape).reshape(-1)
    mk, dr, ag = (np.broadcast_to(np.asarray(x), shape).reshape(-1) for x in (market, draw, agent))
    cat, price, off = (np.zeros(n, np.int32) for _ in range(3))
    mean, sigma = (np.zeros(n, np.float32) for _ in range(2))
    for i in range(n):
        c, sm, ss, pr, o, why = decide(profiles[int(pix[i])], flat[i], seed, counter, int(mk[i]), int(dr[i]), int(ag[i]))
        cat[i], mean[i], sigma[i], price[i], off[i] = c, sm, ss, pr, o
        if branches is not None:
            branches[why] = branches.get(why, 0) + 1
    return tuple(x.reshape(shape) for x in (cat, mean, sigma, price, off))


def views_from_report(levels, agents, net_position, t_step, tick, depth_levels):
    """The views of every (market, agent) pair from independent readings of the state: `levels` = book_levels(L >= max depth)'s i64 [n, 2, L, 3], `agents` =
    book_agents()'s i64 [n, 2, A, 6], net_position int [n, A], t_step int [n], tick int [n] (or a scalar), depth_levels int [n, A] (each slot's profile's; or a
    scalar).  Returns VIEW_DTYPE [n, A]."""
    lv, ag = (np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x).astype(np.int64) for x in (levels, agents))
    n, A = ag.shape[0], ag.shape[2]
    depth = np.broadcast_to(np.asarray(depth_levels, np.int64), (n, A))
    if depth.min() < 1 or depth.max() > lv.shape[2]:
        raise ValueError(f"depth_levels must lie in 1 .. {lv.shape[2]} (the ladder's rows)")
    v = np.zeros((n, A), VIEW_DTYPE)
    v["t_step"] = np.broadcast_to(np.asarray(t_step, np.int64), (n,))[:, None]
    v["tick"] = np.broadcast_to(np.asarray(tick, np.int64), (n,))[:, None]
    v["net_position"] = np.asarray(net_position, np.int64).reshape(n, A)
    v["best_bid"] = lv[:, 0, 0, 0][:, None]
    v["best_ask"] = lv[:, 1, 0, 0][:, None]
    cum = np.cumsum(lv[:, :, :, 1], axis=2)                          # [n, 2, L]: volume of the first k + 1 levels
    for s in (0, 1):
        v["own_orders"][:, :, s] = ag[:, s, :, 0]
        v["own_best"][:, :, s] = ag[:, s, :, 3]
        v["vol"][:, :, s] = np.take_along_axis(cum[:, s, :], depth - 1, axis=1)
    return v
