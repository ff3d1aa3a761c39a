"""CPU: the scripted opponents' laws (include/cda_scripted_agents.h) against their numpy specification (gym_continuousdoubleauction_amd/scripted.py): the
specification on hand-written views, every branch named; cda_scripted_decide_host against it on random views that sit on every edge; the taker's draws; the
profile's bounds; views_from_report on hand-written books and on books the CPU oracle played.  No GPU."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from gym_continuousdoubleauction_amd import book as B
from gym_continuousdoubleauction_amd import scripted as S
from gym_continuousdoubleauction_amd.scripted import Profile

ERR_INVALID = -1
MAKER = Profile(law=S.LAW_MAKER, size_mean=0.25, size_sigma=0.125, max_position=10, skew_position=4, max_orders=2)
TAKER = Profile(law=S.LAW_TAKER, size_mean=-0.5, size_sigma=0.5, max_position=3, p_trade_q32=1 << 32)
IMB = Profile(law=S.LAW_IMBALANCE, size_mean=0.5, size_sigma=0.25, max_position=5, depth_levels=3, imb_num=3, imb_den=2)
PASS = Profile(law=S.LAW_PASS, size_mean=1.0, size_sigma=1.0)


def view(**kw):
    v = np.zeros((), S.VIEW_DTYPE)
    for k, x in kw.items():
        v[k] = x
    return v


def _taker_key(buy):
    """an agent index whose draw (seed 7, counter 2, market 11, draw 3) has bit 32 clear (a buy) / set (a sell)"""
    return next(a for a in range(64) if ((S.taker_draw(7, 2, 11, 3, a) >> 32) & 1 == 0) == buy)


BUY, SELL = _taker_key(True), _taker_key(False)
ORDER = (0.25, 0.125)
# name of the branch, profile, view, agent, the intended (category, size_mean, size_sigma, price, price_offset)
TABLE = [
    ("law_pass", PASS, view(net_position=3, best_bid=100, best_ask=105, tick=1), 0, (0, 0.0, 0.0, 0, 1)),
    ("taker_buy", TAKER, view(net_position=2), BUY, (1, -0.5, 0.5, 0, 1)),
    ("taker_buy_capped", TAKER, view(net_position=3), BUY, (0, 0.0, 0.0, 0, 1)),
    ("taker_sell", TAKER, view(net_position=-2), SELL, (5, -0.5, 0.5, 0, 1)),
    ("taker_sell_capped", TAKER, view(net_position=-3), SELL, (0, 0.0, 0.0, 0, 1)),
    ("taker_idle", dataclasses.replace(TAKER, p_trade_q32=0), view(), BUY, (0, 0.0, 0.0, 0, 1)),
    ("maker_stop_sell", MAKER, view(net_position=11, best_bid=100, best_ask=110, tick=1), 0, (5, *ORDER, 0, 1)),
    ("maker_stop_buy", MAKER, view(net_position=-11, best_bid=100, best_ask=110, tick=1), 0, (1, *ORDER, 0, 1)),
    # at the cap itself the maker still quotes (the stop is strictly beyond it), on the reducing side
    ("maker_skew_ask_limit_inside", MAKER, view(net_position=10, best_bid=100, best_ask=110, tick=1), 0, (6, *ORDER, 0, 2)),
    ("maker_skew_bid_limit_inside", MAKER, view(net_position=-5, best_bid=100, best_ask=110, tick=1), 0, (2, *ORDER, 0, 2)),
    # inside the skew band: (t_step + agent) even -> bid, odd -> ask
    ("maker_alt_bid_limit_inside", MAKER, view(net_position=4, t_step=6, best_bid=100, best_ask=110, tick=1), 2, (2, *ORDER, 0, 2)),
    ("maker_alt_ask_limit_inside", MAKER, view(net_position=-4, t_step=6, best_bid=100, best_ask=110, tick=1), 3, (6, *ORDER, 0, 2)),
    # a spread of exactly one tick, in the book's unit (tick 5: prices move in fives): join; two ticks: inside
    ("maker_alt_bid_limit_join", MAKER, view(t_step=0, best_bid=100, best_ask=105, tick=5), 0, (2, *ORDER, 0, 1)),
    ("maker_alt_bid_limit_inside", MAKER, view(t_step=0, best_bid=100, best_ask=110, tick=5), 0, (2, *ORDER, 0, 2)),
    ("maker_alt_bid_limit_inside", MAKER, view(t_step=0, best_bid=100, best_ask=102, tick=1), 0, (2, *ORDER, 0, 2)),
    # wide spread, the agent already at the side's best: join
    ("maker_alt_bid_limit_join", MAKER, view(t_step=0, best_bid=100, best_ask=110, tick=1, own_orders=(1, 0), own_best=(100, 0)), 0, (2, *ORDER, 0, 1)),
    ("maker_alt_ask_limit_join", MAKER, view(t_step=1, best_bid=100, best_ask=110, tick=1, own_orders=(0, 1), own_best=(0, 110)), 0, (6, *ORDER, 0, 1)),
    # ... not at best (its own order lies deeper): inside
    ("maker_alt_ask_limit_inside", MAKER, view(t_step=1, best_bid=100, best_ask=110, tick=1, own_orders=(0, 1), own_best=(0, 112)), 0, (6, *ORDER, 0, 2)),
    # max_orders resting on the side: modify (the reference moves the oldest order)
    ("maker_alt_bid_modify_inside", MAKER, view(t_step=0, best_bid=100, best_ask=110, tick=1, own_orders=(2, 0), own_best=(98, 0)), 0, (3, *ORDER, 0, 2)),
    ("maker_alt_ask_modify_join", MAKER, view(t_step=1, best_bid=100, best_ask=101, tick=1, own_orders=(0, 3), own_best=(0, 104)), 0, (7, *ORDER, 0, 1)),
    # an empty own side / an empty opposite side / an empty book: join level 0
    ("maker_alt_bid_limit_join", MAKER, view(t_step=0, best_bid=0, best_ask=110, tick=1), 0, (2, *ORDER, 0, 1)),
    ("maker_alt_bid_limit_join", MAKER, view(t_step=0, best_bid=100, best_ask=0, tick=1), 0, (2, *ORDER, 0, 1)),
    ("maker_alt_ask_limit_join", MAKER, view(t_step=1), 0, (6, *ORDER, 0, 1)),
    # imbalance 3 : 2 - strictly over the ratio trades, at it does not
    ("imb_buy", IMB, view(vol=(31, 20)), 0, (1, 0.5, 0.25, 0, 1)),
    ("imb_balanced", IMB, view(vol=(30, 20)), 0, (0, 0.0, 0.0, 0, 1)),
    ("imb_sell", IMB, view(vol=(20, 31)), 0, (5, 0.5, 0.25, 0, 1)),
    ("imb_balanced", IMB, view(vol=(20, 30)), 0, (0, 0.0, 0.0, 0, 1)),
    ("imb_buy_capped", IMB, view(vol=(31, 20), net_position=5), 0, (0, 0.0, 0.0, 0, 1)),
    ("imb_buy", IMB, view(vol=(31, 20), net_position=4), 0, (1, 0.5, 0.25, 0, 1)),
    ("imb_sell_capped", IMB, view(vol=(0, 1), net_position=-5), 0, (0, 0.0, 0.0, 0, 1)),
    ("imb_sell", IMB, view(vol=(0, 1), net_position=-4), 0, (5, 0.5, 0.25, 0, 1)),
    ("imb_balanced", IMB, view(vol=(0, 0)), 0, (0, 0.0, 0.0, 0, 1)),
]
ALL_BRANCHES = {"law_pass", "taker_buy", "taker_buy_capped", "taker_sell", "taker_sell_capped", "taker_idle", "maker_stop_sell", "maker_stop_buy",
                "imb_buy", "imb_buy_capped", "imb_sell", "imb_sell_capped", "imb_balanced"} | {
                    f"maker_{how}_{side}_{kind}_{where}" for how in ("alt", "skew") for side in ("bid", "ask") for kind in ("limit", "modify") for where in ("inside", "join")}


def decide_host(profiles, pix, views, seed, counter, market, draw, agent):
    """cda_scripted_decide_host on arrays; returns the five action arrays"""
    from gym_continuousdoubleauction_amd._lib import lib
    n = len(views)
    pa = S.profiles_array(profiles, validate=False)
    pix, market, draw, agent = (np.ascontiguousarray(np.broadcast_to(x, (n,)), dt) for x, dt in ((pix, np.int32), (market, np.uint64), (draw, np.uint32), (agent, np.uint32)))
    views = np.ascontiguousarray(views)
    cat, price, off = (np.full(n, -7, np.int32) for _ in range(3))
    mean, sigma = (np.full(n, -7, np.float32) for _ in range(2))
    rc = lib().cda_scripted_decide_host(pa.ctypes.data, len(pa), pix.ctypes.data, views.ctypes.data, n, seed, counter, market.ctypes.data, draw.ctypes.data,
                                        agent.ctypes.data, cat.ctypes.data, mean.ctypes.data, sigma.ctypes.data, price.ctypes.data, off.ctypes.data)
    return rc, (cat, mean, sigma, price, off)


def same_actions(got, want):
    return all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))


def test_the_specification_on_hand_written_views():
    seen = set()
    for name, prof, v, agent, want in TABLE:
        c, sm, ss, p, o, why = S.decide(prof, v, seed=7, counter=2, market=11, draw=3, agent=agent)
        assert why == name and (c, float(sm), float(ss), p, o) == tuple(want), (name, (c, sm, ss, p, o), want)
        seen.add(why)
    # every law's every rule is in the table, apart from the maker's (how, side, kind, where) products, of which each FACTOR is
    flat = {x for n in seen for x in n.split("_")}
    assert {"alt", "skew", "bid", "ask", "limit", "modify", "inside", "join", "stop"} <= flat
    assert {n for n in ALL_BRANCHES if not n.startswith("maker_alt") and not n.startswith("maker_skew")} <= seen
    # ... and the C function says the same on the very same table
    rc, got = decide_host([t[1] for t in TABLE], np.arange(len(TABLE)), np.array([t[2] for t in TABLE]), 7, 2, 11, 3, np.array([t[3] for t in TABLE]))
    assert rc == 0
    for k, (name, _p, _v, _a, want) in enumerate(TABLE):
        assert (int(got[0][k]), float(got[1][k]), float(got[2][k]), int(got[3][k]), int(got[4][k])) == tuple(want), name


def random_views(rng, n, profiles, pix):
    """views that sit on the laws' edges: positions at and one beyond each cap and the skew, spreads of exactly one and two ticks, empty sides, own best at /
    off the side's best, volumes at and next to the imbalance ratio"""
    v = np.zeros(n, S.VIEW_DTYPE)
    cap = np.array([p.max_position for p in profiles])[pix]
    skew = np.array([p.skew_position for p in profiles])[pix]
    num, den = (np.array([getattr(p, k) for p in profiles])[pix] for k in ("imb_num", "imb_den"))
    pick = rng.integers(0, 12, n)
    pos = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4, pick == 5, pick == 6, pick == 7, pick == 8],
                    [cap, cap + 1, -cap, -cap - 1, skew, skew + 1, -skew, -skew - 1, cap - 1], rng.integers(-40, 41, n))
    v["net_position"] = pos
    v["t_step"] = rng.integers(0, 300, n)
    tick = rng.choice([1, 5, 7], n)
    v["tick"] = tick
    bid = tick * rng.integers(1, 60, n)
    spread = tick * np.select([rng.integers(0, 3, n) == 0, rng.integers(0, 2, n) == 0], [1, 2], rng.integers(1, 9, n))
    ask = bid + spread
    empty = rng.integers(0, 8, n)
    bid = np.where((empty == 0) | (empty == 2), 0, bid)
    ask = np.where((empty == 1) | (empty == 2), 0, ask)
    v["best_bid"], v["best_ask"] = bid, ask
    for s, best, worse in ((0, bid, bid - tick), (1, ask, ask + tick)):
        cnt = rng.integers(0, 5, n)
        v["own_orders"][:, s] = cnt
        v["own_best"][:, s] = np.where(cnt == 0, 0, np.where(rng.integers(0, 2, n) == 0, best, worse))
    Bv = rng.integers(0, 2000, n)
    how = rng.integers(0, 6, n)
    Sv = np.select([how == 0, how == 1, how == 2], [Bv * den // num, Bv * den // num + 1, Bv * num // den], rng.integers(0, 2000, n))
    swap = rng.integers(0, 2, n) == 0
    v["vol"][:, 0], v["vol"][:, 1] = np.where(swap, Sv, Bv), np.where(swap, Bv, Sv)
    return v


LAW_PROFILES = {
    "pass": [PASS, Profile(law=S.LAW_PASS)],
    "taker": [dataclasses.replace(TAKER, p_trade_q32=p, max_position=c) for p in (0, 1, 1 << 31, (1 << 32) - 1, 1 << 32) for c in (0, 3)],
    "maker": [MAKER, dataclasses.replace(MAKER, max_position=0, skew_position=0, max_orders=1), dataclasses.replace(MAKER, max_position=7, skew_position=7, max_orders=4)],
    "imbalance": [IMB, dataclasses.replace(IMB, imb_num=1, imb_den=1, max_position=0), dataclasses.replace(IMB, imb_num=7, imb_den=3, max_position=30)],
}


@pytest.mark.parametrize("law", sorted(LAW_PROFILES))
def test_decide_host_equals_the_specification(law):
    n = 20000
    rng = np.random.default_rng(S.LAWS[law])
    profiles = LAW_PROFILES[law]
    pix = rng.integers(0, len(profiles), n)
    views = random_views(rng, n, profiles, pix)
    market, draw, agent = rng.integers(0, 1 << 40, n), rng.integers(0, 1 << 31, n), rng.integers(0, 16, n)
    seed, counter = 0xfedcba9876543210, 12345
    tally = {}
    want = S.actions_from_views(profiles, pix, views, seed, counter, market, draw, agent, branches=tally)
    rc, got = decide_host(profiles, pix, views, seed, counter, market, draw, agent)
    assert rc == 0 and same_actions(got, want), [np.flatnonzero(g != w)[:4] for g, w in zip(got, want)]
    fired = {k for k in tally if k in ALL_BRANCHES}
    assert fired == set(tally)                                           # no branch name outside the list
    need = {"pass": {"law_pass"}, "taker": {b for b in ALL_BRANCHES if b.startswith("taker")}, "imbalance": {b for b in ALL_BRANCHES if b.startswith("imb")},
            "maker": {b for b in ALL_BRANCHES if b.startswith("maker")}}[law]
    assert need <= fired, sorted(need - fired)                           # the random views reach every rule of the law


def test_taker_draws_are_not_the_random_modules():
    """equal (seed, market, step / draw, agent) and counter 0: the taker's draw differs from cda_random_action's w0 - whose Python restatement here is first pinned
    to the C function through the category it implies"""
    from gym_continuousdoubleauction_amd._lib import lib
    seed, base, step, n, a = 99, 1000, 17, 64, 16
    cat = np.zeros((n, a), np.int32); price = np.zeros((n, a), np.int32); off = np.zeros((n, a), np.int32)
    mean = np.zeros((n, a), np.float32); sigma = np.zeros((n, a), np.float32)
    assert lib().cda_random_actions_host(seed, base, step, n, a, cat.ctypes.data, mean.ctypes.data, sigma.ctypes.data, price.ctypes.data, off.ctypes.data) == 0
    M64 = (1 << 64) - 1
    for m in range(n):
        for j in range(a):
            w0 = S.mix((S.mix((seed + (base + m) * 0xd1342543de82ef95) & M64) + ((step << 32) | j)) & M64)
            assert ((w0 & 0xffffffff) * 9) >> 32 == cat[m, j] and ((w0 >> 32) * 10) >> 32 == price[m, j]
            w = S.taker_draw(seed, 0, base + m, step, j)
            assert w != w0 and (w & 0xffffffff) != (w0 & 0xffffffff)


def test_taker_trade_frequency():
    n, p = 100000, 1 << 30
    prof = dataclasses.replace(TAKER, p_trade_q32=p, max_position=1 << 20)
    rng = np.random.default_rng(5)
    views = np.zeros(n, S.VIEW_DTYPE)
    rc, got = decide_host([prof], 0, views, 31337, 3, rng.integers(0, 1 << 20, n), np.arange(n) % 4096, rng.integers(0, 16, n))
    assert rc == 0
    freq = float((got[0] != 0).mean())
    sd = (0.25 * 0.75 / n) ** 0.5
    assert abs(freq - 0.25) <= 4 * sd, (freq, sd)
    buys = float((got[0] == 1).sum()) / float((got[0] != 0).sum())
    assert abs(buys - 0.5) <= 4 * (0.25 / (got[0] != 0).sum()) ** 0.5, buys


BOUNDS = [  # field, values that are valid, values one step outside
    ("law", (1, 4), (0, 5)),
    ("size_mean", (-1.0, 1.0), (np.nextafter(np.float32(-1), np.float32(-2)), np.nextafter(np.float32(1), np.float32(2)), float("nan"))),
    ("size_sigma", (0.0, 1.0), (-np.nextafter(np.float32(0), np.float32(1)), np.nextafter(np.float32(1), np.float32(2)), float("nan"))),
    ("max_position", (4, 2 ** 31 - 1), (3, -1)),                        # (3: below the base profile's skew_position of 4)
    ("skew_position", (0, 10), (-1, 11)),
    ("max_orders", (1, 2 ** 31 - 1), (0,)),
    ("depth_levels", (1, 10), (0, 11)),
    ("imb_den", (1, 3), (0, 4)),
    ("imb_num", (2, 2 ** 31 - 1), (1,)),
    ("p_trade_q32", (0, 1 << 32), ((1 << 32) + 1,)),
]


def test_profile_validation():
    from gym_continuousdoubleauction_amd._lib import lib
    base = Profile(law=S.LAW_MAKER, size_mean=0.5, size_sigma=0.5, max_position=10, skew_position=4, max_orders=2, depth_levels=5, imb_num=3, imb_den=2, p_trade_q32=5)

    def c_valid(p):
        pa = S.profiles_array([p], validate=False)
        return lib().cda_scripted_profile_check_host(pa.ctypes.data, 1)

    assert base.problems() == [] and c_valid(base) == 0
    for field, good, bad in BOUNDS:
        for x in good:
            p = dataclasses.replace(base, **{field: x})
            assert p.problems() == [] and c_valid(p) == 0, (field, x)
        for x in bad:
            p = dataclasses.replace(base, **{field: x})
            assert p.problems() != [] and c_valid(p) == ERR_INVALID, (field, x)
            with pytest.raises(ValueError):
                S.profiles_array([p])
            # an invalid profile is refused by the host entry point, and nothing is written
            rc, got = decide_host([p], 0, np.zeros(3, S.VIEW_DTYPE), 0, 0, 0, 0, 0)
            assert rc == ERR_INVALID and (got[0] == -7).all()
    for name in S.NAMED:
        assert S.parse_profile(name).problems() == [] and S.parse_profile(name).law == S.LAWS[name]
    p = S.parse_profile("taker:p_trade_q32=1073741824,size_mean=0.5")
    assert p.p_trade_q32 == 1 << 30 and p.size_mean == 0.5 and p.law == S.LAW_TAKER
    for bad in ("momentum", "taker:p_trade_q32=4294967297", "maker:law=2", "maker:nosuch=1", "maker:max_orders"):
        with pytest.raises(ValueError):
            S.parse_profile(bad)
    assert C.sizeof(C.c_char * S.PROFILE_DTYPE.itemsize) == 64


def brute_views(books, num_agents, net_position, t_step, tick, depth):
    """the views straight from the order rows, with loops: an independent statement of views_from_report"""
    n = len(books)
    v = np.zeros((n, num_agents), S.VIEW_DTYPE)
    for i, pair in enumerate(books):
        for a in range(num_agents):
            v[i, a]["t_step"], v[i, a]["tick"], v[i, a]["net_position"] = t_step[i], tick[i], net_position[i][a]
            for s, rows in enumerate(pair):
                rows = B.as_orders(rows)
                prices = []
                for r in rows:
                    if not prices or prices[-1] != r[0]:
                        prices.append(int(r[0]))
                v[i, a]["best_bid" if s == 0 else "best_ask"] = prices[0] if prices else 0
                top = set(prices[:int(depth[i][a])])
                v[i, a]["vol"][s] = sum(int(r[1]) for r in rows if int(r[0]) in top)
                own = [r for r in rows if r[2] == a]
                v[i, a]["own_orders"][s] = len(own)
                v[i, a]["own_best"][s] = int(own[0][0]) if own else 0
    return v


def views_of_books(books, num_agents, net_position, t_step, tick, depth):
    rep = B.report_from_books(books, num_agents, max_levels=S.MAX_DEPTH)
    return S.views_from_report(rep["levels"], rep["agents"], net_position, t_step, tick, depth)


def test_views_from_report_on_hand_written_books():
    bids = [(100, 5, 0, 1, 1), (100, 2, 1, 2, 2), (99, 7, 0, 3, 3), (97, 1, 2, 4, 4)]
    asks = [(103, 4, 2, 5, 5), (104, 6, 2, 6, 6), (104, 1, 1, 7, 7)]
    books = [(np.array(bids, np.int32), np.array(asks, np.int32)), (np.zeros((0, 5), np.int32), np.array(asks[:1], np.int32))]
    pos = [[3, -3, 0], [1, 0, -1]]
    depth = [[1, 2, 10], [3, 1, 2]]
    v = views_of_books(books, 3, pos, [12, 0], [1, 5], depth)
    assert v.shape == (2, 3) and v["t_step"].tolist() == [[12] * 3, [0] * 3] and v["tick"].tolist() == [[1] * 3, [5] * 3] and v["net_position"].tolist() == pos
    assert v["best_bid"].tolist() == [[100] * 3, [0] * 3] and v["best_ask"].tolist() == [[103] * 3, [103] * 3]
    assert v["vol"][0].tolist() == [[7, 4], [14, 11], [15, 11]] and v["vol"][1].tolist() == [[0, 4]] * 3
    assert v["own_orders"][0].tolist() == [[2, 0], [1, 1], [1, 2]] and v["own_best"][0].tolist() == [[100, 0], [100, 104], [97, 103]]
    assert v["own_orders"][1].tolist() == [[0, 0], [0, 0], [0, 1]] and v["own_best"][1].tolist() == [[0, 0], [0, 0], [0, 103]]
    assert np.array_equal(v, brute_views(books, 3, pos, [12, 0], [1, 5], depth))
    with pytest.raises(ValueError):
        views_of_books(books, 3, pos, [12, 0], [1, 5], 11)


def test_views_from_report_on_oracle_books():
    import oracle_lib as O
    n, a = 12, 5
    ora = O.OracleEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 4096, "is_render": False}, n)
    ora.reset(seeds=np.arange(40, 40 + n, dtype=np.uint64))
    ora.run_random(0, 120, action_seed=9)
    books = [ora.get_book(i) for i in range(n)]
    assert sum(len(b) + len(s) for b, s in books) > 20 * n
    pos = [[int(ora.get_state(i).acc[j].net_position) for j in range(a)] for i in range(n)]
    t = [int(ora.get_state(i).t_step) for i in range(n)]
    depth = np.random.default_rng(1).integers(1, 11, (n, a))
    got = views_of_books(books, a, pos, t, [1] * n, depth)
    assert np.array_equal(got, brute_views(books, a, pos, t, [1] * n, depth))
    ora.close()


def test_the_script_kernel_exists_once_and_keeps_everything_in_registers():
    from test_kernel_resources import _kernels
    ks, bodies = _kernels()
    inst = {n: v for n, v in ks.items() if "k_script_actions" in n}
    assert len(inst) == 1, sorted(inst)
    (n, v), = inst.items()
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 128, (n, v)
    body = bodies[n]
    assert not any("global_atomic" in l or "flat_atomic" in l for l in body), n          # nothing depends on scheduling
    assert not any("scratch_" in l for l in body), n
    # the name carries none of the stems other tests count kernels by
    assert not any(stem in n for stem in ("k_stepILb", "k_tstepILb", "k_policy_step", "k_tape_"))
