"""Test helpers for the stateful opponents (tests/test_stateful_host.py, tests/test_hip_stateful.py): the host entry point on arrays, the shared closed-loop case
(profiles, slot table, seeds, shapes - played on the CPU oracle with the specification choosing the actions, and on the device by the GPU tests), and views read
from an env's own reports."""
import dataclasses
import functools

import numpy as np

from gym_continuousdoubleauction_amd import scripted as S
from gym_continuousdoubleauction_amd import stateful as F
from gym_continuousdoubleauction_amd.stateful import Profile

KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset")
TRADING = {"trend_buy", "trend_sell", "value_buy", "value_sell", "exec_passive_limit", "exec_passive_modify", "exec_market"}

# the closed-loop case: six profiles mixed across the slots of every market, episodes of MAX_STEP steps so that a market resets itself several times in STEPS steps
MAX_STEP, STEPS, SEED, BASE, RESET_SEED = 6, 24, 41, 500, 900
SHAPES = [(16, 4, 0), (8, 16, 0), (8, 16, 512)]
# Six steps leave little time for a mid to move, so the case is built around it: two patient parent orders quote both sides from step 1 (limit, then modify), an
# impatient large buyer sweeps the ask level from step 2, the seller's next limit order then rests one tick off the new last price - the mid has moved, and the
# fast trend follower buys while the contrarian sells; the value trader's V walks every step until the touch is cheap or dear against it.
_SZ = dict(size_mean=0.02, size_sigma=0.01)
CASE = [
    Profile(law=F.LAW_TREND, max_position=3, fast_shift=0, slow_shift=1, band_ticks=0, direction=1, warmup=0, **_SZ),
    Profile(law=F.LAW_EXECUTION, target=40, start_step=0, duration=2, patience=5, **_SZ),
    Profile(law=F.LAW_EXECUTION, target=-40, start_step=0, duration=2, patience=5, **_SZ),
    Profile(law=F.LAW_EXECUTION, size_mean=0.3, size_sigma=0.1, target=400, start_step=1, duration=2, patience=0),
    Profile(law=F.LAW_TREND, max_position=50, fast_shift=0, slow_shift=2, band_ticks=0, direction=-1, warmup=1, **_SZ),
    Profile(law=F.LAW_VALUE, max_position=3, band_ticks=0, p_move_q32=1 << 32, **_SZ),
]


def case_config(a, tile=0):
    return {"num_of_agents": a, "init_cash": 10 ** 9, "max_step": MAX_STEP, "is_render": False, "book_capacity": tile}


def case_ticks(n):
    return [1 if i % 2 == 0 else 5 for i in range(n)]


def mixed_slots(n, a, k=len(CASE)):
    m, j = np.meshgrid(np.arange(n), np.arange(a), indexing="ij")
    return (1 + (m * 5 + j * 7 + m // 3) % k).astype(np.int32)


def advance_host(profiles, pix, views, states, seed, counter, market, draw, agent):
    """cda_stateful_advance_host on arrays; returns (rc, the five action arrays, the new states [n, 4])"""
    from gym_continuousdoubleauction_amd._lib import lib
    n = len(views)
    pa = F.profiles_array(profiles, validate=False)
    pix, market, draw, agent = (np.ascontiguousarray(np.broadcast_to(x, (n,)), dt) for x, dt in ((pix, np.int32), (market, np.uint64), (draw, np.uint32), (agent, np.uint32)))
    views = np.ascontiguousarray(views)
    st = np.ascontiguousarray(np.asarray(states, np.int64).reshape(n, F.STATE_WORDS)).copy()
    cat, price, off = (np.full(n, -7, np.int32) for _ in range(3))
    mean, sigma = (np.full(n, -7, np.float32) for _ in range(2))
    rc = lib().cda_stateful_advance_host(pa.ctypes.data, len(pa), pix.ctypes.data, views.ctypes.data, n, seed, counter, market.ctypes.data, draw.ctypes.data,
                                         agent.ctypes.data, st.ctypes.data, cat.ctypes.data, mean.ctypes.data, sigma.ctypes.data, price.ctypes.data, off.ctypes.data)
    return rc, (cat, mean, sigma, price, off), st


def same_actions(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32)) for g, w in zip(got, want))


def views_of_books(books, num_agents, net_position, t_step, tick):
    from gym_continuousdoubleauction_amd import book as B
    rep = B.report_from_books(books, num_agents, max_levels=1)
    return S.views_from_report(rep["levels"], rep["agents"], net_position, t_step, tick, 1)


def views_of_env(env, dumps=False):
    """the views [N, A] from independent readings of the device's state: book_levels / book_agents / get_state / market_config - or, dumps=True, host dumps of
    the books through book.py.  vol is zeroed: the stateful kernel sums none."""
    n, a = env.n_markets, env.num_agents
    states = [env.get_state(i) for i in range(n)]
    pos = [[int(s.acc[j].net_position) for j in range(a)] for s in states]
    t = [int(s.t_step) for s in states]
    tick = [int(env.market_config(i)["tick_size"]) for i in range(n)]
    if dumps:
        v = views_of_books([env.get_book(i) for i in range(n)], a, pos, t, tick)
    else:
        v = S.views_from_report(env.book_levels(1), env.book_agents(), pos, t, tick, 1)
    v["vol"] = 0
    return v


class OracleByTick:
    """n markets on the CPU oracle, market i with tick case_ticks(n)[i]: one OracleEnv per tick size (an oracle env has one config), indexed as one batch"""

    def __init__(self, cfg, n, seeds):
        import oracle_lib as O
        self.n, self.a = n, cfg["num_of_agents"]
        self.ticks = case_ticks(n)
        self.groups = []
        for tick in sorted(set(self.ticks)):
            idx = np.array([i for i in range(n) if self.ticks[i] == tick])
            env = O.OracleEnv(dict({k: v for k, v in cfg.items() if k not in ("auto_reset", "book_capacity")}, tick_size=tick), n_markets=len(idx))
            env.reset(seeds=np.asarray(seeds, np.uint64)[idx])
            self.groups.append((idx, env))

    def states_and_books(self):
        st, bk = [None] * self.n, [None] * self.n
        for idx, env in self.groups:
            for k, i in enumerate(idx):
                st[i], bk[i] = env.get_state(k), env.get_book(k)
        return st, bk

    def views(self):
        st, bk = self.states_and_books()
        v = views_of_books(bk, self.a, [[int(s.acc[j].net_position) for j in range(self.a)] for s in st], [int(s.t_step) for s in st], self.ticks)
        v["vol"] = 0
        return v

    def step(self, acts):
        """step every market, reset the ones whose episode ended (what the device's auto_reset does inside the step kernel); returns the done mask [n]"""
        done = np.zeros(self.n, bool)
        for idx, env in self.groups:
            _o, _r, term, trunc, _ = env.step(*(np.ascontiguousarray(x[idx]) for x in acts))
            d = (term | trunc).astype(bool)
            if d.any():
                env.reset(mask=d.astype(np.uint8))
            done[idx] = d
        return done

    def close(self):
        for _idx, env in self.groups:
            env.close()


@functools.lru_cache(maxsize=None)
def oracle_episode(n, a):
    """The closed-loop case on the oracle alone: every slot plays CASE[mixed_slots - 1], the specification (stateful.play) choosing the actions from the oracle's
    books and accounts and keeping the state.  Returns a dict: `tally` (branch -> count over STEPS steps), `resets` [n], `unquoted` (slot-steps seen with a side
    empty), `actions` (the five arrays [STEPS, n, a]) and `states` [STEPS, n, a, 4] after every step's advance."""
    slots = mixed_slots(n, a)
    pix = slots - 1
    m, j = np.meshgrid(np.arange(n), np.arange(a), indexing="ij")
    ora = OracleByTick(case_config(a), n, RESET_SEED + np.arange(n))
    state = np.zeros((n, a, F.STATE_WORDS), np.int64)
    tally, resets, unquoted = {}, np.zeros(n, np.int64), 0
    acts_all, states_all = [], []
    for t in range(STEPS):
        views = ora.views()
        unquoted += int(((views["best_bid"] == 0) | (views["best_ask"] == 0)).sum())
        acts, state = F.play(CASE, pix, views, state, SEED, 0, BASE + m, t, j, branches=tally)
        acts_all.append(acts)
        states_all.append(state.copy())
        resets += ora.step(acts)
    ora.close()
    return {"tally": tally, "resets": resets, "unquoted": unquoted, "actions": tuple(np.stack([x[k] for x in acts_all]) for k in range(5)), "states": np.stack(states_all)}


def replace(p, **kw):
    return dataclasses.replace(p, **kw)
