"""Shared by the order-schedule tests (tests/test_hip_order_schedule.py): the hook replay, the market comparison, the message source and the plain statement of
what an attached schedule does - an oracle (or any env with the hooks' call shapes) driven window by window."""
import functools

import numpy as np

import oracle_lib as O
from gym_continuousdoubleauction_amd import _capi as K
from gym_continuousdoubleauction_amd import orders as OR

COUNTERS = ("num_trades_step", "num_passive_fills_step", "order_step_placed", "num_rejected_step")
INFO_KEYS = ("num_trades", "net_position", "num_trades_step", "num_passive_fills_step", "order_step_placed", "num_rejected_step", "lob_actions", "is_pass_action")
# the chunk of the message walk is 64 messages: none, one, one short of it, exactly it, one over, two chunks and a bit
EDGE_LENGTHS = (0, 1, 63, 64, 65, 130)


def cfg(cap, a=4, n_hist=4, **kw):
    return dict({"num_of_agents": a, "n_hist": n_hist, "init_cash": 20000, "max_step": 16, "is_render": False, "book_capacity": cap}, **kw)


def law(rng, n, a):
    """random actions with every order type well represented"""
    cat = rng.choice([1, 1, 2, 2, 2, 3, 3, 4, 5, 5, 6, 6, 6, 7, 7, 8, 0], (n, a)).astype(np.int32)
    price = rng.choice([0, 0, 0, 1, 2, 5, 9], (n, a)).astype(np.int32)
    off = rng.choice([2, 2, 1, 0], (n, a)).astype(np.int32)
    mean = rng.uniform(-0.3, 0.3, (n, a)).astype(np.float32)
    sigma = rng.uniform(0, 1, (n, a)).astype(np.float32)
    return cat, mean, sigma, price, off


def play_hooks(env, market, stream):
    """a list of messages through the one-order hooks (HipEnv and OracleEnv share the call shapes)"""
    for m in stream:
        if m == OR.MARK:
            env.mark_to_mkt(market)
        else:
            tr, typ, side, size, price = m[:5]
            env.place_order(market, tr, typ, side, size, price if typ != K.T_MARKET else 1)


def same_market(got, want, i, j=None, tag=""):
    j = i if j is None else j
    assert bytes(got.get_state(i)) == bytes(want.get_state(j)), (tag, i)
    for side in (0, 1):
        g, w = got.get_book(i, side), want.get_book(j, side)
        assert g.shape == w.shape and np.array_equal(g, w), (tag, i, side, g.shape, w.shape)


@functools.lru_cache(maxsize=None)
def source_messages(a=4, n_hist=4, want=900):
    """One long list of messages, cut from an oracle random-agent run's decoded orders in that run's execution order (three markets one after the other), a mark
    behind every 4 orders.  Computed once per (agents, history depth) on the CPU and shared; never modified."""
    n, steps = 3, 90
    src = O.OracleEnv(cfg(256, a, n_hist, max_step=256), n)
    src.reset(np.arange(700, 700 + n, dtype=np.uint64))
    rng = np.random.default_rng(17)
    la, ex = [], []
    for _ in range(steps):
        _, _, _, _, info = src.step(*law(rng, n, a))
        la.append(info["lob_actions"].copy())
        ex.append(np.array([[src.trace[i].exec_order[j] for j in range(a)] for i in range(n)]))
    src.close()
    la, ex = np.stack(la), np.stack(ex)
    out = []
    for i in range(n):
        out += OR.from_lob_actions(la[:, i], ex[:, i], mark_every=4)
    assert len(out) >= want, len(out)
    return tuple(out)


def rows_from_lengths(msgs, lengths):
    """lengths[r][t] messages for window t of row r, cut from `msgs` one after the other"""
    pos, rows = 0, []
    for row in lengths:
        r = []
        for n in row:
            assert pos + n <= len(msgs), (pos, n, len(msgs))
            r.append(list(msgs[pos:pos + n]))
            pos += n
        rows.append(r)
    return rows


def episode_over(state, num_agents, max_step):
    return bin(state.done_mask).count("1") == num_agents or state.t_step >= max_step


class Scheduled:
    """The specification of an attached order schedule, on an env with the hooks' call shapes: play(i) runs market i's window of its current t_step through
    place_order / mark_to_mkt; step() plays every market, steps, and - auto_reset - resets the markets whose episode ended.  counts: [N, 4] = done, rejected,
    invalid, fills, as the device's table.  max_step: the config's horizon, or one per market (per-market parameter rows: the market's own row's)."""

    def __init__(self, env, rows, sched_of, num_agents, max_step, loop=False, clear_step_counters=False, auto_reset=True):
        self.env, self.rows, self.sched_of, self.A, self.max_step = env, rows, list(sched_of), num_agents, max_step
        self.loop, self.clear, self.auto_reset = loop, clear_step_counters, auto_reset
        self.counts = np.zeros((len(self.sched_of), 4), np.int64)
        self.played = []                                   # (market, row, window, messages) of every non-empty play

    def horizon(self, i):
        return int(self.max_step[i]) if np.ndim(self.max_step) else self.max_step

    def window(self, i):
        r = self.sched_of[i]
        if r < 0:
            return None
        s = self.env.get_state(i)
        if episode_over(s, self.A, self.horizon(i)):
            return None
        t, S = s.t_step, len(self.rows[r])
        if self.loop:
            t %= S
        elif t >= S:
            return None
        return r, t

    def play(self, i):
        rt = self.window(i)
        if rt is None or not self.rows[rt[0]][rt[1]]:
            return
        msgs = self.rows[rt[0]][rt[1]]
        ok = OR.valid(OR.pack([msgs])[1], self.A)
        good = [m for m, k in zip(msgs, ok) if k]
        self.counts[i, 2] += len(msgs) - len(good)
        self.played.append((i, rt[0], rt[1], len(msgs)))
        if not good:
            return
        before = self.env.get_state(i)
        for m in good:
            play_hooks(self.env, i, [m])
            after = self.env.get_state(i)
            rej = m != OR.MARK and after.acc[m[0]].num_rejected_step != before.acc[m[0]].num_rejected_step
            self.counts[i, 1 if rej else 0] += 1
            before = after                                 # (one dump per message: the state behind a message is the state ahead of the next)
        if self.clear:
            s = self.env.get_state(i)
            for a in range(self.A):
                for k in COUNTERS:
                    setattr(s.acc[a], k, 0)
            self.env.set_state(i, s)

    def play_all(self):
        for i in range(len(self.sched_of)):
            self.play(i)

    def step(self, *acts):
        self.play_all()
        obs, rew, term, trunc, info = self.env.step(*acts)
        obs, rew, term, trunc = obs.copy(), rew.copy(), term.copy(), trunc.copy()
        info = {k: v.copy() for k, v in info.items()}
        done = ((term != 0) | (trunc != 0)).astype(np.uint8)
        if self.auto_reset and done.any():
            obs[done == 1] = self.env.reset(None, done)[done == 1]
        return obs, rew, term, trunc, info, done
