"""The oracle side of the services fuzz (tests/test_hip_services_fuzz.py), shared with its CPU dry run (tests/test_services_fuzz_host.py): one oracle per distinct
per-market row, the deep books, the order streams cut from the oracle copy's next steps, the schedule's rows cut from the same messages, what feeds the quote
replay, and dry_run() - a whole case on the oracles alone, drawing from the case's generator exactly what the GPU test draws, which shows on the CPU that the
drawn inputs meet the conditions the GPU comparison relies on.  No device code."""
import numpy as np

import fuzz_cases as F
import oracle_lib as O
import schedule_util as U
from gym_continuousdoubleauction_amd import orders as OR
from gym_continuousdoubleauction_amd import quotes as Q

COUNTERS = U.COUNTERS
# A fill consumes a resting order or ends its taker.  A prefilled order (512 a side at the most) never was a taker: one record at the most; every other order
# that ever entered the market two: 2 x 512 + 2 x (66 steps x 16 agents + 134 streamed messages + 17 scheduled windows x 130 messages) = 7824 < 8192 per market
TAPE_CAPACITY = 8192
SCHEDULE_PLAYS = F.SERVICE_STEPS_AFTER + 1           # windows a market plays at the most: one per step of the schedule leg, and the play past the row's horizon


def tape_bound(prefilled, agents, streamed, scheduled):
    """the most tape records one market can write in a case (see TAPE_CAPACITY): prefilled = the orders put into its book through the state dump, both sides"""
    return prefilled + 2 * ((F.SERVICE_STEPS + F.SERVICE_STEPS_AFTER + F.SERVICE_STEPS_TAIL) * agents + streamed + scheduled)


class Oracles:
    """one OracleEnv per distinct row (tests/test_hip_market_params.py's construction), market m read from oracle m % k; with the env's auto-reset rule in short-
    horizon cases: the step, then reset(mask = terminated | truncated) with the new episode's first observation in the row"""

    def __init__(self, case):
        rows = case["rows"]
        self.n, self.A, self.auto = case["n_markets"], case["cfg"]["num_of_agents"], case["short"]
        self.o = [O.OracleEnv(dict(case["oracle_cfg"], **r), self.n) for r in rows] if rows else [O.OracleEnv(case["oracle_cfg"], self.n)]
        self.k = len(self.o)

    def of(self, m):
        return self.o[m % self.k]

    def _mix(self, arrs):
        out = np.array(arrs[0], copy=True)
        for j in range(1, self.k):
            out[j::self.k] = arrs[j][j::self.k]
        return out

    def reset(self, seeds):
        return self._mix([o.reset(seeds) for o in self.o])

    def step(self, acts, present, feed=None):
        outs = [o.step(*acts, present) for o in self.o]
        obs, rew, term, trunc = (self._mix([x[i] for x in outs]) for i in range(4))
        info = {key: self._mix([x[4][key] for x in outs]) for key in outs[0][4]}
        if feed is not None:                                   # the host-side episode tallies see the step BEFORE the masked reset
            feed(info, rew, term, trunc)
        done = (term != 0) | (trunc != 0)
        if self.auto and done.any():
            fresh = self._mix([o.reset(None, done.astype(np.uint8)) for o in self.o])
            obs[done] = fresh[done]
        return obs, rew, term, trunc, info

    def exec_order(self):
        return np.array([[self.of(m).trace[m].exec_order[j] for j in range(self.A)] for m in range(self.n)])

    def get_state(self, m):
        return self.of(m).get_state(m)

    def set_state(self, m, s):
        self.of(m).set_state(m, s)

    def get_book(self, m, side=None):
        return self.of(m).get_book(m, side)

    def book_size(self, m):
        return self.of(m).book_size(m)

    def place_order(self, m, *a):
        self.of(m).place_order(m, *a)

    def mark_to_mkt(self, m):
        self.of(m).mark_to_mkt(m)

    def flags(self):
        return self._mix([o.flags() for o in self.o])

    def close(self):
        for o in self.o:
            o.close()


def prefill(case, envs, seed_shift=0):
    """every third market of every env gets the same deep book (fuzz_cases.prefill_book through the state dump)"""
    n, a = case["n_markets"], case["cfg"]["num_of_agents"]
    for m in range(0, n, 3):
        nb, na = F.service_prefill_sizes(case, m + seed_shift)
        for e in envs:
            F.prefill_book(e, m, np.random.default_rng(case["prefill_seed"] + 7 * seed_shift + m + 1), a, nb, na)


def horizons(case):
    """every market's own max_step: its row's, or the config's when the case has no rows"""
    rows, n = case["rows"], case["n_markets"]
    return [int(rows[m % len(rows)]["max_step"]) if rows else int(case["cfg"]["max_step"]) for m in range(n)]


def cut_streams(case, src, rng):
    """The order-stream leg's input: the oracle copy plays the law's next steps; every market's decoded orders in execution order, cut (repeated if need be) to the
    drawn length; in two markets one invalid message of each kind is spliced in.  -> (streams, pools): pools[m] = the uncut messages of market m, which the
    schedule's rows are cut from too."""
    n, a = case["n_markets"], case["cfg"]["num_of_agents"]
    la, ex = [], []
    for _ in range(F.STREAM_SOURCE_STEPS):
        acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
        *_, info = src.step(acts, present)
        la.append(info["lob_actions"].copy()); ex.append(src.exec_order())
    la, ex = np.stack(la), np.stack(ex)
    streams, pools = [], []
    for m in range(n):
        st, want = OR.from_lob_actions(la[:, m], ex[:, m], mark_every=case["mark_every"]), int(case["stream_lengths"][m])
        pools.append(list(st))
        streams.append((st * (want // len(st) + 1))[:want] if st and want else [])
    for m in case["invalid_markets"]:
        for pos, bad in sorted(zip(rng.integers(0, len(streams[m]) + 1, 5).tolist(), F.invalid_messages(a)), reverse=True):
            streams[m].insert(pos, bad)
    return streams, pools


def stream_into_oracle(ora, m, stream, a, clear):
    """one market's stream through the oracle's hooks: the valid messages in order, then - clear - the step counters of a market that saw one (a market without
    a valid message is not touched: csrc/cda_orders.inc).  -> the validity mask"""
    ok = OR.valid(OR.pack([stream])[1], a)
    U.play_hooks(ora, m, [st for st, good in zip(stream, ok) if good])
    if clear and ok.any():
        s = ora.get_state(m)
        for j in range(a):
            for key in COUNTERS:
                setattr(s.acc[j], key, 0)
        ora.set_state(m, s)
    return ok


def schedule_rows(case, extras, pools):
    """rows[r][t] = the messages of window t of schedule row r: extras["lengths"] messages each, cut one after the other (wrapping) from the stream leg's messages
    of the markets that play row r - the flow is priced where those books stand -, the five invalid messages spliced into their window"""
    a, ms, bad = case["cfg"]["num_of_agents"], extras["schedule"]["market_schedule"], extras["invalid"]
    rows = []
    for r, lens in enumerate(extras["lengths"]):
        pool = [msg for m in np.flatnonzero(ms == r) for msg in pools[m]] or [msg for p in pools for msg in p]
        pos, row = 0, []
        for t, want in enumerate(lens):
            spliced = (r, t) == (bad["row"], bad["window"])
            k = want - (F.INVALID_KINDS if spliced else 0)
            w = [pool[(pos + i) % len(pool)] for i in range(k)] if pool else []
            pos += k
            if spliced:
                for at, msg in sorted(zip(bad["positions"], F.invalid_messages(a)), reverse=True):
                    w.insert(at, msg)
            row.append(w)
        rows.append(row)
    return rows


def scheduled(case, extras, ora, rows):
    """schedule_util.Scheduled - the statement of an attached schedule - on the oracles: market m's window goes into the oracle that owns m, and "episode over"
    asks the market's own row's max_step"""
    sc = extras["schedule"]
    return U.Scheduled(ora, rows, sc["market_schedule"], case["cfg"]["num_of_agents"], horizons(case), loop=sc["loop"], clear_step_counters=sc["clear_step_counters"])


def clocks_past_the_row_horizon(case, extras):
    """{market: t_step} - where the schedule leg puts, for one play, the clocks of every second market that can tell its own row's horizon from the config's: the
    market plays a row, its row's max_step H lies below the config's, the schedule loops (without the loop flag a t_step of 256 or more lies beyond every schedule
    anyway), and t_step is the first of H, H + 1, ... whose window t_step % S holds messages.  Over by the market's row, live by the config: nothing may play."""
    sc, top = extras["schedule"], int(case["cfg"]["max_step"])
    if not (case["rows"] and sc["loop"]):
        return {}
    hz, S, out = horizons(case), sc["n_windows"], {}
    for m in range(case["n_markets"]):
        r = int(sc["market_schedule"][m])
        if r >= 0 and hz[m] < top:
            t = next((t for t in range(hz[m], min(hz[m] + S, top)) if extras["lengths"][r][t % S]), None)
            if t is not None:
                out[m] = t
    return dict(list(out.items())[::2])


def move_clocks(envs, clocks):
    """t_step of the markets in `clocks` set through the state dump on every env; -> the clocks they had (the first env's)"""
    had = {}
    for m, t in clocks.items():
        for e in envs:
            s = e.get_state(m)
            had.setdefault(m, int(s.t_step))
            s.t_step = int(t)
            e.set_state(m, s)
    return had


def live(state, a, max_step):
    """the recorder visits the market: its episode is not over"""
    return bin(state.done_mask).count("1") != a and state.t_step < max_step


def feed_quotes(replays, source, case, left=None):
    """Ahead of a step: every live market of `source` (host dumps: get_state, get_book) visits each of `replays` with the top of its book.  left: a dict that
    collects, per market, the t_steps at which the market was found with its episode over (the recorder passes it by)"""
    a, hz = case["cfg"]["num_of_agents"], horizons(case)
    for m in range(case["n_markets"]):
        s = source.get_state(m)
        if live(s, a, hz[m]):
            row = Q.quote_from_orders(s.t_step, *source.get_book(m))
            for rp in replays:
                rp.visit(m, s.t_step, row)
        elif left is not None:
            left.setdefault(m, set()).add(int(s.t_step))


def set_clocks(replay, source, n):
    for m in range(n):
        replay.clock(m, source.get_state(m).t_step)


def dry_run(case, extras):
    """One case on the oracles alone - steps, stream, schedule; the generator's draws taken in the GPU test's order, the device's own draws (the twin's seeds and
    steps, the fork's seeds) taken and dropped - and what it shows of the inputs: a dict of
      peak_total, peak_side    the most resting orders a market held, both sides together (the oracle's census, inside steps too) and on one side (between launches)
      tape_bound               the largest tape_bound() of a market, from the messages it really got
      played                   Scheduled.played: (market, row, window, messages) of every non-empty play
      counts                   Scheduled.counts; trades: account trades the scheduled windows made (twice the fills: both parties count)"""
    n, a = case["n_markets"], case["cfg"]["num_of_agents"]
    rng = np.random.default_rng(case["seed"])
    ora, src = Oracles(case), Oracles(case)
    seeds = rng.integers(0, 2 ** 63, n).astype(np.uint64)
    ora.reset(seeds); src.reset(seeds)
    prefilled = np.zeros(n, np.int64)
    if case["prefill"]:
        prefill(case, (ora, src))
        for m in range(0, n, 3):
            prefilled[m] = sum(F.service_prefill_sizes(case, m))
    peak_side = 0
    peak_total = 0

    def census():
        nonlocal peak_side, peak_total
        peak_side = max([peak_side] + [max(ora.book_size(m)) for m in range(n)])
        peak_total = max([peak_total] + [int(o.book_peak()[j::ora.k].max()) for j, o in enumerate(ora.o)] + [sum(ora.book_size(m)) for m in range(n)])

    def trades():
        return sum(int(s.acc[j].num_trades) for s in (ora.get_state(m) for m in range(n)) for j in range(a))

    census()
    for _ in range(F.SERVICE_STEPS):
        acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
        ora.step(acts, present); src.step(acts, present)
        census()
    rng.integers(0, 2 ** 63, n)                                # the twin's seeds, its three steps, the fork's seeds
    for _ in range(3):
        F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
    rng.integers(0, 2 ** 63, case["fork"]["n_markets"])
    streams, pools = cut_streams(case, src, rng)
    src.close()
    for m in range(n):
        stream_into_oracle(ora, m, streams[m], a, case["clear_step_counters"])
    census()
    rows = schedule_rows(case, extras, pools)
    spec = scheduled(case, extras, ora, rows)
    made = 0
    for _ in range(F.SERVICE_STEPS_AFTER):
        before = trades()
        spec.play_all()
        made += trades() - before
        census()
        acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
        ora.step(acts, present)
        census()
    clocks = clocks_past_the_row_horizon(case, extras)         # the play past the row's horizon: the moved markets play nothing, the others their window once more
    had = move_clocks((ora,), clocks)
    quiet = spec.counts[list(clocks)].copy()
    spec.play_all()
    assert np.array_equal(spec.counts[list(clocks)], quiet)
    move_clocks((ora,), had)
    census()
    for _ in range(extras["tail_steps"]):
        acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
        ora.step(acts, present)
        census()
    flags = ora.flags()
    ora.close()
    got = np.zeros(n, np.int64)
    for m, _, _, k in spec.played:
        got[m] += k
    bound = max(tape_bound(int(prefilled[m]), a, len(streams[m]), int(got[m])) for m in range(n))
    return {"peak_total": peak_total, "peak_side": peak_side, "tape_bound": bound, "played": list(spec.played), "counts": spec.counts.copy(), "trades": made,
            "rows": rows, "flags": flags, "past_horizon": clocks}
