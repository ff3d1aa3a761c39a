"""The cases of the P&L report's tests.  (1) episode(): seeded random small episodes - tape rows and quote rows of one market - for tests/test_pnl_host.py, which
holds pnl.pnl_from_records to a scalar restatement on them.  (2) DEVICE_CASES: what tests/test_hip_pnl.py plays on the GPU - shapes, ring sizes, stops - with
actions(), the draws of every step, and replay(): the same cases on the CPU oracle with the quote recorder's host replay (tests/quote_replay.py), which shows
without a device that the played episodes hold what the comparison is about.  No device code."""
import numpy as np

BARS = (1, 2, 3, 7)


# ---- 1. random small episodes ---------------------------------------------------------------------------------------------------------------
def episode(rng):
    """one market's episode: {"tape": int32 [K, 8] in step order, "quotes": int32 [S, 8] consecutive steps, "agents", "bar", "tape_lost", "quote_lost"}.
    agents 1 .. 16; 0 .. 200 quote steps; 0 .. 300 fills, some self-trades; one-sided and empty stretches at the start, in the middle and at the end; a quote head
    or a tape head cut off in some; fills beyond the last quote in some."""
    agents = int(rng.integers(1, 17))
    steps = int(rng.choice([0, 1, 2, int(rng.integers(3, 64)), int(rng.integers(64, 201))], p=[0.04, 0.04, 0.04, 0.44, 0.44]))
    quote_lost = int(rng.integers(1, 40)) if rng.random() < 0.3 else 0                      # the quotes start at this step
    flags = np.where(rng.random(steps) < 0.85, 3, rng.integers(0, 3, steps))
    for where in ("start", "middle", "end"):
        if steps and rng.random() < 0.5:
            k = int(rng.integers(1, max(2, steps // 3 + 1)))
            at = 0 if where == "start" else steps - k if where == "end" else int(rng.integers(0, steps - k + 1))
            flags[at:at + k] = rng.integers(0, 3)
    mid = 700 + np.cumsum(rng.integers(-3, 4, steps))               # (200 steps of at most 3 down: prices stay positive)
    quotes = np.zeros((steps, 8), np.int32)
    for i in range(steps):
        bid, ask = int(mid[i]) - int(rng.integers(0, 3)), int(mid[i]) + 1 + int(rng.integers(0, 3))
        quotes[i] = (quote_lost + i, flags[i], bid if flags[i] & 1 else 0, ask if flags[i] & 2 else 0, 5, 6, 1, 1)
    fills = int(rng.choice([0, 1, int(rng.integers(2, 64)), int(rng.integers(64, 301))], p=[0.06, 0.04, 0.45, 0.45]))
    last = quote_lost + steps - 1 + (int(rng.integers(1, 10)) if rng.random() < 0.3 else 0)  # the last step a fill may carry: beyond the last quote in some
    tape_lost = int(rng.integers(1, 50)) if rng.random() < 0.3 else 0                       # records of the head the ring has lost: the tape starts later
    first = min(int(rng.integers(1, 30)), max(last, 0)) if tape_lost else 0
    at = np.sort(rng.integers(first, max(last, first) + 1, fills))
    tape = np.zeros((fills, 8), np.int32)
    for i in range(fills):
        cid = int(rng.integers(0, agents))
        iid = cid if rng.random() < 0.1 else int(rng.integers(0, agents))
        side = int(rng.integers(0, 2))                                                       # the initiator's; the counterparty has the other
        tape[i] = (i, 40 + int(rng.integers(0, 40)), 1 + int(rng.integers(0, 30)), cid, i, 0, iid, (int(at[i]) << 2) | (side << 1) | (1 - side))
    return {"tape": tape, "quotes": quotes, "agents": agents, "bar": int(rng.choice(BARS)), "tape_lost": tape_lost, "quote_lost": quote_lost}


def episodes(seed, count):
    rng = np.random.default_rng(seed)
    return [episode(rng) for _ in range(count)]


# ---- 2. what the GPU test plays ----------------------------------------------------------------------------------------------------------------
def _case(name, n, a, max_step, stops, tape_cap=2048, quote_cap=512, seed=0, bars=(1, 7)):
    return {"name": name, "n": n, "a": a, "max_step": max_step, "stops": tuple(stops), "tape_cap": tape_cap, "quote_cap": quote_cap, "seed": seed, "bars": tuple(bars)}


# stops: the step counts at which the report is compared, on the current and on the previous episode - mid-episode first, then behind the auto reset
DEVICE_CASES = [
    _case("base", 24, 4, 150, (100, 180)),
    _case("agents2", 8, 2, 70, (50, 100), seed=1),
    _case("agents5", 8, 5, 70, (50, 100), seed=2),
    _case("agents16", 8, 16, 70, (50, 100), seed=3),
    _case("pass64", 8, 4, 64, (74,), seed=4),                       # the scan passes' borders: episodes of exactly 64, 65 and 128 points
    _case("pass65", 8, 4, 65, (75,), seed=5),
    _case("pass128", 8, 4, 128, (138,), seed=6),
    _case("small_rings", 24, 4, 150, (100, 180), tape_cap=64, quote_cap=64, seed=7),
]
REPLAY_MARKETS = 6                                                  # replay() follows the first markets of a case: the GPU test plays them too


def case(name):
    return next(c for c in DEVICE_CASES if c["name"] == name)


def seeds(c):
    return np.arange(900 + c["seed"], 900 + c["seed"] + c["n"], dtype=np.uint64)


def actions(rng, n, a):
    """one step's env actions for n markets x a agents (the draws of tests/test_hip_tape.py _actions)"""
    return (rng.integers(0, 9, (n, a)).astype(np.int32), rng.uniform(-1, 1, (n, a)).astype(np.float32), rng.uniform(0, 1, (n, a)).astype(np.float32),
            rng.integers(0, 10, (n, a)).astype(np.int32), rng.integers(0, 3, (n, a)).astype(np.int32))


def _resting(ora, side, trader):
    """order id -> quantity of the trader's resting orders on one side of the oracle's market 0"""
    return {int(r[3]): int(r[1]) for r in ora.get_book(0, side) if int(r[2]) == trader}


def self_trades(c, markets=2, steps=60):
    """The self-trades the first `steps` steps of the case's first `markets` markets make, counted on the CPU.  The oracle keeps no tape and a self-trade moves no
    trade counter, so a shadow oracle replays every step order by order: it takes the market's state ahead of the step, then the step's decoded orders in their
    execution order through the one-order hook; a market or limit order that consumes a resting order of its OWN trader on the other side is a self-trade."""
    import oracle_lib as O
    import schedule_util as U
    from gym_continuousdoubleauction_amd import _capi as K
    from gym_continuousdoubleauction_amd import orders as OR
    n, a, k = c["n"], c["a"], min(markets, c["n"])
    cfg = {"num_of_agents": a, "init_cash": 1000000, "max_step": c["max_step"], "is_render": False}
    ora, shadow = O.OracleEnv(cfg, n_markets=k), O.OracleEnv(cfg, n_markets=1)
    ora.reset(seeds=seeds(c)[:k])
    shadow.reset(seeds=seeds(c)[:1])
    rng = np.random.default_rng(c["seed"])
    found = 0
    for _ in range(min(steps, c["max_step"] - 1)):                  # (inside the first episode: no reset to follow)
        states = [ora.get_state(m) for m in range(k)]
        acts = [x[:k] for x in actions(rng, n, a)]
        *_, info = ora.step(*acts)
        for m in range(k):
            shadow.set_state(0, states[m])
            order = [ora.trace[m].exec_order[j] for j in range(a)]
            for msg in OR.from_lob_actions(info["lob_actions"][m][None], [order]):
                tr, typ, side = msg[:3]
                if typ not in (K.T_MARKET, K.T_LIMIT):
                    U.play_hooks(shadow, 0, [msg])
                    continue
                before = _resting(shadow, 1 - side, tr)
                U.play_hooks(shadow, 0, [msg])
                after = _resting(shadow, 1 - side, tr)
                found += sum(1 for oid, q in before.items() if after.get(oid, 0) < q)
            for side in (0, 1):                                      # the shadow followed the step: the same book stands behind both
                assert np.array_equal(shadow.get_book(0, side)[:, :3], ora.get_book(m, side)[:, :3]), (c["name"], m, side)
    ora.close(); shadow.close()
    return found


def replay(c, markets=REPLAY_MARKETS):
    """The case on the CPU: the oracle with the env's auto-reset rule plays the first `markets` markets, the quote replay records the top of every book ahead of
    every step, and the steps' trade counters give the non-self fills of every step (each counts for both parties; a self-trade moves no counter, so the replay
    cannot see one).  -> per stop, per episode ("current", "previous"), per market a dict: quotes (the held rows), quote_lost, fills (non-self fills per step of
    that episode, a list over its steps), tape_lost (non-self fills the tape ring of the case's size has at least lost of that episode's head)."""
    import oracle_lib as O
    import services_fuzz_util as SU
    from quote_replay import QuoteReplay
    n, a, k = c["n"], c["a"], min(markets, c["n"])
    cfg = {"num_of_agents": a, "init_cash": 1000000, "max_step": c["max_step"], "is_render": False}
    ora = O.OracleEnv(cfg, n_markets=k)
    mini = {"cfg": cfg, "rows": None, "n_markets": k}
    rp = QuoteReplay(k, c["quote_cap"])
    ora.reset(seeds=seeds(c)[:k])
    rng = np.random.default_rng(c["seed"])
    now, before = [[] for _ in range(k)], [[] for _ in range(k)]   # non-self fills per step of the current / previous episode
    out = []
    for t in range(1, max(c["stops"]) + 1):
        SU.feed_quotes([rp], ora, mini)
        acts = [x[:k] for x in actions(rng, n, a)]
        _, _, term, trunc, info = ora.step(*acts)
        per_step = info["num_trades_step"].sum(axis=1) // 2
        done = (term != 0) | (trunc != 0)
        for m in range(k):
            now[m].append(int(per_step[m]))
            if done[m]:
                before[m], now[m] = now[m], []
        if done.any():
            ora.reset(None, done.astype(np.uint8))
        SU.set_clocks(rp, ora, k)
        if t in c["stops"]:
            stop = {}
            for which, fills_of, newer in (("current", now, None), ("previous", before, now)):
                rows = []
                for m in range(k):
                    q, _, lost, _, _ = rp.held(m, which)
                    behind = sum(newer[m]) if newer is not None else 0                     # what the ring holds behind this episode
                    rows.append({"quotes": q, "quote_lost": lost, "fills": list(fills_of[m]),
                                 "tape_lost": max(0, min(sum(fills_of[m]), sum(fills_of[m]) + behind - c["tape_cap"]))})
                stop[which] = rows
            out.append(stop)
    ora.close()
    return out
