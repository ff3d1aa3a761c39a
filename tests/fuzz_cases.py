"""Random env configurations and action laws shared by the build-container cross-check of the oracle against the reference
(tests/golden/crosscheck_oracle.py) and the GPU fuzz tests of the HIP path against the oracle; service_case() draws, on top of a configuration, what
the device services are fuzzed with (tests/test_hip_services_fuzz.py: the legs steps, book_report, scripted, tape, snapshot, order_stream, steps_after and end),
and service_extras(), from a generator of its own, what the legs quotes and schedule are run with - ten legs in all.  edge_case() / edge_cases() draw, again from a
generator of their own, configurations on the border of the accepted domain (tests/test_hip_config_edges.py; tests/test_config_edges_host.py holds them to
their coverage), and in_reach() states when such a case is one the device and the oracle must agree on bit for bit."""
import numpy as np


def random_config(rng):
    A = int(rng.choice([2, 3, 4, 5, 8, 12, 16]))
    cfg = {"num_of_agents": A, "init_cash": int(rng.choice([400, 3000, 50000, 1000000, 1000000, 50000000000])),
           "max_step": 4096, "is_render": False, "n_hist": int(rng.choice([1, 2, 4, 4, 6]))}
    if rng.random() < 0.4:
        lo = int(rng.choice([1, 10, 500, 20000]))
        cfg.update(initial_price_min=lo, initial_price_max=lo + int(rng.integers(0, 300)))
    if rng.random() < 0.4:
        cfg.update(min_size=int(rng.integers(1, 5)), mkt_max_size=int(rng.choice([20, 100, 3000])), limit_size_multiple=int(rng.choice([1, 3, 10, 20])))
    if rng.random() < 0.3:
        cfg.update(order_penalty=float(rng.uniform(0, 1)), trade_penalty=float(rng.uniform(0, 1)), drawdown_penalty=float(rng.uniform(0, 1)),
                   passive_bonus=float(rng.uniform(0, 1)), loss_multiplier=float(rng.uniform(1, 3)))
    law = str(rng.choice(["uniform", "uniform", "aggressive", "edges", "trend"]))
    present_p = None if rng.random() < 0.7 else float(rng.uniform(0.3, 0.9))
    if rng.random() < 0.3:                                    # an integer tick other than 1 (round 6): the ladder's step and the unit of the observation's spread
        cfg["tick_size"] = int(rng.choice([2, 3, 5, 10, 250]))
    return cfg, law, present_p


def random_order(rng):
    """how the caller's action dicts are keyed: None = ascending agent ids, "shuffle" = a new random key order every step"""
    return "shuffle" if rng.random() < 0.35 else None


def prefill_book(env, market, rng, agents, n_bids, n_asks, qty=(1, 6), level_orders=(1, 5)):
    """Give `market` of `env` (product or oracle: same get_state / set_state) a deep book through the state dump: n_bids / n_asks
    resting orders (up to 512 per side, far more than the LDS tile) in levels of one to four orders around the market's price,
    with the traders' escrow (cash_on_hold) set to match.  Both envs get the same book when called with equally seeded `rng`s.
    qty / level_orders: the half-open ranges an order's quantity and a level's number of orders are drawn from."""
    from decimal import Decimal

    from gym_continuousdoubleauction_amd import _capi as K
    s = env.get_state(market)
    lp = max(2, int(s.last_price))
    hold = [0] * agents
    oid = 0
    for side, n, arr in ((0, n_bids, s.bids), (1, n_asks, s.asks)):
        price, left_in_level = (lp - 1 if side == 0 else lp + 1), int(rng.integers(*level_orders))
        for k in range(n):
            if left_in_level == 0:
                step = int(rng.integers(1, 3))
                price = max(1, price - step) if side == 0 else price + step
                left_in_level = int(rng.integers(*level_orders))
            left_in_level -= 1
            o = arr[k]
            oid += 1
            o.price, o.qty, o.owner, o.order_id, o.timestamp = price, int(rng.integers(*qty)), int(rng.integers(0, agents)), oid, oid
            hold[o.owner] += o.price * o.qty
    s.n_bids, s.n_asks = n_bids, n_asks
    s.lob_time = s.next_order_id = oid
    for j in range(agents):
        cash = K.dec_to_decimal(s.acc[j].cash)
        s.acc[j].cash_on_hold = K.decimal_to_dec(Decimal(hold[j]) * Decimal("1.0"))
        s.acc[j].cash = K.decimal_to_dec(cash - Decimal(hold[j]) * Decimal("1.0"))
    env.set_state(market, s)


def batch_actions(rng, n, a, law, present_p, order=None):
    """[n, a] action arrays under one of the golden generator's laws, plus `present` (or None): a 0 / 1 mask, or - order ==
    "shuffle" - each market's own random dict order (0 = absent, else 1 + position in the dict; cda_step's encoding)."""
    if law == "uniform":
        cat, price, off = rng.integers(0, 9, (n, a)), rng.integers(0, 10, (n, a)), rng.integers(0, 3, (n, a))
        mean, sigma = rng.uniform(-1, 1, (n, a)), rng.uniform(0, 1, (n, a))
    elif law == "aggressive":
        cat, price, off = rng.choice([1, 2, 2, 5, 6, 6, 3, 7, 4, 8], (n, a)), rng.integers(0, 3, (n, a)), rng.choice([1, 2, 2], (n, a))
        mean, sigma = rng.uniform(-0.05, 0.05, (n, a)), rng.uniform(0, 1, (n, a))
    elif law == "trend":
        cat = rng.choice([2, 2, 2, 2, 2, 6, 6, 6, 1, 1, 1, 5, 3, 7, 4, 8, 0], (n, a))
        price, off = rng.choice([0, 0, 0, 1, 2, 5, 9], (n, a)), rng.choice([2, 2, 1, 0], (n, a))
        mean, sigma = rng.uniform(-0.004, 0.004, (n, a)), rng.uniform(0, 1, (n, a))
    else:
        cat, price, off = rng.integers(0, 9, (n, a)), rng.choice([0, 9], (n, a)), rng.choice([0, 2], (n, a))
        mean, sigma = rng.choice([-1.0, 1.0, 0.0], (n, a)), rng.choice([0.0, 1.0], (n, a))
    present = None if present_p is None else (rng.uniform(0, 1, (n, a)) < present_p).astype(np.uint8)
    if order == "shuffle":
        mask = np.ones((n, a), np.uint8) if present is None else present
        keys = rng.random((n, a)) + (mask == 0) * 2.0                      # absent agents sort last
        rank = np.argsort(np.argsort(keys, axis=1), axis=1)                 # 0-based position of each agent in its market's dict
        present = np.where(mask != 0, rank + 1, 0).astype(np.uint8)
    return (cat.astype(np.int32), mean.astype(np.float32), sigma.astype(np.float32), price.astype(np.int32), off.astype(np.int32)), present


# ---------------------------------------------------------------------------------------------------------------- service cases
SERVICE_SEED = 20277                                 # the default CDA_FUZZ_SEED of the services fuzz: tests/test_services_fuzz_host.py holds its cases to the coverage
SERVICE_CASES = 12
SERVICE_MARKETS = 24                                 # six workgroups of CDA_WPB = 4 market-waves, the last one full ...
RAGGED_CASE, RAGGED_MARKETS = 5, 22                  # ... and in one case ragged: two waves of the last workgroup leave at once
SERVICE_HISTS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 16)
STREAM_LENGTHS = (0, 1, 63, 64, 65, 129)             # around the order kernel's chunk of 64 messages
SERVICE_STEPS, SERVICE_STEPS_AFTER, STREAM_SOURCE_STEPS = 40, 16, 16
# one invalid message of each kind (tests/test_hip_orders.py test_invalid_messages_are_skipped_and_reported): trader = A, type 5, side 2, size 0, price 0 on a limit
def invalid_messages(a):
    return [(a, 1, 0, 5, 50, 0), (0, 5, 0, 5, 50, 0), (0, 1, 2, 5, 50, 0), (0, 1, 0, 0, 50, 0), (0, 1, 0, 5, 0, 0)]


def tile_of(cfg):
    """the LDS book tile cda_create picks (include/cda.h book_capacity: 0 = by agent count)"""
    return int(cfg.get("book_capacity", 0)) or (256 if cfg["num_of_agents"] <= 8 else 512)


def row_in_domain(cfg, row):
    """cda_check_market_params' rule on plain numbers (csrc/cda_hip.hip cfg_ok + row_ok), so that the generator can redraw without a library"""
    c = dict(cfg, **row)
    lo, hi = c.get("initial_price_min", 10), c.get("initial_price_max", 10)
    mn, mx, mul = c.get("min_size", 1), c.get("mkt_max_size", 1), c.get("limit_size_multiple", 1)
    return (1 <= c.get("tick_size", 1) <= 65536 and 0 <= lo <= hi < (1 << 24) and 1 <= mn <= mx and mul >= 1 and mx * mul + mn <= (1 << 30) // 512
            and 1 <= c["max_step"] <= cfg["max_step"] and abs(c.get("init_cash", 0)) <= 1 << 62)


def granted_ring(cfg):
    """the HBM ring per side cda_create grants a config (csrc/cda_hip.hip), device memory permitting: what was asked for - automatic: num_agents x max_step, at
    least 1024 - rounded up to a power of two; an automatic ring is halved while the config's largest order size times tile + ring would leave int32, an explicit
    one (book_spill > 0) that would is refused: ValueError"""
    from gym_continuousdoubleauction_amd import _capi as K
    c = K.make_config(cfg)[1]
    if c["book_spill"] < 0:
        return 0
    want = c["book_spill"] if c["book_spill"] > 0 else max(1024, c["num_of_agents"] * c["max_step"])
    ring = 64
    while ring < want and ring < (1 << 20):
        ring <<= 1
    scale = c["mkt_max_size"] * c["limit_size_multiple"] + c["min_size"]
    while ring > 64 and scale * (tile_of(cfg) + ring) > 0x7fffffff:
        if c["book_spill"] > 0:
            raise ValueError(f"cda_create refuses book_spill {c['book_spill']} for order sizes up to {scale}")
        ring >>= 1
    return ring


def row_fits_ring(cfg, row):
    """cda_set_market_params' further rule (csrc/cda_hip.hip): the env's ring was cut for the CONFIG's order sizes, and a row must keep to that ring - its largest
    decodable size times tile + ring stays in int32.  (CDA_FUZZ_SEED=90417 drew, as case 110, 16 agents x 4096 steps - a ring of 65536 - with a row of sizes up to
    60003: the env refused it at construction.)"""
    from gym_continuousdoubleauction_amd import _capi as K
    c = K.make_config(dict(cfg, **row))[1]
    ring = granted_ring(cfg)
    return ring == 0 or (c["mkt_max_size"] * c["limit_size_multiple"] + c["min_size"]) * (tile_of(cfg) + ring) <= 0x7fffffff


def _service_row(rng, cfg, short):
    row = {"tick_size": int(rng.choice([1, 1, 2, 5, 10, 250]))}
    lo = int(rng.choice([1, 10, 500, 20000]))
    row.update(initial_price_min=lo, initial_price_max=lo + int(rng.integers(0, 300)))
    row.update(min_size=int(rng.integers(1, 5)), mkt_max_size=int(rng.choice([20, 100, 3000])), limit_size_multiple=int(rng.choice([1, 3, 10, 20])))
    row["max_step"] = int(rng.integers(4, cfg["max_step"] + 1)) if short else int(rng.choice([256, 1000, 4096]))
    row.update(order_penalty=float(rng.uniform(0, 1)), trade_penalty=float(rng.uniform(0, 1)), drawdown_penalty=float(rng.uniform(0, 1)),
               passive_bonus=float(rng.uniform(0, 1)), loss_multiplier=float(rng.uniform(1, 3)))
    return row


def _service_profile(rng, law):
    from gym_continuousdoubleauction_amd.scripted import Profile
    cap = int(rng.integers(0, 61))
    den = int(rng.integers(1, 4))
    return Profile(law=law, size_mean=float(rng.uniform(0, 0.3)), size_sigma=float(rng.uniform(0, 0.3)), max_position=cap, skew_position=int(rng.integers(0, cap + 1)),
                   max_orders=int(rng.integers(1, 5)), depth_levels=int(rng.integers(1, 11)), imb_num=den + int(rng.integers(0, 4)), imb_den=den,
                   p_trade_q32=int(rng.choice([0, 1 << 30, 1 << 31, 1 << 32, int(rng.integers(0, 1 << 32))])))


def service_case(rng, n_markets=SERVICE_MARKETS):
    """One case of the services fuzz: random_config's draws first (the config, the law, the subset probability), then everything the services are run with.
    Pure host code; every value is a plain number, list or numpy array.  The env config is case["cfg"]; case["oracle_cfg"] is the same without the keys the
    oracle does not take; market m runs case["rows"][m % k] when the case has per-market rows."""
    cfg, law, present_p = random_config(rng)
    order = random_order(rng)
    n, a = int(n_markets), cfg["num_of_agents"]
    cfg["n_hist"] = int(rng.choice(SERVICE_HISTS))
    cfg["book_capacity"] = int(rng.choice([0, 0, 256, 512]))
    # A small explicit ring (a third of all cases) makes a wrapped window reachable.  The oracle's book is unbounded while the device drops (and flags) a rest beyond
    # tile + ring, so the book must stay inside: the trend law (tiny sizes, mostly limit orders: several resting orders more per step and agent count) is left
    # out, and service_prefill_sizes keeps a prefilled book of such a case close to the tile.
    small_ring = law != "trend" and rng.random() < 0.42
    if small_ring:
        cfg["book_spill"] = int(rng.choice([64, 128]))
    short = bool(rng.random() < 0.25)                     # the short horizon: episodes end, and auto reset, inside the case
    if short:
        cfg.update(max_step=int(rng.integers(6, 15)), auto_reset=True)
    rows = None
    if rng.random() < 0.5:
        rows, k = [], int(rng.choice([2, 3]))
        while len(rows) < k:                                  # (validated on the host and redrawn; distinct)
            row = _service_row(rng, cfg, short)
            if row_in_domain(cfg, row) and row_fits_ring(cfg, row) and row not in rows:
                rows.append(row)
    n_prof = int(rng.integers(3, 7))                          # the four laws in a random order, then two more drawn: the first n_prof of them
    laws = ([1 + int(x) for x in rng.permutation(4)] + [int(x) for x in rng.integers(1, 5, 2)])[:n_prof]
    profiles = [_service_profile(rng, int(w)) for w in laws]
    slots = rng.integers(1, n_prof + 1, (n, a)).astype(np.int32)
    slots[rng.random((n, a)) < 0.35] = 0
    lengths = rng.choice(STREAM_LENGTHS, n).astype(np.int64)
    long_enough = np.flatnonzero(lengths >= 63)
    case = {
        "cfg": cfg, "oracle_cfg": {k: v for k, v in cfg.items() if k != "auto_reset"}, "law": law, "present_p": present_p, "order": order, "n_markets": n,
        "rows": rows, "short": short, "small_ring": small_ring, "tile": tile_of(cfg),
        "seed": int(rng.integers(0, 2 ** 62)),               # of the test's own generator: reset seeds, actions, positions of the spliced messages
        "prefill": bool(rng.random() < 0.4), "prefill_seed": int(rng.integers(0, 2 ** 31)),
        "profiles": profiles, "slots": slots, "script_seed": int(rng.integers(0, 2 ** 62)), "script_base": int(rng.integers(0, 10 ** 6)),
        "script_draw": int(rng.integers(0, 1000)), "script_counter": int(rng.integers(0, 50)),
        "stream_lengths": lengths, "mark_every": int(rng.integers(0, 7)),
        "invalid_markets": sorted(int(x) for x in rng.choice(long_enough if len(long_enough) >= 2 else np.arange(n), 2, replace=False)),
        "max_per_launch": int(rng.choice([16, 50, 64])), "split_twin": bool(rng.random() < 0.5), "clear_step_counters": bool(rng.random() < 0.5),
        "bar_steps": int(rng.integers(1, 9)), "n_bars": int(rng.integers(1, 13)),
        "horizons": sorted({int(x) for x in rng.choice([0, 1, 2, 5, 20, 1000], int(rng.integers(1, 5)))}),
        "levels": int(rng.integers(1, 41)), "impact_sizes": sorted({int(x) for x in rng.choice([1, 2, 7, 33, 150, 10 ** 6], int(rng.integers(1, 5)))}),
    }
    n3 = int(rng.integers(5, 17))                             # the env of another size a sub-range is restored into
    cnt = int(rng.integers(1, min(n3, n) + 1))
    case["fork"] = {"n_markets": n3, "n": cnt, "first": int(rng.integers(0, n3 - cnt + 1)), "src_first": int(rng.integers(0, n - cnt + 1))}
    return case


def service_prefill_sizes(case, market):
    """(n_bids, n_asks) of a prefilled market (every third one of a prefilled case): up to 512 per side - tile and ring both in play; with a small explicit
    ring each side stays within a quarter of the ring around half the tile: the largest books start beyond the tile, in the ring, and every side has most of its
    ring left for what the law adds (the device drops and flags a rest beyond tile + ring, the oracle's book is unbounded: such a case would fail on its flags)."""
    r = np.random.default_rng(case["prefill_seed"] + market)
    if not case["small_ring"]:
        return tuple(int(x) for x in r.integers(0, 513, 2))
    half, quarter = case["tile"] // 2, case["cfg"]["book_spill"] // 4
    return tuple(int(x) for x in r.integers(half - quarter, half + quarter + 1, 2))


# ---------------------------------------------------------------------------------------------------------------- what the quotes and schedule legs are run with
EXTRAS_STREAM = 0x5C4ED                              # service_extras' own generator: [case["seed"], EXTRAS_STREAM]
QUOTE_CAPACITIES = (8, 24, 40, 64, 128)              # quote rings: 8 and 24 wrap inside the 56 steps of a long case; 24 and 40 are no powers of two
SCHEDULE_EDGES = (63, 64, 65, 130)                   # schedule_util.EDGE_LENGTHS without 0 and 1: around the message walk's chunk of 64
SCHEDULE_WINDOW_MAX = max(SCHEDULE_EDGES)            # the longest window (the five invalid messages go into a small one: 9 + 5 at the most)
INVALID_KINDS = 5                                    # len(invalid_messages(a))
SERVICE_STEPS_TAIL = 10                              # 40 + 16 + 10 steps = 66 quotes of one episode: more than the quote readers' pass of 64 records


def schedule_reach(case, n_windows, loop):
    """THE WINDOW RULE: the windows of a schedule of `n_windows` windows that the schedule leg of `case` reaches in every market that plays a row.  The leg is
    SERVICE_STEPS_AFTER = 16 steps behind SERVICE_STEPS = 40 steps (the order stream between them moves no clock).
      long horizon    every market is at t_step 40 .. 55: with loop the windows {t % n_windows}, without it the windows 40 .. min(n_windows, 56) - 1.
      short horizon   every episode is shorter than 16 steps, so every market passes every t_step 0 .. H - 1 of its own horizon H >= H_min (the smallest max_step of
                      the case, rows included): the windows 0 .. min(n_windows, H_min) - 1, with loop or without.
    service_extras puts messages into these windows only, so every drawn length is played."""
    lo, hi = SERVICE_STEPS, SERVICE_STEPS + SERVICE_STEPS_AFTER
    if case["short"]:
        h_min = min([case["cfg"]["max_step"]] + [r["max_step"] for r in case["rows"] or []])
        return list(range(min(n_windows, h_min)))
    if loop:
        return sorted({t % n_windows for t in range(lo, hi)})
    return list(range(lo, min(n_windows, hi)))


def short_quote_capacity(case, r):
    """the quote ring of a short-horizon case (auto reset, per-market horizons of 4 .. 14 steps): no power of two, and with H the case's longest horizon in
    H + 1 .. H + H // 2 - a whole episode fits, one and a half do not: once a longest-horizon market's current episode is half way, its previous one has lost
    its head"""
    h = max([x["max_step"] for x in case["rows"]] if case["rows"] else [case["cfg"]["max_step"]])
    hi = h + max(1, h // 2)
    k = int(r.integers(h + 1, hi + 1))
    if k & (k - 1) == 0:                                  # 8 or 16: the neighbour inside the range
        k = k + 1 if k + 1 <= hi else k - 1
    return k


def service_extras(case):
    """What the two legs added behind service_case - quotes and schedule - are run with, drawn from a generator of ITS OWN ([case["seed"], EXTRAS_STREAM]): not one
    draw is taken from the stream service_case draws from, so service_extras changes no case of any seed.  (What did change other seeds' streams, in the same
    commit, is service_case's own redraw of a row the env would refuse - row_fits_ring: from the first such row on, a seed's later cases are other cases.  The
    default seed draws no such row: its twelve cases are what they were.)  Plain numbers, lists and numpy arrays:
      quote_capacity     the quote rings' capacity (QUOTE_CAPACITIES; short_quote_capacity in a short-horizon case)
      tail_steps         steps of the law behind the schedule leg: SERVICE_STEPS_TAIL where a ring holds more than one pass of the readers (64 records) and the
                         horizon is long - the episode then holds 66 quotes, and the statistics' carry from one pass into the next is in play -, else 0
      schedule           n_rows (1 .. 3), n_windows (S), market_schedule int [n_markets] (at least one -1, every row played by at least two markets), loop,
                         clear_step_counters
      lengths[r][t]      messages of window t of row r, the five invalid messages included: mostly 0 (sparse flow); per row two or more windows of
                         schedule_reach(), the first of them one of SCHEDULE_EDGES, the others small counts.  On a small ring (case["small_ring"]) every window
                         is 1 .. 4 messages: the flow stays a few orders per step, as the law's, and the book inside tile + ring.
      reach              schedule_reach(case, S, loop)
      invalid            row, window, positions: where one invalid message of each kind (invalid_messages) is spliced into a small window, and a market that plays it"""
    r = np.random.default_rng([case["seed"], EXTRAS_STREAM])
    n = case["n_markets"]
    n_rows, loop, clear = int(r.integers(1, 4)), bool(r.random() < 0.5), bool(r.random() < 0.5)
    if case["short"]:
        S = int(r.integers(3, 7))
    elif loop:
        S = int(r.integers(5, 13))
    else:
        S = SERVICE_STEPS + int(r.integers(8, SERVICE_STEPS_AFTER + 1))      # 48 .. 56: the leg's last steps may lie beyond the schedule
    reach = schedule_reach(case, S, loop)
    lengths = np.zeros((n_rows, S), np.int64)
    small = []
    for row in range(n_rows):
        k = int(r.integers(2, max(2, len(reach) // 2) + 1))
        at = [int(x) for x in r.choice(reach, k, replace=False)]
        for j, t in enumerate(at):
            lengths[row, t] = int(r.integers(1, 5)) if case["small_ring"] else int(r.choice(SCHEDULE_EDGES)) if j == 0 else int(r.integers(1, 10))
        small += [(row, t) for t in (at if case["small_ring"] else at[1:])]
    perm = [int(x) for x in r.permutation(n)]
    ms = r.integers(0, n_rows, n).astype(np.int64)
    ms[r.random(n) < 0.2] = -1
    ms[perm[0]] = -1
    for row in range(n_rows):
        ms[perm[1 + 2 * row]] = ms[perm[2 + 2 * row]] = row
    bad_row, bad_window = small[int(r.integers(0, len(small)))]
    positions = sorted(int(x) for x in r.integers(0, lengths[bad_row, bad_window] + 1, INVALID_KINDS))
    lengths[bad_row, bad_window] += INVALID_KINDS
    if case["short"]:
        capacity = short_quote_capacity(case, r)
    else:
        capacity = int(r.choice(QUOTE_CAPACITIES))
    return {"quote_capacity": capacity, "tail_steps": SERVICE_STEPS_TAIL if capacity > 64 and not case["short"] else 0,
            "schedule": {"n_rows": n_rows, "n_windows": S, "market_schedule": ms, "loop": loop, "clear_step_counters": clear},
            "lengths": [[int(x) for x in row] for row in lengths], "reach": reach,
            "invalid": {"row": bad_row, "window": bad_window, "positions": positions, "market": int(np.flatnonzero(ms == bad_row)[0])}}


def service_cases(seed=SERVICE_SEED, count=SERVICE_CASES):
    """the first `count` cases of a seed's stream, in order (case RAGGED_CASE with the ragged market count)"""
    rng = np.random.default_rng(seed)
    return [service_case(rng, RAGGED_MARKETS if i == RAGGED_CASE else SERVICE_MARKETS) for i in range(count)]


# ---------------------------------------------------------------------------------------------------------------- the edges of the accepted config domain
EDGE_SEED = 86031                                    # the default CDA_FUZZ_SEED of tests/test_hip_config_edges.py: tests/test_config_edges_host.py holds its cases to the coverage
EDGE_CASES = 32                                      # case i plays 1 + i % 16 agents: every agent count twice
EDGE_STREAM = 0xED6E5                                # edge_cases' own generator: [seed, EDGE_STREAM] - not one draw from random_config's callers' streams
EDGE_MARKETS, EDGE_STEPS = SERVICE_MARKETS, 48
EDGE_RAGGED_CASE = 7                                 # the one case of RAGGED_MARKETS markets
PRICE_TOP = (1 << 24) - 1                            # the largest price of the domain (csrc/cda_hip.hip cfg_ok; a decoded price beyond it is clamped and flagged)
SCALE_MAX = (1 << 30) // 512                         # the largest mkt_max_size * limit_size_multiple + min_size
CASH_MAX = 1 << 62
HEADROOM_TICKS = 64                                  # a market of a top-of-the-domain price band starts at least this many ticks below 2^24 (see _edge_seeds)
# factor -> its levels.  A "max" level (sizes, prices or tick at the top of the domain) brings init_cash = 2^62 with it, so that the case trades instead of
# rejecting; such a level is therefore never combined with a level of init_cash, and a top price band not with a short horizon either (an in-episode reset
# draws a start price the generator has no hold on).
EDGE_LEVELS = {
    "init_cash": (-CASH_MAX, -1, 0, 1, CASH_MAX - 1, CASH_MAX),
    "tick_size": (65535, 65536),
    "price": ("zero", "one", "tick", "top"),        # (0, 0), (1, 1), (tick, tick), (2^23, 2^24 - 1)
    "scale": ("mkt", "mul1024", "mul"),             # 2^21 as mkt_max_size = 2^21 - min_size, mul = 1; as mul = 2^10; as mkt_max_size = 1, mul = 2^21 - min_size
    "flat_size": (True,),                           # mkt_max_size == min_size
    "max_step": (1, 2, 3),
    "n_hist": (1, 16),
    "book_capacity": (256, 512),
}
EDGE_LEADS = [(f, v) for f, levels in EDGE_LEVELS.items() for v in levels]       # case i holds EDGE_LEADS[i % 23] for sure, and up to two more factors drawn
# company for three cases, by case index: the three largest-scale leads fall on 13 to 15 agents (tile 512, where cda_create halves the automatic ring down to 256
# slots) - one of them is played on the small tile, where the int32 rule leaves 512 slots; init_cash = 0 is played a second time at a horizon of one step,
# where both causes of an episode's end meet on every step; and init_cash = 1 is played a second time where it can trade: an order is approved when cash >= price
# x opening size (the reference's Trader._order_approved), so with 1 of cash only one unit at a price of 1 - a start price of 1 (bids are clamped up to one tick,
# an ask one tick inside the empty side's first level lands on 1) and mkt_max_size == min_size = 1 (a market order's size is then rint(|sigma z|) + 1)
EDGE_ALSO = {13: (("book_capacity", 256),), 25: (("max_step", 1),), 26: (("price", "one"), ("flat_size", True))}
_EDGE_MAX = {("tick_size", 65535), ("tick_size", 65536), ("price", "top"), ("scale", "mkt"), ("scale", "mul1024"), ("scale", "mul")}


def _edge_allowed(held, factor, level):
    """may (factor, level) join the levels a case holds already?"""
    if factor in held or (factor == "flat_size" and "scale" in held) or (factor == "scale" and "flat_size" in held):
        return False
    has_max, has_cash = any((f, v) in _EDGE_MAX for f, v in held.items()), "init_cash" in held
    has_top, has_short = held.get("price") == "top", "max_step" in held
    if (factor, level) in _EDGE_MAX and has_cash or factor == "init_cash" and has_max:
        return False
    if (factor, level) == ("price", "top") and has_short or factor == "max_step" and has_top:
        return False
    return True


def _edge_seeds(rng, n, cfg):
    """reset seeds of a case.  Under a price band that ends at 2^24 - 1 only seeds whose market starts HEADROOM_TICKS ticks or more below the top are kept: the
    reference (and the oracle) decode prices beyond 2^24 where the device clamps and flags (tests/test_hip_domain_flags.py test_price_clamp_edge), so a case
    that is to agree bit for bit has to stay below in what it decodes.  The start price is reset's first draw, integers(lo, hi, endpoint=True) of the seed's
    PCG64 stream (tests/test_config_edges_host.py checks this restatement against the oracle)."""
    lo, hi = cfg.get("initial_price_min", 10), cfg.get("initial_price_max", 100)
    room = PRICE_TOP - HEADROOM_TICKS * cfg.get("tick_size", 1)
    seeds = []
    while len(seeds) < n:
        s = int(rng.integers(0, 2 ** 63))
        if hi <= room or int(np.random.default_rng(s).integers(lo, hi, endpoint=True)) <= room:
            seeds.append(s)
    return np.array(seeds, np.uint64)


def edge_case(rng, agents=None, lead=None, n_markets=EDGE_MARKETS, also=()):
    """One case on the border of the accepted domain: an ordinary random_config draw (from `rng`, the edge generator's own) with the agent count set, `lead` = a
    (factor, level) of EDGE_LEVELS held for sure (None: drawn), `also` = further such pairs, and up to two more factors drawn, each moved to one of its levels.  Pure host code.
    The case: cfg (the env's config; oracle_cfg: the same, the oracle takes every key), edges {factor: level}, law / present_p / order as the configuration fuzz draws
    them, n_markets, steps (EDGE_STEPS, 3 * max_step + 2 on a short horizon), seeds (uint64 per market), seed (of the test's own action generator), tile."""
    cfg, law, present_p = random_config(rng)
    order = random_order(rng)
    if agents is not None:
        cfg["num_of_agents"] = int(agents)
    if lead is None:
        lead = EDGE_LEADS[int(rng.integers(0, len(EDGE_LEADS)))]
    held = {lead[0]: lead[1]}
    for f, v in also:
        assert _edge_allowed(held, f, v), (held, f, v)
        held[f] = v
    for _ in range(int(rng.integers(0, 3))):
        f, v = EDGE_LEADS[int(rng.integers(0, len(EDGE_LEADS)))]
        if len(held) < 3 and _edge_allowed(held, f, v):       # one to three factors at an edge
            held[f] = v
    if any((f, v) in _EDGE_MAX for f, v in held.items()):
        cfg["init_cash"] = CASH_MAX
    for f in ("init_cash", "tick_size", "max_step", "n_hist", "book_capacity"):
        if f in held:
            cfg[f] = held[f]
    tick = cfg.get("tick_size", 1)
    if "price" in held:
        lo, hi = {"zero": (0, 0), "one": (1, 1), "tick": (tick, tick), "top": (1 << 23, PRICE_TOP)}[held["price"]]
        cfg.update(initial_price_min=lo, initial_price_max=hi)
    mn = cfg.get("min_size", 1)
    if held.get("scale") == "mkt":
        cfg.update(min_size=mn, mkt_max_size=SCALE_MAX - mn, limit_size_multiple=1)
    elif held.get("scale") == "mul1024":                  # 2047 * 1024 + 1024
        cfg.update(min_size=1024, mkt_max_size=(SCALE_MAX - 1024) // 1024, limit_size_multiple=1024)
    elif held.get("scale") == "mul":
        cfg.update(min_size=1, mkt_max_size=1, limit_size_multiple=SCALE_MAX - 1)
    elif held.get("flat_size"):
        if cfg["init_cash"] == 1:                             # (see EDGE_ALSO: one unit is all that 1 of cash buys)
            mn = 1
        cfg.update(min_size=mn, mkt_max_size=mn, limit_size_multiple=cfg.get("limit_size_multiple", 10))
    short = "max_step" in held
    n = int(n_markets)
    return {"cfg": cfg, "oracle_cfg": dict(cfg), "edges": held, "law": law, "present_p": present_p, "order": order, "n_markets": n, "short": short,
            "broke": cfg["init_cash"] <= 0, "steps": 3 * cfg["max_step"] + 2 if short else EDGE_STEPS, "tile": tile_of(cfg),
            "seeds": _edge_seeds(rng, n, cfg), "seed": int(rng.integers(0, 2 ** 62))}


def edge_cases(seed=EDGE_SEED, count=EDGE_CASES):
    """the first `count` edge cases of a seed, in order: case i plays 1 + i % 16 agents and holds EDGE_LEADS[i % len(EDGE_LEADS)] (with EDGE_ALSO's company);
    case EDGE_RAGGED_CASE has the ragged market count"""
    rng = np.random.default_rng([int(seed), EDGE_STREAM])
    return [edge_case(rng, 1 + i % 16, EDGE_LEADS[i % len(EDGE_LEADS)], RAGGED_MARKETS if i == EDGE_RAGGED_CASE else EDGE_MARKETS,
                      also=EDGE_ALSO.get(i, ())) for i in range(count)]


def edge_actions(case):
    """the case's own action stream: a generator to hand to batch_actions step by step"""
    return np.random.default_rng([case["seed"], EDGE_STREAM])


def in_reach(case, oracle_env, trace=None):
    """Is `case`, as far as `oracle_env` has played it, one the device must reproduce bit for bit?  None if so, else the reason as a string:
      every price the oracle decoded in its last step is below 2^24 (`trace`, default oracle_env.trace: beyond, the device clamps and flags where the reference goes on);
      every side of every book is within the LDS tile + the granted HBM ring (the oracle's book is unbounded, the device drops and flags a rest beyond);
      the oracle's flags are 0.
    Call it after every step: the decoded prices are the last step's."""
    trace = oracle_env.trace if trace is None else trace
    a = case["cfg"]["num_of_agents"]
    for m in range(oracle_env.n):
        worst = max(trace[m].dec_price[:a])
        if worst > PRICE_TOP:
            return f"market {m} decoded the price {worst} >= 2^24"
    room = case["tile"] + granted_ring(case["cfg"])
    for m in range(oracle_env.n):
        nb, na = oracle_env.book_size(m)
        if max(nb, na) > room:
            return f"market {m} holds {nb} bids / {na} asks, the device {room} per side"
    if oracle_env.flags().any():
        return f"the oracle's flags are {oracle_env.flags()}"
    return None
