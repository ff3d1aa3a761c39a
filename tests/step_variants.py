"""Test helper (host only: nothing here touches the GPU): the scenarios that walk the step-kernel instance table, and their oracle side.

The env launches one of about two dozen step instances (csrc/cda_kernels.inc, cda_policy_step.inc): by tile (cap256 / cap512), info tensors, episode metrics, trade
tape, and whether the market is cold (market_is_cold: resting orders + agents > tile, or a tail bit) and goes to the out-of-line general build.  ROWS below is the
matrix tests/test_hip_step_variants.py runs with episode metrics ON; tests/test_step_variants_host.py checks on the oracle alone that every row meets what it claims.

A row: the launch path, the tile, tape on / off, the book at the first episode's end, agents, groups, the account size, max_step and the batch.  Every row plays
3 max_step + 2 steps: a prefilled market ends its FIRST episode cold, the auto reset empties its book and its later episodes end hot - both branches in one run.

  path step          cda_step, with_info=False: the in-kernel auto reset (k_step<false, 1>; k_tstep<false> with the tape)
       step_info     cda_step, with_info=True: the k_reset pass behind the step (k_step<true, 1>; k_tstep<true>)
       run_random    one launch per episode, no auto reset: launch, collect, reset, launch ... (k_run_random<1>; k_tape_run)
       rollout       mlp.RolloutChains, the policy inside the step kernel where the env qualifies (k_policy_step<1>; tile 512 or 16 agents: policy launch + k_step)
       rollout_tape  the same chains with the tape on: policy launch + k_tstep<false>
  book shallow       never cold
       cold          prefilled to the tile's brim: everything in the tile, nb + na + agents > tile
       spilled       prefilled beyond the tile: both sides continue in the HBM ring (300 + 300 at tile 256; 500 + 500 at tile 512 - the state dump holds at most
                     512 orders per side)
       the run_random rows with a prefill leave every fourth market ON THE BRINK instead (nb + na + agents == tile: hot, one more resting order and it is cold):
       there the hot kernel hands the episode to the general build in the middle of a launch.
  rollout rows use max_step 6 and a horizon of 5 steps (4 x 5 = 3 x 6 + 2): the book is looked at after the first run (before the step that ends the first episode),
  the first collection follows the second run - only first episodes have ended by then.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ACTION_KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset")
SMALL = 3500            # the small account: bankruptcies, and episodes that end `terminated`
PATHS = ("step", "step_info", "run_random", "rollout", "rollout_tape")
FACTORS = {"path": PATHS, "tile": (256, 512), "tape": (False, True), "book": ("shallow", "cold", "spilled"), "agents": (4, 8, 16), "groups": (1, 3),
           "cash": (1000000, SMALL)}


# the small account on an empty book trades sizes that can sink it (market orders of up to ~200 at prices of 10 .. 20); where its book is prefilled the sizes stay
# small, so that the resting single units are not swept away before the first episode ends
SINK = {"initial_price_min": 10, "initial_price_max": 20, "mkt_max_size": 200, "limit_size_multiple": 4}
FIRM = {"mkt_max_size": 20}     # a book at the tile's brim is cold by a margin of `agents` orders: market orders smaller than a resting order leave it standing
MILD = {"initial_price_min": 10, "initial_price_max": 20, "mkt_max_size": 10, "limit_size_multiple": 2}


def _row(path, tile, tape, book, agents, groups, cash, max_step, N, seed, law="uniform", cfg=None):
    return {"path": path, "tile": tile, "tape": tape, "book": book, "agents": agents, "groups": groups, "cash": cash, "max_step": max_step, "N": N, "seed": seed,
            "law": law, "cfg": cfg or {}}


ROWS = [
    # gap 1: a cold market under the tallies, every path
    _row("step", 256, False, "cold", 4, 1, 1000000, 7, 41, 1100, cfg=FIRM),
    _row("step", 512, False, "cold", 16, 3, 1000000, 5, 38, 1200, cfg=FIRM),
    _row("step_info", 256, False, "cold", 8, 1, 1000000, 6, 41, 1300, cfg=FIRM),
    _row("rollout", 256, False, "cold", 4, 3, 1000000, 6, 41, 1400, cfg=FIRM),
    _row("run_random", 256, False, "spilled", 8, 1, 1000000, 7, 38, 1500),
    # gap 2: tape and tallies together
    _row("step", 256, True, "shallow", 8, 1, SMALL, 5, 41, 1600, "aggressive", SINK),
    _row("step_info", 512, True, "shallow", 4, 3, 1000000, 6, 38, 1700),
    _row("run_random", 512, True, "shallow", 16, 1, SMALL, 7, 41, 1800, cfg=SINK),
    _row("rollout_tape", 256, True, "shallow", 4, 1, SMALL, 6, 41, 1900, cfg=SINK),
    _row("step", 512, True, "cold", 4, 1, 1000000, 6, 38, 2000, cfg=FIRM),
    _row("run_random", 256, True, "cold", 4, 3, 1000000, 5, 41, 2100, cfg=FIRM),
    # the rest of the pairs (gap 3: cap512, groups, 16 agents)
    _row("rollout_tape", 512, True, "spilled", 8, 3, SMALL, 6, 38, 2200, cfg=MILD),
    _row("rollout", 256, False, "shallow", 16, 1, SMALL, 6, 41, 2300, cfg=SINK),
    _row("step_info", 256, False, "cold", 16, 3, SMALL, 7, 38, 2400, "maker", MILD),
    _row("rollout_tape", 512, True, "cold", 16, 3, 1000000, 6, 41, 2500, cfg=FIRM),
    _row("rollout", 512, False, "spilled", 4, 1, 1000000, 6, 38, 2600),
    _row("rollout", 512, False, "cold", 8, 3, 1000000, 6, 41, 2700, cfg=FIRM),
    _row("step", 256, False, "spilled", 8, 1, 1000000, 5, 38, 2800),
    # once more where two cold instances meet: the tape's general build behind the info kernel, the tape's random-agent launch handing over, the policy kernel on a spilled book
    _row("step_info", 256, True, "spilled", 8, 1, 1000000, 5, 41, 2900),
    _row("run_random", 256, True, "spilled", 16, 3, 1000000, 6, 38, 3000),
    _row("rollout", 256, False, "spilled", 8, 1, 1000000, 6, 41, 3100),
]


def name_of(row):
    return "-".join([row["path"], f"t{row['tile']}", "tape" if row["tape"] else "notape", row["book"], f"A{row['agents']}", f"g{row['groups']}",
                     "small" if row["cash"] == SMALL else "rich"])


NAMES = [name_of(r) for r in ROWS]


def uncovered_pairs():
    """the pairs of factor levels no row holds (a rollout row cannot have the tape on, a rollout_tape row cannot have it off)"""
    import itertools
    missing = []
    for fa, fb in itertools.combinations(FACTORS, 2):
        for a in FACTORS[fa]:
            for b in FACTORS[fb]:
                if {fa: a, fb: b} in ({"path": "rollout", "tape": True}, {"path": "rollout_tape", "tape": False}):
                    continue
                if not any(r[fa] == a and r[fb] == b for r in ROWS):
                    missing.append((fa, a, fb, b))
    return missing


def n_steps(row):
    return 3 * row["max_step"] + 2


def horizon(row):
    """rollout rows: steps per run of the chains"""
    assert row["path"].startswith("rollout") and n_steps(row) % (row["max_step"] - 1) == 0
    return row["max_step"] - 1


def small(row):
    return row["cash"] == SMALL


def config_of(row):
    cfg = {"num_of_agents": row["agents"], "init_cash": row["cash"], "max_step": row["max_step"], "is_render": False, "book_capacity": row["tile"]}
    if row["path"] != "run_random":
        cfg["auto_reset"] = True
    cfg.update(row["cfg"])
    return cfg


def actions_of(row, stand_in=False):
    """the row's action stream, [n_steps] tuples of five [N, A] arrays (step / step_info rows; stand_in: what the host test plays in place of the device policy's
    samples of a rollout row - the GPU test checks the row's claims again on the actions the policy really took)"""
    assert stand_in or row["path"] in ("step", "step_info")
    rng = np.random.default_rng(row["seed"] + 7)
    N, A = row["N"], row["agents"]
    out = []
    for _ in range(n_steps(row)):
        cat = rng.integers(0, 9, (N, A)).astype(np.int32)
        if row["law"] == "aggressive":                        # half of the orders are market orders
            cat = np.where(rng.random((N, A)) < 0.5, rng.choice([1, 5], (N, A)), cat).astype(np.int32)
        elif row["law"] == "maker":                           # half of the orders are limit orders: the book does not thin out
            cat = np.where(rng.random((N, A)) < 0.5, rng.choice([2, 6], (N, A)), cat).astype(np.int32)
        out.append((cat, rng.uniform(-1, 1, (N, A)).astype(np.float32), rng.uniform(0, 1, (N, A)).astype(np.float32), rng.integers(0, 10, (N, A)).astype(np.int32),
                    rng.integers(0, 3, (N, A)).astype(np.int32)))
    return out


def action_seed(row, launch):
    """run_random rows: the random agents' seed of launch 0, 1, 2 (the sampler is keyed by the episode's step: another seed, another episode)"""
    return row["seed"] * 10 + launch


def prefill_sizes(row, market):
    """(n_bids, n_asks) the market starts its first episode with; None: an empty book"""
    if row["book"] == "shallow":
        return None
    tile, A = row["tile"], row["agents"]
    if row["path"] == "run_random" and market % 4 == 3:       # on the brink: hot now, cold with one more resting order
        return (tile - A) // 2, tile - A - (tile - A) // 2
    if row["book"] == "cold":
        return tile // 2, tile // 2
    return (300, 300) if tile == 256 else (500, 500)


def prefill(env, row):
    """the row's first books through the state dump, on the product or on the oracle (same get_state / set_state): equally seeded, the same book.  The escrow moves
    from cash to cash_on_hold: NAV is conserved, and no account is left without cash.  A rich account rests orders of up to 60 (a market order of at most ~100
    consumes a few of them: the book stays deep to the episode's end); a small one rests a few units per order in levels of 20 .. 40 orders."""
    from fuzz_cases import prefill_book
    from gym_continuousdoubleauction_amd import _capi as K
    for i in range(row["N"]):
        sizes = prefill_sizes(row, i)
        if sizes is None:
            continue
        if small(row):
            kw = {"qty": (1, 2) if row["book"] == "spilled" else (5, 8), "level_orders": (20, 41)}
        else:                                                 # (the escrow of an agent's share of the orders, at ~120 a unit, stays below a third of its cash)
            q = max(1, min(60, int(0.3 * row["cash"] * row["agents"] / (sum(sizes) * 120))))
            kw = {"qty": (max(1, 2 * q // 3), q + 1)}
        prefill_book(env, i, np.random.default_rng(row["seed"] + 1000 + i), row["agents"], *sizes, **kw)
        acc = env.get_state(i).acc
        assert all(K.dec_to_decimal(acc[a].cash) > 0 for a in range(row["agents"])), (name_of(row), i)
    if small(row):                                            # `terminated` needs EVERY agent in the sticky done set: no law gets 4 .. 16 accounts there within 5 .. 7 steps,
        for i in terminated_markets(row):                     # so two markets start with the set full - their first step ends the episode terminated (and out of step
            s = env.get_state(i)                              # with the batch from then on)
            s.done_mask = (1 << row["agents"]) - 1
            env.set_state(i, s)


def terminated_markets(row):
    return (1, row["N"] - 2) if small(row) else ()


def _replay(ora, em, acts_per_step):
    """the actions through the oracle with the env's auto-reset rule; feeds the host-side tallies"""
    for acts in acts_per_step:
        _, rew, term, trunc, info = ora.step(*acts)
        ended = em.feed(info, rew, term, trunc, done_mask_of=lambda i: ora.get_state(i).done_mask)
        if len(ended):
            ora.reset(mask=(term | trunc).astype(np.uint8))


class _Recording:
    """an OracleEnv whose step() / reset() also keep what the row's checks need (_replay drives it unchanged): per step every market's resting orders BEFORE the
    step, the step's outputs as the env hands them out (the observation of a market that ended is its new episode's first), fills and the done mask"""

    def __init__(self, ora):
        self._o, self.steps = ora, []

    def get_state(self, i):
        return self._o.get_state(i)

    def step(self, *acts):
        o = self._o
        orders = np.array([sum(o.book_size(i)) for i in range(o.n)], np.int64)
        obs, rew, term, trunc, info = o.step(*acts)
        ended = (term | trunc).astype(bool)
        done = np.zeros(o.n, np.uint32)
        for i in np.flatnonzero(ended):
            done[i] = o.get_state(int(i)).done_mask
        self.steps.append({"orders": orders, "obs": obs.copy(), "reward": rew.copy(), "terminated": term.astype(bool), "truncated": trunc.astype(bool), "ended": ended,
                           "fills": info["num_trades_step"].sum(1) > 0, "done_mask": done})
        return obs, rew, term, trunc, info

    def reset(self, mask=None):
        self.steps[-1]["obs"] = self._o.reset(mask=mask).copy()


class OracleRun:
    """the oracle side of a row: the CPU oracle seeded and prefilled like the env, the host-side tallies (episode_metrics_util.OracleEpisodeMetrics) and the record
    of every step.  play(actions): steps under the env's auto-reset rule; play_random(launch): one cda_run_random launch - every market to its own episode end -
    followed by the reset of all markets the row's driver issues."""

    def __init__(self, row):
        import oracle_lib as O
        from episode_metrics_util import OracleEpisodeMetrics
        self.row = row
        cfg = {k: v for k, v in config_of(row).items() if k != "auto_reset"}
        self.ora = O.OracleEnv(cfg, row["N"])
        self.ora.reset(seeds=(row["seed"] + np.arange(row["N"])).astype(np.uint64))
        prefill(self.ora, row)
        self.em = OracleEpisodeMetrics(row["N"], row["agents"], row["cash"])
        self.rec = _Recording(self.ora)

    @property
    def steps(self):
        return self.rec.steps

    def play(self, acts_per_step):
        _replay(self.rec, self.em, acts_per_step)

    def play_random(self, launch):
        import oracle_lib as O
        row, o, em = self.row, self.ora, self.em
        N, A = row["N"], row["agents"]
        alive = np.ones(N, bool)
        ret, steps = np.zeros((N, A)), np.zeros(N, np.int32)
        term_out, trunc_out = np.zeros(N, bool), np.zeros(N, bool)
        for t in range(row["max_step"]):
            if not alive.any():
                break
            orders = np.array([sum(o.book_size(i)) for i in range(N)], np.int64)
            for i in np.flatnonzero(alive):                   # a market that ended is not stepped again: its outputs stay those of its last step
                assert O.lib().oracle_run_random_range_info(o.h, int(i), 1, t, 1, action_seed(row, launch), 0, o.obs.ctypes.data, o.reward.ctypes.data,
                                                            o.term.ctypes.data, o.trunc.ctypes.data, o._info_ptrs) == 0
            dead = ~alive
            info = {k: v.copy() for k, v in o.info.items()}
            rew, term, trunc = o.reward.copy(), o.term.copy(), o.trunc.copy()
            for k in ("reward_terms", "is_pass_action", "num_rejected_step", "order_step_placed", "num_trades_step", "num_passive_fills_step"):
                info[k][dead] = 0
            rew[dead] = 0; term[dead] = 0; trunc[dead] = 0
            em.steps[dead] -= 1                               # (feed counts a step for every market)
            ended_idx = em.feed(info, rew, term, trunc, done_mask_of=lambda i: o.get_state(i).done_mask)
            ret[alive] += rew[alive]; steps[alive] += 1
            ended = np.zeros(N, bool); ended[ended_idx] = True
            term_out[ended], trunc_out[ended] = term[ended].astype(bool), trunc[ended].astype(bool)
            done = np.zeros(N, np.uint32)
            for i in ended_idx:
                done[i] = o.get_state(int(i)).done_mask
            self.rec.steps.append({"orders": orders, "alive": alive.copy(), "ended": ended, "terminated": term.astype(bool), "truncated": trunc.astype(bool),
                                   "fills": (info["num_trades_step"].sum(1) > 0) & alive, "done_mask": done})
            alive[ended_idx] = False
        assert not alive.any()
        out = {"obs": o.obs.copy(), "return": ret, "terminated": term_out, "truncated": trunc_out, "steps": steps, "flags": o.flags().copy(),
               "orders": np.array([sum(o.book_size(i)) for i in range(N)], np.int64),      # the books the launch leaves behind (nothing resets them inside it)
               "states": {i: bytes(o.get_state(i)) for i in ledger_markets(row)}}
        o.reset()
        return out

    def close(self):
        self.ora.close()


def ledger_markets(row):
    return sorted(set(range(0, row["N"], 4)) | {row["N"] - 1})


def claims(row, steps):
    """what the oracle's record of a row shows, counted: the figures both test files assert on"""
    tile, A, N = row["tile"], row["agents"], row["N"]
    seen = np.zeros(N, bool)                                  # the market's first episode is over
    first_end_cold, first_end_fill, ever_cold = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
    handed_mid = np.zeros(N, bool)                            # hot at the first episode's first step, cold at a later one
    hot_start = np.zeros(N, bool)
    episodes = terminated = last_fill = bankrupt = 0
    started = np.zeros(N, bool)
    for s in steps:
        act = s.get("alive", np.ones(N, bool))
        cold = (s["orders"] + A > tile) & act
        ever_cold |= cold
        first = ~seen & act
        hot_start |= first & ~started & ~cold
        handed_mid |= first & started & hot_start & cold
        started |= first
        e = s["ended"]
        first_end_cold |= e & ~seen & cold
        first_end_fill |= e & ~seen & s["fills"]
        last_fill += int((e & s["fills"]).sum())
        episodes += int(e.sum())
        terminated += int((e & s["terminated"] & (s["done_mask"] != 0)).sum())
        bankrupt += int((e & ~s["terminated"] & (s["done_mask"] != 0)).sum())
        seen |= e
    return {"episodes": episodes, "terminated": terminated, "truncated_with_bankrupt": bankrupt, "first_end_cold": int(first_end_cold.sum()), "ever_cold": int(ever_cold.sum()),
            "last_step_fills": last_fill, "first_end_cold_with_fill": int((first_end_cold & first_end_fill).sum()), "handed_mid": int(handed_mid.sum())}


def check_claims(row, c, violating):
    """the conditions on a row's inputs (tests/test_step_variants_host.py states them; the GPU test asserts them again on what it really played)"""
    N = row["N"]
    if row["book"] == "shallow":
        assert c["ever_cold"] == 0, (name_of(row), c)
    else:
        assert 4 * c["first_end_cold"] >= 3 * N, (name_of(row), c)
        assert c["first_end_cold_with_fill"] >= 1, (name_of(row), c)
        if row["path"] == "run_random":
            assert c["handed_mid"] >= 1, (name_of(row), c)
    assert c["episodes"] >= 2 * N, (name_of(row), c)
    if small(row):
        assert c["terminated"] >= 1, (name_of(row), c)
    assert c["last_step_fills"] >= 1, (name_of(row), c)
    assert not violating, (name_of(row), violating)


def oracle_run(row, actions=None):
    """the whole row on the oracle: (OracleRun, per-launch outputs of a run_random row | None).  actions: the stream to play (default: the row's own)"""
    run = OracleRun(row)
    if row["path"] == "run_random":
        return run, [run.play_random(k) for k in range(3)]
    run.play(actions_of(row, stand_in=row["path"].startswith("rollout")) if actions is None else actions)
    return run, None
