"""CPU: the generator of the services fuzz (tests/fuzz_cases.py service_case) on its own - no device, no oracle.  The default seed's cases must cover what
tests/test_hip_services_fuzz.py relies on, every drawn per-market row must pass the library's own check and every scripted profile the host's, and the generator
must leave random_config's stream (which tests/golden/crosscheck_oracle.py and the two older fuzz tests replay) exactly as it was."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzz_cases as F      # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return F.service_cases()


def _ticks(case):
    return [case["cfg"].get("tick_size", 1)] + [r["tick_size"] for r in case["rows"] or []]


def test_the_default_cases_cover_what_the_gpu_test_relies_on(cases):
    assert len(cases) == F.SERVICE_CASES == 12
    agents = [c["cfg"]["num_of_agents"] for c in cases]
    assert any(a % 2 for a in agents) and 16 in agents
    assert any(c["cfg"]["n_hist"] > 8 for c in cases) and any(c["cfg"]["n_hist"] == 16 for c in cases)
    assert any(c["tile"] == 512 for c in cases) and any(c["tile"] == 256 for c in cases)
    assert any(c["small_ring"] and c["cfg"]["book_spill"] in (64, 128) for c in cases)
    assert any(t != 1 for c in cases for t in _ticks(c))
    assert any(c["rows"] for c in cases) and any(c["short"] for c in cases) and any(c["short"] and c["rows"] for c in cases)
    assert {int(x) for c in cases for x in c["stream_lengths"]} == set(F.STREAM_LENGTHS)
    # a prefilled case whose books can outgrow the tile (the GPU test asserts from the ring counts that one does), and one on a small ring
    assert any(c["prefill"] and not c["small_ring"] for c in cases) and any(c["prefill"] and c["small_ring"] for c in cases)
    assert [c["n_markets"] for c in cases] == [F.RAGGED_MARKETS if i == F.RAGGED_CASE else F.SERVICE_MARKETS for i in range(len(cases))]
    assert F.RAGGED_MARKETS % 4 == 2 and F.SERVICE_MARKETS % 4 == 0


def test_every_leg_can_run_on_every_default_case(cases):
    """what the GPU test's tally (every leg on at least 10 of the 12 cases) needs from the inputs: messages to stream, scripted slots, a fork that fits"""
    for i, c in enumerate(cases):
        n, a = c["n_markets"], c["cfg"]["num_of_agents"]
        assert c["slots"].shape == (n, a) and (c["slots"] != 0).any() and (c["slots"] == 0).any(), i
        assert 3 <= len(c["profiles"]) <= 6 and c["slots"].max() <= len(c["profiles"]) and len({p.law for p in c["profiles"]}) >= 3, i
        assert len(c["stream_lengths"]) == n and (c["stream_lengths"] > 0).sum() >= 2, i
        assert len(set(c["invalid_markets"])) == 2 and all(0 <= m < n for m in c["invalid_markets"]), i
        f = c["fork"]
        assert f["n_markets"] != n and f["first"] + f["n"] <= f["n_markets"] and f["src_first"] + f["n"] <= n and f["n"] >= 1, i
        assert 1 <= c["levels"] <= 40 and 1 <= len(c["impact_sizes"]) <= 4 and 1 <= len(c["horizons"]) <= 4 and c["bar_steps"] >= 1 and c["n_bars"] >= 1, i
        if c["short"]:
            assert c["cfg"]["auto_reset"] and c["cfg"]["max_step"] < F.SERVICE_STEPS // 2, i                # at least two episode ends inside the first leg
        else:
            horizon = min([c["cfg"]["max_step"]] + [r["max_step"] for r in c["rows"] or []])
            assert horizon > F.SERVICE_STEPS + F.SERVICE_STEPS_AFTER and "auto_reset" not in c["cfg"], i
        if c["small_ring"]:
            assert c["law"] != "trend", i
        for m in range(0, n, 3):
            nb, na = F.service_prefill_sizes(c, m)
            assert 0 <= nb <= 512 and 0 <= na <= 512, (i, m)
            if c["small_ring"]:                              # within tile + ring with room to grow, and - both sides at their largest - beyond the tile
                assert nb + na <= c["tile"] + c["cfg"]["book_spill"] // 2, (i, m)


def test_every_row_passes_the_library_check_and_every_profile_the_hosts(cases):
    import __graft_entry__ as g
    g.build_hip()
    from gym_continuousdoubleauction_amd import _capi as K
    from gym_continuousdoubleauction_amd.market_params import market_config, row_of, rows_of, validate_rows
    from gym_continuousdoubleauction_amd.scripted import profiles_array
    more = F.service_cases(seed=F.SERVICE_SEED + 1, count=40)                   # ... beyond the default seed too
    n_rows = 0
    for i, c in enumerate(list(cases) + more):
        base = K.make_config(c["cfg"])[1]
        K.make_config(c["oracle_cfg"])
        for row in c["rows"] or []:
            assert F.row_in_domain(c["cfg"], row) and F.row_fits_ring(c["cfg"], row), (i, row)
            rows = (K.MarketParams * 1)(row_of(market_config(base, row)))
            validate_rows(base, rows)                                           # raises ValueError on a refused row
            n_rows += 1
        if c["rows"]:
            assert len(c["rows"]) in (2, 3) and all(c["rows"][x] != c["rows"][y] for x in range(len(c["rows"])) for y in range(x)), i
            rows_of(base, [c["rows"][m % len(c["rows"])] for m in range(c["n_markets"])])
        for p in c["profiles"]:
            assert p.problems() == [], (i, p)
        assert len(profiles_array(c["profiles"])) == len(c["profiles"])
    assert n_rows > 20
    # the generator's own statement of the rule refuses what the library refuses
    cfg = cases[0]["cfg"]
    for bad in ({"tick_size": 0}, {"initial_price_min": 50, "initial_price_max": 10}, {"max_step": cfg["max_step"] + 1}, {"mkt_max_size": 300000, "limit_size_multiple": 10},
                {"min_size": -1}, {"min_size": 0}, {"initial_price_max": 1 << 24}):
        row = dict({"max_step": cfg["max_step"]}, **bad)
        assert not F.row_in_domain(cfg, row), bad
        with pytest.raises(ValueError):
            rows_of(K.make_config(cfg)[1], [row])


# ---- the twelve default cases are what they were before service_extras came: their seed fields and shapes, literals taken from the commit before it ----
DEFAULT_SEEDS = [649081748879560493, 2698841326163019393, 2505966728131038087, 789277998334646751, 2575916902629827419, 2024318441497068961,
                 2047527317627600816, 6912268489781382, 4059451142223408395, 1124075379147082851, 1955962979324153592, 1152983785470081220]
# (num_of_agents, n_hist, tile, short, bool(rows))
DEFAULT_SHAPES = [(2, 9, 512, False, True), (16, 16, 512, False, False), (2, 8, 256, False, False), (8, 4, 512, False, True), (12, 1, 256, False, False),
                  (4, 9, 256, False, False), (4, 8, 256, False, True), (8, 5, 512, False, False), (5, 4, 256, False, True), (5, 9, 256, True, True),
                  (8, 3, 256, False, False), (5, 5, 512, False, True)]


def test_service_extras_left_the_default_cases_alone(cases):
    assert [c["seed"] for c in cases] == DEFAULT_SEEDS
    assert [(c["cfg"]["num_of_agents"], c["cfg"]["n_hist"], c["tile"], c["short"], bool(c["rows"])) for c in cases] == DEFAULT_SHAPES
    # drawing the extras draws nothing from the cases' stream: the cases drawn with the extras taken in between are the same cases
    rng = np.random.default_rng(F.SERVICE_SEED)
    for i, c in enumerate(cases):
        again = F.service_case(rng, F.RAGGED_MARKETS if i == F.RAGGED_CASE else F.SERVICE_MARKETS)
        F.service_extras(again)
        assert again["seed"] == c["seed"] and again["cfg"] == c["cfg"] and again["fork"] == c["fork"] and np.array_equal(again["slots"], c["slots"]), i
    a, b = F.service_extras(cases[3]), F.service_extras(cases[3])                # ... and the extras are a function of the case
    assert a["lengths"] == b["lengths"] and np.array_equal(a["schedule"]["market_schedule"], b["schedule"]["market_schedule"]) and a["invalid"] == b["invalid"]


def test_the_extras_of_the_default_cases_cover_what_the_new_legs_rely_on(cases):
    import schedule_util as U
    assert set(F.SCHEDULE_EDGES) == set(U.EDGE_LENGTHS) - {0, 1} and F.INVALID_KINDS == len(F.invalid_messages(4))
    extras = [F.service_extras(c) for c in cases]
    caps = [x["quote_capacity"] for x in extras]
    assert any(k & (k - 1) for k in caps)                      # a capacity that is no power of two
    for c, x in zip(cases, extras):                            # short auto-reset episodes get a small ring that is no power of two: it wraps across the resets
        if c["short"]:
            k, h_max = x["quote_capacity"], max([r["max_step"] for r in c["rows"] or []] + ([] if c["rows"] else [c["cfg"]["max_step"]]))
            assert k & (k - 1) and h_max < k <= h_max + max(1, h_max // 2), (k, h_max)      # an episode of the longest horizon fits, one and a half do not: a previous episode loses its head
        else:
            assert x["quote_capacity"] in F.QUOTE_CAPACITIES
    for c in F.service_cases(F.SERVICE_SEED + 2, 60):          # ... at every horizon the generator can draw
        if c["short"]:
            k, h_max = F.service_extras(c)["quote_capacity"], max([r["max_step"] for r in c["rows"] or []] + ([] if c["rows"] else [c["cfg"]["max_step"]]))
            assert k & (k - 1) and h_max < k <= h_max + max(1, h_max // 2), (k, h_max)
    assert any(c["short"] and c["rows"] for c in cases)
    assert any(x["quote_capacity"] < 40 and not c["short"] for c, x in zip(cases, extras))          # ... and one that wraps inside the 56 steps of a long case
    assert {x["schedule"]["loop"] for x in extras} == {True, False} and {x["schedule"]["clear_step_counters"] for x in extras} == {True, False}
    seen = set()
    for i, (c, x) in enumerate(zip(cases, extras)):
        sc, n = x["schedule"], c["n_markets"]
        ms, S, lengths = sc["market_schedule"], sc["n_windows"], np.array(x["lengths"])
        assert 1 <= sc["n_rows"] <= 3 and lengths.shape == (sc["n_rows"], S) and ms.shape == (n,) and ms.min() == -1 and ms.max() == sc["n_rows"] - 1, i
        assert all((ms == r).sum() >= 2 for r in range(sc["n_rows"])), i                            # every row is played, and shared
        # THE WINDOW RULE (fuzz_cases.schedule_reach): messages lie in windows the leg reaches, and nowhere else
        reach = F.schedule_reach(c, S, sc["loop"])
        assert x["reach"] == reach and len(reach) >= 3, i
        if c["short"]:
            h_min = min([c["cfg"]["max_step"]] + [r["max_step"] for r in c["rows"] or []])
            assert h_min < F.SERVICE_STEPS_AFTER and reach == list(range(min(S, h_min))), i        # every market passes every t_step of its episode inside the leg
        else:
            steps = range(F.SERVICE_STEPS, F.SERVICE_STEPS + F.SERVICE_STEPS_AFTER)
            assert reach == sorted({t % S for t in steps} if sc["loop"] else {t for t in steps if t < S}), i
        for r in range(sc["n_rows"]):
            on = np.flatnonzero(lengths[r])
            assert len(on) >= 2 and set(on.tolist()) <= set(reach), (i, r)
            assert len(on) <= max(2, S // 2), (i, r)                                               # sparse flow
        assert lengths.max() <= F.SCHEDULE_WINDOW_MAX and (not c["small_ring"] or lengths.max() <= 4 + F.INVALID_KINDS), i
        bad = x["invalid"]
        assert lengths[bad["row"], bad["window"]] >= F.INVALID_KINDS and ms[bad["market"]] == bad["row"] and len(bad["positions"]) == F.INVALID_KINDS, i
        assert max(bad["positions"]) <= lengths[bad["row"], bad["window"]] - F.INVALID_KINDS, i
        seen |= {int(v) for v in lengths.reshape(-1)}
    assert set(F.SCHEDULE_EDGES) <= seen, seen


@pytest.fixture(scope="module")
def dry(cases):
    """the oracle-only dry run of the default cases (tests/services_fuzz_util.py dry_run), once for the module"""
    import services_fuzz_util as SU
    return [(i, c, x, SU.dry_run(c, x)) for i, c in enumerate(cases) for x in [F.service_extras(c)]]


def test_an_oracle_only_dry_run_shows_the_conditions_the_gpu_comparison_relies_on(dry):
    """Steps, stream and schedule of every default case on the oracles alone, no device: conditions on the INPUTS, which on the GPU would hide behind a flag
    mismatch.  (1) on a small ring the book stays inside tile + ring - both sides together, the oracle's own census, inside steps too: then neither side can -
    through the whole case, scheduled flow included; (2) no tape can drop a record: the bound behind TAPE_CAPACITY, from the messages each market really got;
    (3) every case plays at least two non-empty windows - and the drawn lengths are all reached, scheduled fills and rejections occur.  Measured: 3 to 5 s for the
    twelve cases together (0.12 to 1.7 s each) on a built tree, so all twelve are kept.  (4) the play past the row's horizon has markets to move in some case."""
    import services_fuzz_util as SU
    fills = rejected = 0
    reached = set()
    for i, c, x, d in dry:
        assert not d["flags"].any(), i
        if c["small_ring"]:
            assert d["peak_total"] <= c["tile"] + c["cfg"]["book_spill"] and d["peak_side"] <= d["peak_total"], (i, d["peak_total"], d["peak_side"])
        assert d["tape_bound"] < SU.TAPE_CAPACITY, (i, d["tape_bound"])
        windows = {(r, w) for _, r, w, _ in d["played"]}
        drawn = {(r, w) for r, row in enumerate(x["lengths"]) for w, k in enumerate(row) if k}
        assert len(windows) >= 2 and windows == drawn, (i, sorted(drawn - windows))                 # every drawn window is played somewhere
        assert all(k == x["lengths"][r][w] for _, r, w, k in d["played"]), i
        per_market = np.zeros(c["n_markets"], np.int64)
        for m, _, _, k in d["played"]:
            per_market[m] += k
        assert per_market.max() <= SU.SCHEDULE_PLAYS * F.SCHEDULE_WINDOW_MAX, i                     # the term of the TAPE_CAPACITY bound
        for m, t in d["past_horizon"].items():                 # over by the market's own row, live by the config, and a window with messages under that clock
            sc, hz = x["schedule"], SU.horizons(c)
            assert sc["loop"] and hz[m] <= t < c["cfg"]["max_step"] and x["lengths"][sc["market_schedule"][m]][t % sc["n_windows"]] > 0, (i, m, t)
        assert (d["counts"][x["schedule"]["market_schedule"] < 0] == 0).all(), i
        bad = x["invalid"]
        assert d["counts"][bad["market"], 2] >= F.INVALID_KINDS and d["counts"][:, 2].sum() % F.INVALID_KINDS == 0, i
        fills += d["trades"]
        rejected += int(d["counts"][:, 1].sum())
        reached |= {k for *_, k in d["played"]}
    assert fills > 0 and rejected > 0
    assert set(F.SCHEDULE_EDGES) <= reached, reached
    assert all(d["trades"] > 0 for *_, d in dry)                                                    # scheduled fills in every case
    assert sum(len(d["past_horizon"]) >= 2 for *_, d in dry) >= 2                                   # cases whose schedule meets markets past their own row's horizon


def test_a_row_keeps_to_the_ring_the_env_was_cut_for():
    """cda_set_market_params refuses a row whose largest order size times tile + ring leaves int32 - the ring is cut for the config's sizes at construction.  A soak
    found it: CDA_FUZZ_SEED=90417, case 110 was refused by the env.  The generator now redraws such a row; the stream of that seed draws no such row any more."""
    cfg = {"num_of_agents": 16, "init_cash": 1000000, "max_step": 4096, "is_render": False, "n_hist": 12, "book_capacity": 512}
    assert F.granted_ring(cfg) == 65536 and F.granted_ring(dict(cfg, book_spill=100)) == 128 and F.granted_ring(dict(cfg, book_spill=-1)) == 0
    assert F.granted_ring(dict(cfg, mkt_max_size=3000, limit_size_multiple=20, min_size=3)) == 32768      # 60003 x (512 + 65536) > 2^31 - 1: halved once
    row = {"tick_size": 1, "initial_price_min": 20000, "initial_price_max": 20021, "min_size": 3, "mkt_max_size": 3000, "limit_size_multiple": 20, "max_step": 4096}
    assert F.row_in_domain(cfg, row) and not F.row_fits_ring(cfg, row)
    assert F.row_fits_ring(cfg, dict(row, mkt_max_size=100)) and F.row_fits_ring(dict(cfg, max_step=1024), row) and F.row_fits_ring(dict(cfg, book_spill=-1), row)
    for c in F.service_cases(90417, 120):
        assert all(F.row_fits_ring(c["cfg"], r) for r in c["rows"] or []), c["cfg"]


PINNED = (8, 50000, 1, "uniform")


def test_random_config_draws_what_it_drew_before():
    """service_case starts with random_config's draws and adds its own behind them: the older fuzz tests' and the cross-check's cases stay what they are"""
    a, b = np.random.default_rng(31337), np.random.default_rng(31337)
    cfg, law, present_p = F.random_config(a)
    case = F.service_case(b)
    for k, v in cfg.items():
        if k not in ("n_hist", "max_step"):
            assert case["cfg"][k] == v, k
    assert (case["law"], case["present_p"]) == (law, present_p)
    # the first configuration of the older fuzz test's default seed, pinned
    assert (cfg["num_of_agents"], cfg["init_cash"], cfg["n_hist"], law) == PINNED

