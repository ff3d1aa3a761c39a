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
            assert F.row_in_domain(c["cfg"], row), (i, row)
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
                {"min_size": -1}, {"initial_price_max": 1 << 24}):
        row = dict({"max_step": cfg["max_step"]}, **bad)
        assert not F.row_in_domain(cfg, row), bad
        with pytest.raises(ValueError):
            rows_of(K.make_config(cfg)[1], [row])


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

