"""CPU: the border of the accepted config domain (csrc/cda_hip.hip cfg_ok + row_ok, restated in oracle/cda_oracle.c, tests/fuzz_cases.py row_in_domain and - through
the library - market_params.py).

  the bound table    every comparison of cfg_ok / row_ok at its bound and one beyond it: the same return code from the product library (cda_check_market_params
                     needs no device) and from the oracle, the same verdict from row_in_domain and from market_params.rows_of
  the edge cases     fuzz_cases.edge_cases() of the default seed - what tests/test_hip_config_edges.py plays on the device - cover every agent count and every
                     level of every factor, stay within the device's reach (fuzz_cases.in_reach) and trade
  the goldens        the reference's own traces at the border (tests/golden/trace_edge_*.npz; tests/test_oracle_golden.py and tests/test_hip_golden.py replay them)
                     are what make_goldens.py lists, and decode no price the device would clamp"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzz_cases as F      # noqa: E402
import config_edges_util as U      # noqa: E402
from gym_continuousdoubleauction_amd import _capi as K      # noqa: E402

BASE = {"num_of_agents": 4, "n_hist": 4, "max_step": 256, "is_render": False}
OK, INVALID, UNSUPPORTED = 0, K.ERR_INVALID, K.ERR_UNSUPPORTED
P24, S21, C62 = 1 << 24, 1 << 21, 1 << 62
SPILL_MAX = 1 << 20                                          # include/cda.h CDA_SPILL_MAX

# (fields set together, the return code).  Per-market fields are tried in the config and as a row of the BASE env; the others in the config only.
PER_MARKET = [
    ({"tick_size": 1}, OK), ({"tick_size": 65536}, OK), ({"tick_size": 0}, UNSUPPORTED), ({"tick_size": 65537}, UNSUPPORTED),
    ({"initial_price_min": 0, "initial_price_max": 0}, OK), ({"initial_price_min": -1, "initial_price_max": 0}, INVALID),
    ({"initial_price_min": 50, "initial_price_max": 50}, OK), ({"initial_price_min": 50, "initial_price_max": 49}, INVALID),
    ({"initial_price_min": P24 - 1, "initial_price_max": P24 - 1}, OK), ({"initial_price_max": P24 - 1}, OK), ({"initial_price_max": P24}, INVALID),
    ({"min_size": 1, "mkt_max_size": 1}, OK), ({"min_size": 0, "mkt_max_size": 5}, INVALID), ({"min_size": 0, "mkt_max_size": 0}, INVALID), ({"min_size": -1}, INVALID),
    ({"min_size": 7, "mkt_max_size": 7}, OK), ({"min_size": 7, "mkt_max_size": 6}, INVALID),
    ({"limit_size_multiple": 1}, OK), ({"limit_size_multiple": 0}, INVALID),
    ({"min_size": 1, "mkt_max_size": S21 - 1, "limit_size_multiple": 1}, OK), ({"min_size": 1, "mkt_max_size": S21, "limit_size_multiple": 1}, INVALID),
    ({"min_size": 1024, "mkt_max_size": 2047, "limit_size_multiple": 1024}, OK), ({"min_size": 1025, "mkt_max_size": 2047, "limit_size_multiple": 1024}, INVALID),
    ({"min_size": 1, "mkt_max_size": 1, "limit_size_multiple": S21 - 1}, OK), ({"min_size": 1, "mkt_max_size": 1, "limit_size_multiple": S21}, INVALID),
    ({"min_size": 1, "mkt_max_size": 1 << 16, "limit_size_multiple": 1 << 16}, INVALID),            # (the product leaves int32: the rule is evaluated in int64)
    ({"max_step": 1}, OK), ({"max_step": 0}, INVALID), ({"max_step": -1}, INVALID),
    ({"init_cash": C62}, OK), ({"init_cash": -C62}, OK), ({"init_cash": C62 + 1}, INVALID), ({"init_cash": -C62 - 1}, INVALID), ({"init_cash": 0}, OK),
]
CONFIG_ONLY = [
    ({"num_agents": 1}, OK), ({"num_agents": 16}, OK), ({"num_agents": 0}, INVALID), ({"num_agents": 17}, INVALID),
    ({"n_hist": 1}, OK), ({"n_hist": 16}, OK), ({"n_hist": 0}, INVALID), ({"n_hist": 17}, INVALID),
    ({"book_spill": -1}, OK), ({"book_spill": SPILL_MAX}, OK), ({"book_spill": -2}, INVALID), ({"book_spill": SPILL_MAX + 1}, INVALID),
    ({"book_capacity": 0}, OK), ({"book_capacity": 256}, OK), ({"book_capacity": 512}, OK), ({"book_capacity": 255}, INVALID), ({"book_capacity": 257}, INVALID),
    ({"book_capacity": 511}, INVALID), ({"book_capacity": 513}, INVALID), ({"book_capacity": -1}, INVALID),
    ({"auto_reset": 0}, OK), ({"auto_reset": 1}, OK), ({"auto_reset": 2}, INVALID), ({"auto_reset": -1}, INVALID),
]
ROW_ONLY = [
    ({"max_step": 256}, OK), ({"max_step": 257}, INVALID),                                           # a row's horizon: the env's at the most
    ({"reserved": 0}, OK), ({"reserved": 1}, INVALID), ({"reserved": -1}, INVALID),
]


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g
    g.build_hip()
    from gym_continuousdoubleauction_amd._lib import lib as L
    import oracle_lib as O
    return L(), O.lib()


def _both(libs, cfg, n, row):
    lib, ora = libs
    rowp = C.byref(row) if row is not None else None
    got = lib.cda_check_market_params(C.byref(cfg), n, rowp), ora.oracle_check_market_params(C.byref(cfg), n, rowp)
    assert got[0] == got[1], f"the product library says {got[0]}, the oracle {got[1]}"
    return got[0]


def _base_row(lib, cfg):
    r = K.MarketParams()
    assert lib.cda_market_params_from_config(C.byref(cfg), C.byref(r)) == 0
    return r


def test_the_base_of_the_table_is_accepted(libs):
    cfg, _ = K.make_config(BASE)
    assert _both(libs, cfg, 0, None) == OK and _both(libs, cfg, 1, _base_row(libs[0], cfg)) == OK
    assert F.row_in_domain(BASE, {"max_step": 256})


@pytest.mark.parametrize("fields,rc", PER_MARKET + CONFIG_ONLY, ids=lambda x: ",".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else str(x))
def test_bound_table_in_the_config(libs, fields, rc):
    cfg, _ = K.make_config(BASE)
    for k, v in fields.items():
        setattr(cfg, k, v)
    assert _both(libs, cfg, 0, None) == rc
    # the oracle's constructor applies the same rule (the product's needs a device)
    import oracle_lib as O
    h = C.c_void_p()
    assert O.lib().oracle_create(C.byref(cfg), 1, C.byref(h)) == rc
    if rc == OK:
        O.lib().oracle_destroy(h)


@pytest.mark.parametrize("fields,rc", PER_MARKET + ROW_ONLY, ids=lambda x: ",".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else str(x))
def test_bound_table_in_a_row(libs, fields, rc):
    from gym_continuousdoubleauction_amd.market_params import rows_of
    cfg, base = K.make_config(BASE)
    row = _base_row(libs[0], cfg)
    for k, v in fields.items():
        setattr(row, k, v)
    assert _both(libs, cfg, 1, row) == rc
    if "reserved" in fields:                                  # (no key of a config dict reaches it)
        return
    assert F.row_in_domain(BASE, dict({"max_step": 256}, **fields)) == (rc == OK)
    if rc == OK:
        rows_of(base, [fields])
    else:
        with pytest.raises(ValueError):
            rows_of(base, [fields])


def test_min_size_zero_is_refused_everywhere(libs):
    """a decoded size is rint(|sample|) + min_size: with min_size = 0 it can be 0, where the reference exits (process_order) - the domain starts at 1"""
    import oracle_lib as O
    from gym_continuousdoubleauction_amd.market_params import rows_of
    bad = dict(BASE, min_size=0, mkt_max_size=5)
    cfg, base = K.make_config(bad)
    assert _both(libs, cfg, 0, None) == INVALID
    with pytest.raises(RuntimeError):
        O.OracleEnv(bad, 1)
    with pytest.raises(ValueError):
        rows_of(K.make_config(BASE)[1], [{"min_size": 0}])
    assert not F.row_in_domain(BASE, {"max_step": 256, "min_size": 0})
    assert F.row_in_domain(BASE, {"max_step": 256, "min_size": 1})


# ---------------------------------------------------------------------------------------------------------------- the default seed's edge cases
@pytest.fixture(scope="module")
def cases():
    return F.edge_cases()


@pytest.fixture(scope="module")
def played(cases):
    return [U.play_on_oracle(c) for c in cases]


def test_the_default_cases_cover_every_agent_count_and_every_level(cases):
    assert len(cases) == F.EDGE_CASES == 32
    assert [c["cfg"]["num_of_agents"] for c in cases] == [1 + i % 16 for i in range(32)]
    held = {(f, v) for c in cases for f, v in c["edges"].items()}
    assert held == set(F.EDGE_LEADS) and len(F.EDGE_LEADS) == 23
    assert all(1 <= len(c["edges"]) <= 3 for c in cases)
    assert {c["tile"] for c in cases} == {256, 512}
    assert {c["cfg"]["book_capacity"] for c in cases if "book_capacity" in c["cfg"]} == {256, 512}
    assert [c["n_markets"] for c in cases] == [F.RAGGED_MARKETS if i == F.EDGE_RAGGED_CASE else F.EDGE_MARKETS for i in range(32)]
    assert all(c["steps"] == (3 * c["cfg"]["max_step"] + 2 if c["short"] else 48) for c in cases)
    for c in cases:                                            # the levels as the config spells them
        cfg, e = c["cfg"], c["edges"]
        scale = cfg.get("mkt_max_size", 100) * cfg.get("limit_size_multiple", 10) + cfg.get("min_size", 1)
        tick = cfg.get("tick_size", 1)
        assert ("scale" in e) == (scale == F.SCALE_MAX) and scale <= F.SCALE_MAX
        if "scale" in e:
            assert {"mkt": cfg["limit_size_multiple"] == 1, "mul1024": cfg["limit_size_multiple"] == 1024, "mul": cfg["mkt_max_size"] == 1}[e["scale"]]
        if "flat_size" in e:
            assert cfg["mkt_max_size"] == cfg["min_size"]
        if "price" in e:
            want = {"zero": (0, 0), "one": (1, 1), "tick": (tick, tick), "top": (1 << 23, F.PRICE_TOP)}[e["price"]]
            assert (cfg["initial_price_min"], cfg["initial_price_max"]) == want
        for f in ("init_cash", "tick_size", "max_step", "n_hist", "book_capacity"):
            if f in e:
                assert cfg[f] == e[f]
        # cash follows sizes and prices
        if scale == F.SCALE_MAX or tick >= 65535 or e.get("price") == "top":
            assert cfg["init_cash"] == F.CASH_MAX
        assert F.row_in_domain(cfg, {})
        K.make_config(cfg)
        F.granted_ring(cfg)                                    # (raises on a ring the env would refuse)
    # at the largest scale the automatic ring is cut to 512 (tile 256) or 256 (tile 512) slots by the int32 rule
    rings = {(c["tile"], F.granted_ring(c["cfg"])) for c in cases if "scale" in c["edges"]}
    assert rings == {(256, 512), (512, 256)}


# the configuration fuzz's first two draws of its default seed (tests/test_hip_vs_oracle_batch.py, CDA_FUZZ_SEED 31337): literals taken at the commit before edge_case came
FUZZ_FIRST = ({"num_of_agents": 8, "init_cash": 50000, "max_step": 4096, "is_render": False, "n_hist": 1, "initial_price_min": 20000, "initial_price_max": 20103,
               "min_size": 3, "mkt_max_size": 100, "limit_size_multiple": 3, "order_penalty": 0.4313841222686283, "trade_penalty": 0.50207334256556,
               "drawdown_penalty": 0.0703451230577341, "passive_bonus": 0.5860405927004654, "loss_multiplier": 2.592681261502405}, "uniform", 0.4812131311466695)
FUZZ_SECOND = ({"num_of_agents": 3, "init_cash": 1000000, "max_step": 4096, "is_render": False, "n_hist": 2, "initial_price_min": 1, "initial_price_max": 239,
                "tick_size": 5}, "aggressive", 0.3762451283778607)


def test_the_edge_generator_leaves_the_other_streams_alone(cases):
    """random_config and random_order draw what they drew (the configuration fuzz's first cases against literals; tests/test_services_fuzz_host.py holds the service
    cases to theirs), and an edge case is a function of (seed, index)"""
    rng = np.random.default_rng(31337)
    assert F.random_config(rng) == FUZZ_FIRST and F.random_order(rng) is None and F.random_config(rng) == FUZZ_SECOND
    again = F.edge_cases(count=5)
    for a, b in zip(again, cases):
        assert a["cfg"] == b["cfg"] and a["seed"] == b["seed"] and np.array_equal(a["seeds"], b["seeds"]) and a["edges"] == b["edges"]
    assert F.edge_cases(F.EDGE_SEED + 1, 3)[0]["seed"] != cases[0]["seed"]
    for seed in (1, 2, 3):                                     # one to three factors at an edge, whatever the seed
        assert all(1 <= len(c["edges"]) <= 3 for c in F.edge_cases(seed))


def test_the_start_price_restatement_is_the_oracles(cases):
    """_edge_seeds keeps, under a price band that ends at 2^24 - 1, seeds whose market starts with headroom: its numpy restatement of reset's first draw against the oracle"""
    import oracle_lib as O
    top = [c for c in cases if c["edges"].get("price") == "top"]
    assert top
    for c in top + cases[:4]:
        cfg = c["cfg"]
        ora = O.OracleEnv(c["oracle_cfg"], c["n_markets"])
        ora.reset(c["seeds"])
        lo, hi = cfg.get("initial_price_min", 10), cfg.get("initial_price_max", 100)
        for m in range(c["n_markets"]):
            start = int(np.random.default_rng(int(c["seeds"][m])).integers(lo, hi, endpoint=True))
            assert ora.get_state(m).last_price == start
            if c in top:
                assert start <= F.PRICE_TOP - F.HEADROOM_TICKS * cfg.get("tick_size", 1)
        ora.close()


def test_every_default_case_is_within_the_devices_reach(cases, played):
    for i, (c, (why, _fills, _term, _steps)) in enumerate(zip(cases, played)):
        assert why is None, U.generator_message(i, c, why)


def test_the_edges_trade_and_the_broke_terminate(cases, played):
    traded = set()
    for c, (_why, fills, term, steps) in zip(cases, played):
        if c["broke"]:                                         # init_cash <= 0: every agent is bankrupt at the first mark, every step ends the episode
            assert term == steps and fills == 0, c["edges"]
        elif fills > 0:
            traded |= set(c["edges"].items())
    assert any(c["broke"] and c["short"] for c in cases) and sum(c["broke"] for c in cases) >= 4
    # every level of every factor is held by a case that trades - except init_cash <= 0.  (init_cash = 1 trades in the case fuzz_cases.EDGE_ALSO builds for it:
    # an order is approved when cash >= price x opening size, so 1 of cash buys one unit at a price of 1 and nothing else)
    for level in F.EDGE_LEADS:
        if level[0] == "init_cash" and level[1] <= 0:
            continue
        assert level in traded, level


def test_in_reach_tells_what_is_out_of_reach():
    """in_reach on cases built to be out: a market that starts at 2^24 - 1 decodes asks beyond it; a book that outgrows tile + ring"""
    import oracle_lib as O
    rng = np.random.default_rng(5)
    case = F.edge_case(rng, 4, ("price", "top"))
    case["cfg"].update(initial_price_min=F.PRICE_TOP, initial_price_max=F.PRICE_TOP)
    case["oracle_cfg"] = dict(case["cfg"])
    why, *_ = U.play_on_oracle(case)
    assert why is not None and "2^24" in why
    assert "fix the generator" in U.generator_message(0, case, why)
    case = F.edge_case(rng, 16, ("n_hist", 1))
    case["cfg"].update(book_capacity=256, book_spill=-1)
    case["oracle_cfg"] = dict(case["cfg"])
    case["tile"] = 256
    ora = O.OracleEnv(dict(case["oracle_cfg"], book_spill=0), 1)          # (an unbounded oracle book, as under an HBM ring)
    ora.reset(case["seeds"][:1])
    F.prefill_book(ora, 0, np.random.default_rng(1), 16, 300, 10)
    why = F.in_reach(dict(case, n_markets=1), ora)
    assert why is not None and "300 bids" in why
    ora.close()


# ---------------------------------------------------------------------------------------------------------------- the reference at the border
EDGE_TRACES = ["edge_A13_s403", "edge_A16_allmax_s410", "edge_A1_s401", "edge_A7_s402", "edge_cash0_s404", "edge_cashmax_s406", "edge_cashneg_s405", "edge_hist16_s412",
               "edge_price0_s407", "edge_pricetop_tickmax_s408", "edge_scalemax_s409", "edge_step1_s411", "edge_tickmax_floor_s413"]


def test_the_edge_goldens_are_there_and_within_the_devices_reach():
    import golden_util as G
    assert sorted(n for n in G.trace_names() if n.startswith("edge_")) == EDGE_TRACES
    seen = {}
    for name in EDGE_TRACES:
        rec = G.load(name)
        cfg = rec["config"]
        assert rec["cat"].shape[0] <= 48 and os.path.getsize(os.path.join(G.GOLD, f"trace_{name}.npz")) <= os.path.getsize(os.path.join(G.GOLD, "trace_A16_s70.npz"))
        assert int(rec["dec_price"].max()) < P24, name         # beyond, the device clamps and flags: such a trace would not replay bit for bit
        assert F.row_in_domain(cfg, {})
        seen[name] = (cfg, rec)
    assert {seen[n][0]["num_of_agents"] for n in EDGE_TRACES} >= {1, 7, 13, 16}
    assert {seen[n][0]["init_cash"] for n in EDGE_TRACES} >= {0, -1, C62}
    for n in ("edge_cash0_s404", "edge_cashneg_s405"):         # bankrupt at the first mark: terminated on every step, nothing trades
        assert seen[n][1]["term"].all() and seen[n][1]["tape_len"][-1] == 0
    for n in ("edge_A1_s401", "edge_cashmax_s406", "edge_price0_s407", "edge_pricetop_tickmax_s408", "edge_scalemax_s409", "edge_A16_allmax_s410", "edge_hist16_s412",
              "edge_tickmax_floor_s413"):
        assert seen[n][1]["tape_len"][-1] > 0, n               # the edges trade
    cfg = seen["edge_pricetop_tickmax_s408"][0]
    assert cfg["tick_size"] == 65536 and cfg["initial_price_max"] == P24 - 1 and int(seen["edge_pricetop_tickmax_s408"][1]["dec_price"].max()) > 1 << 23
    cfg, rec = seen["edge_A16_allmax_s410"]
    assert cfg["mkt_max_size"] * cfg["limit_size_multiple"] + cfg["min_size"] == S21 and cfg["initial_price_max"] == P24 - 1 and int(rec["dec_size"].max()) > 1 << 15
    assert int(seen["edge_scalemax_s409"][1]["dec_size"].max()) > 1 << 19          # (the largest decodable size is about half the scale)
    rec = seen["edge_tickmax_floor_s413"][1]                    # the floor clamp (a decoded price below one tick becomes one tick) is in play
    assert int(rec["dec_price"][rec["dec_type"] > 0].min()) == 65536 and int(rec["market"][:, 0].min()) <= 65536
    cfg, rec = seen["edge_step1_s411"]
    assert cfg["max_step"] == 1 and rec["trunc"].all() and len(rec["resets"]) == rec["cat"].shape[0] - 1
    assert seen["edge_hist16_s412"][0]["n_hist"] == 16
