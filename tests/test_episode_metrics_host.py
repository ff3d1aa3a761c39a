"""CPU: the host half of the episode metrics - the reference callback's reductions (train/callbk/league_based_self_play_callback.py:295-470) from the accumulator
tables, the driver's strict_nav_check rule (train/train.py:1109-1164) and the test helper that restates the callback's tallies (tests/episode_metrics_util.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gym_continuousdoubleauction_amd import _capi as K
from gym_continuousdoubleauction_amd import episode_metrics as EM


def _table():
    t = np.zeros((3, K.EM_AGENT_FIELDS))
    # module 0: two (episode, agent) pairs of 10 steps each
    t[0, K.EM_EPISODES], t[0, K.EM_AGENT_STEPS], t[0, K.EM_PASSES], t[0, K.EM_REJECTIONS], t[0, K.EM_PLACED] = 2, 20, 5, 2, 9
    t[0, K.EM_TERM_SUM:K.EM_TERM_SUM + 5] = [10.0, -2.0, -1.0, 0.0, 0.5]
    t[0, K.EM_TERM_SQ:K.EM_TERM_SQ + 5] = [25.0, 0.4, 0.1, 0.0, 0.05]
    t[0, K.EM_RETURN_SUM], t[0, K.EM_RETURN_SQ] = 7.5, 40.0
    t[0, K.EM_NAV_SUM], t[0, K.EM_NAV_MIN], t[0, K.EM_NAV_MAX] = 2000010.0, 999990.0, 1000020.0
    t[0, K.EM_DRAWDOWN_SUM], t[0, K.EM_ABS_POSITION_SUM], t[0, K.EM_NUM_TRADES_SUM] = 30.0, 8, 14
    t[0, K.EM_MAKER_RATIO_SUM], t[0, K.EM_MAKER_RATIO_N], t[0, K.EM_MAKER_RATIO_MAX] = 0.75, 1, 0.75
    # module 2 played one pair; module 1 nothing
    t[2, K.EM_EPISODES], t[2, K.EM_AGENT_STEPS], t[2, K.EM_PASSES] = 1, 10, 10
    t[2, K.EM_NAV_SUM], t[2, K.EM_NAV_MIN], t[2, K.EM_NAV_MAX] = 1000000.0, 1000000.0, 1000000.0
    e = np.zeros(K.EM_ENV_FIELDS)
    e[K.EM_ENV_EPISODES], e[K.EM_ENV_STEPS], e[K.EM_ENV_MAKER_MAX_SUM], e[K.EM_ENV_MAKER_MAX_N], e[K.EM_ENV_TERMINATED] = 1, 10, 0.75, 1, 0
    return t, e


def test_summarise_gives_the_callbacks_metrics():
    t, e = _table()
    s = EM.summarise(t, e, module_names=["policy_0", "policy_1", "champion_1"])
    assert s["episodes"] == 1 and s["nav_conservation_violations"] == 0 and s["episode_len_mean"] == 10 and s["maker_fill_ratio_max"] == 0.75
    assert set(s["modules"]) == {"policy_0", "champion_1"}                     # a module that played nothing reports nothing
    m = s["modules"]["policy_0"]
    assert m["pass_action_fraction"] == 5 / 20 and m["order_rejection_fraction"] == 2 / 20
    assert m["reward_term_mean_nav"] == 0.5 and m["reward_term_mean_order"] == -0.1
    var = {"nav": 25 / 20 - 0.25, "order": 0.4 / 20 - 0.01, "trade": 0.1 / 20 - 0.0025, "drawdown": 0.0, "passive": 0.05 / 20 - 0.025 ** 2}
    tot = sum(var.values())
    for k, v in var.items():
        assert m[f"reward_term_var_share_{k}"] == pytest.approx(v / tot, rel=1e-12)
    assert sum(m[f"reward_term_var_share_{k}"] for k in var) == pytest.approx(1.0)
    assert m["episode_nav_mean"] == 1000005.0 and m["episode_nav_min"] == 999990.0 and m["episode_nav_max"] == 1000020.0
    assert m["mean_agent_drawdown"] == 15.0 and m["mean_abs_net_position"] == 4 and m["mean_num_trades"] == 7 and m["maker_fill_ratio_mean"] == 0.75
    assert m["episode_return_mean"] == 3.75 and m["episode_return_std"] == pytest.approx((20.0 - 3.75 ** 2) ** 0.5)
    a = s["all"]                                                               # every agent of every episode: the callback's own (module-blind) figures
    assert a["agent_episodes"] == 3 and a["pass_action_fraction"] == 15 / 30 and a["episode_nav_min"] == 999990.0 and a["episode_nav_max"] == 1000020.0
    c = s["modules"]["champion_1"]
    assert c["pass_action_fraction"] == 1.0 and "reward_term_var_share_nav" not in c and "maker_fill_ratio_mean" not in c      # no variance to split, no qualifying agent


def test_strict_nav_check_stops_the_run_and_the_lenient_one_logs():
    t, e = _table()
    EM.check_nav_conservation(3, EM.summarise(t, e))                           # conserved: nothing happens
    e[K.EM_ENV_NAV_VIOLATIONS], e[K.EM_ENV_NAV_ERROR_MAX], e[K.EM_ENV_NAV_ERROR_SUM] = 2, 12.5, 13.0
    s = EM.summarise(t, e)
    assert s["nav_conservation_violations"] == 2 and s["nav_conservation_error"] == 12.5
    with pytest.raises(EM.NavConservationError, match="2 episode"):
        EM.check_nav_conservation(3, s, strict=True)
    assert issubclass(EM.NavConservationError, AssertionError)                 # what the reference raises (train.py:1100-1107)
    seen = []
    EM.check_nav_conservation(3, s, strict=False, log=seen.append)
    assert len(seen) == 1 and "iteration 3" in seen[0]


def test_the_helper_restates_the_callbacks_tallies():
    """tests/episode_metrics_util.py against a by-hand episode: two steps, two agents, the episode ends at the second"""
    from decimal import Decimal
    from episode_metrics_util import OracleEpisodeMetrics
    em = OracleEpisodeMetrics(1, 2, 1000)
    dec = lambda x: np.array([[K.decimal_to_dec(Decimal(v)) for v in x]], dtype=object)       # noqa: E731

    def info(navs, passes, rej, placed, trades, passive, terms, dd, pos, ntr):
        nav = np.zeros((1, 2), K.DEC_DTYPE)
        for a, v in enumerate(navs):
            d = K.decimal_to_dec(Decimal(v))
            nav[0, a]["w"], nav[0, a]["exp"], nav[0, a]["sign"] = tuple(d.w), d.exp, d.sign
        return {"nav": nav, "is_pass_action": np.array([passes], np.uint8), "num_rejected_step": np.array([rej], np.int32), "order_step_placed": np.array([placed], np.int32),
                "num_trades_step": np.array([trades], np.int32), "num_passive_fills_step": np.array([passive], np.int32), "reward_terms": np.array([terms], np.float64),
                "drawdown": np.array([dd], np.float64), "net_position": np.array([pos], np.int32), "num_trades": np.array([ntr], np.int32)}
    z5 = [0.0] * 5
    em.feed(info(["1000", "1000"], [1, 0], [0, 1], [0, 0], [0, 0], [0, 0], [z5, [0.0, -0.1, 0, 0, 0]], [0, 0], [0, 0], [0, 0]), np.array([[0.0, -0.1]]), np.array([0]), np.array([0]))
    ended = em.feed(info(["1010.5", "989.5"], [0, 0], [0, 0], [1, 1], [6, 6], [6, 0], [[10.5, -0.1, -0.3, 0, 0.6], [-15.75, -0.1, -0.3, -2.1, 0]], [0, 10.5], [3, -3], [6, 6]),
                    np.array([[10.7, -18.25]]), np.array([0]), np.array([1]))
    assert list(ended) == [0]
    T, E = em.table()
    assert T[0, K.EM_EPISODES] == 2 and T[0, K.EM_AGENT_STEPS] == 4 and T[0, K.EM_PASSES] == 1 and T[0, K.EM_REJECTIONS] == 1 and T[0, K.EM_PLACED] == 2
    assert T[0, K.EM_TRADES] == 12 and T[0, K.EM_PASSIVE] == 6 and T[0, K.EM_MAKER_RATIO_N] == 2 and T[0, K.EM_MAKER_RATIO_MAX] == 1.0 and T[0, K.EM_MAKER_RATIO_SUM] == 1.0
    assert T[0, K.EM_NAV_MIN] == 989.5 and T[0, K.EM_NAV_MAX] == 1010.5 and T[0, K.EM_NAV_SUM] == 2000.0 and T[0, K.EM_DRAWDOWN_SUM] == 10.5 and T[0, K.EM_ABS_POSITION_SUM] == 6
    assert T[0, K.EM_TERM_SUM] == 10.5 - 15.75 and T[0, K.EM_TERM_SQ] == 10.5 ** 2 + 15.75 ** 2 and T[0, K.EM_RETURN_SUM] == pytest.approx(10.7 - 18.35)
    assert E[K.EM_ENV_EPISODES] == 1 and E[K.EM_ENV_NAV_VIOLATIONS] == 0 and E[K.EM_ENV_STEPS] == 2 and E[K.EM_ENV_MAKER_MAX_SUM] == 1.0 and E[K.EM_ENV_TERMINATED] == 0
    assert not em.violating
    em.feed(info(["1010.5", "989.6"], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [z5, z5], [0, 0], [0, 0], [0, 0]), np.zeros((1, 2)), np.array([0]), np.array([1]))
    assert len(em.violating) == 1 and em.violating[0][1] == Decimal("0.1")


# ---- one merge rule (episode_metrics.merge_tables / allreduce_tables): the device's em_combine by column, on the host and over data-parallel ranks -------------------
def _pairs_table(modules, n_modules=4, errors=(), tolerance=1e-6):
    """a table as k_em_final leaves it, from per module a list of (episode, agent) pairs (nav, maker ratio or None); every figure a multiple of 2^-10, so that the sums
    are exact in f64 whatever their order.  errors: |sum(NAV) - A * init_cash| of the episodes behind the env row"""
    t, e = np.zeros((n_modules, K.EM_AGENT_FIELDS)), np.zeros(K.EM_ENV_FIELDS)
    for m, pairs in modules.items():
        navs = [p[0] for p in pairs]
        ratios = [p[1] for p in pairs if p[1] is not None]
        t[m, K.EM_EPISODES], t[m, K.EM_AGENT_STEPS], t[m, K.EM_PASSES], t[m, K.EM_TRADES] = len(pairs), 5 * len(pairs), 2 * len(pairs), 6 * len(ratios)
        t[m, K.EM_NAV_SUM], t[m, K.EM_NAV_MIN], t[m, K.EM_NAV_MAX] = sum(navs), min(navs), max(navs)
        t[m, K.EM_RETURN_SUM], t[m, K.EM_RETURN_SQ] = sum(n - 1000 for n in navs), sum((n - 1000) ** 2 for n in navs)
        t[m, K.EM_TERM_SUM], t[m, K.EM_TERM_SQ] = t[m, K.EM_RETURN_SUM], t[m, K.EM_RETURN_SQ]
        t[m, K.EM_MAKER_RATIO_N], t[m, K.EM_MAKER_RATIO_SUM], t[m, K.EM_MAKER_RATIO_MAX] = len(ratios), sum(ratios), max(ratios, default=0.0)
    e[K.EM_ENV_EPISODES], e[K.EM_ENV_STEPS] = len(errors), 5 * len(errors)
    e[K.EM_ENV_NAV_ERROR_SUM], e[K.EM_ENV_NAV_ERROR_MAX] = sum(errors), max(errors, default=0.0)
    e[K.EM_ENV_NAV_VIOLATIONS] = sum(1 for x in errors if x > tolerance)
    return t, e


def _rank_tables():
    """three ranks' tables over four modules: module 0 played on every rank, module 1 on rank 0 only, module 2 on ranks 1 and 2, module 3 nowhere"""
    return [_pairs_table({0: [(1000.5, 0.75), (999.5, None)], 1: [(1003.0, 0.5), (997.0, 0.25)]}, errors=(0.0, 2.0 ** -30)),
            _pairs_table({0: [(1010.0, None), (990.0, 1.0)], 2: [(1000.0, None)]}, errors=(0.0,)),
            _pairs_table({0: [(998.25, 0.125)], 2: [(1001.75, 0.375), (998.25, None)]}, errors=(12.5, 2.0 ** -30))]


def _same(x, y):
    return all(np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)) for a, b in zip(x, y))


def test_merge_tables_is_the_devices_rule_by_column():
    """MIN for EM_NAV_MIN, MAX for EM_NAV_MAX / EM_MAKER_RATIO_MAX / EM_ENV_NAV_ERROR_MAX, SUM elsewhere; a rank on which a module played nothing (zeros in its row)
    does not touch that module's minimum or maximum"""
    from episode_metrics_util import assert_summary_is_consistent
    ranks = _rank_tables()
    t, e = EM.merge_tables(ranks)
    assert set(EM.AGENT_MIN_COLUMNS) == {K.EM_NAV_MIN} and set(EM.AGENT_MAX_COLUMNS) == {K.EM_NAV_MAX, K.EM_MAKER_RATIO_MAX} and set(EM.ENV_MAX_COLUMNS) == {K.EM_ENV_NAV_ERROR_MAX}
    assert sorted(EM.AGENT_SUM_COLUMNS + EM.AGENT_MIN_COLUMNS + EM.AGENT_MAX_COLUMNS) == list(range(K.EM_AGENT_FIELDS))
    assert sorted(EM.ENV_SUM_COLUMNS + EM.ENV_MAX_COLUMNS) == list(range(K.EM_ENV_FIELDS))
    want = _pairs_table({0: [(1000.5, 0.75), (999.5, None), (1010.0, None), (990.0, 1.0), (998.25, 0.125)], 1: [(1003.0, 0.5), (997.0, 0.25)],
                         2: [(1000.0, None), (1001.75, 0.375), (998.25, None)]}, errors=(0.0, 2.0 ** -30, 0.0, 12.5, 2.0 ** -30))      # the union of the pairs, collected at once
    assert _same((t, e), want)
    assert t[0, K.EM_NAV_MIN] == 990.0 and t[1, K.EM_NAV_MIN] == 997.0 and t[2, K.EM_NAV_MIN] == 998.25 and t[2, K.EM_NAV_MAX] == 1001.75      # one rank only / two of three
    assert not t[3].any()                                                      # played nowhere: k_em_final's zeros, not infinities
    assert e[K.EM_ENV_NAV_ERROR_MAX] == 12.5 and e[K.EM_ENV_NAV_VIOLATIONS] == 1 and e[K.EM_ENV_EPISODES] == 5
    s = EM.summarise(t, e, module_names=["policy_0", "policy_1", "champion_1", "champion_2"])
    assert set(s["modules"]) == {"policy_0", "policy_1", "champion_1"}
    assert_summary_is_consistent(s, "merged")
    assert s["all"]["episode_nav_min"] == 990.0 and s["all"]["episode_nav_max"] == 1010.0 and s["all"]["maker_fill_ratio_best"] == 1.0
    assert s["modules"]["policy_1"]["episode_nav_min"] == 997.0 and s["modules"]["policy_1"]["episode_nav_mean"] == 1000.0
    # ... which a SUM over the ranks - what the data-parallel league did - breaks: the "minimum" of module 0 comes out near three init_cash
    summed = EM.summarise(sum(r[0] for r in ranks), sum(r[1] for r in ranks))
    assert summed["modules"]["module_0"]["episode_nav_min"] > summed["modules"]["module_0"]["episode_nav_mean"]
    with pytest.raises(AssertionError):
        assert_summary_is_consistent(summed, "summed")


def test_merge_of_one_table_is_the_identity_and_the_merge_is_associative():
    a, b, c = _rank_tables()
    for x in (a, b, c):
        assert _same(EM.merge_tables([x]), x)
    abc = EM.merge_tables([a, b, c])
    assert _same(EM.merge_tables([EM.merge_tables([a, b]), c]), abc) and _same(EM.merge_tables([a, EM.merge_tables([b, c])]), abc)
    assert _same(EM.merge_tables([c, a, b]), abc)                               # (exact figures: commutative to the bit as well)
    # the raw identities of a module that never played (+inf / -inf: em_identity) pass through untouched, alone and beside a rank on which it did play
    raw = (a[0].copy(), a[1].copy())
    raw[0][3, K.EM_NAV_MIN], raw[0][3, K.EM_NAV_MAX], raw[0][3, K.EM_MAKER_RATIO_MAX] = np.inf, -np.inf, -np.inf
    assert _same(EM.merge_tables([raw]), raw) and _same(EM.merge_tables([raw, raw])[0][3], raw[0][3])
    played = _pairs_table({3: [(1002.0, 0.5)]}, errors=(0.0,))
    assert _same(EM.merge_tables([raw, played])[0][3], played[0][3]) and _same(EM.merge_tables([played, raw])[0][3], played[0][3])
    with pytest.raises(ValueError):
        EM.merge_tables([a, (b[0][:2], b[1])])
    with pytest.raises(ValueError):
        EM.merge_tables([])


def test_summarise_folds_the_modules_with_the_same_columns():
    """`all` is the merge of the module rows: a module that played nothing (a row of zeros) contributes neither a minimum of 0 nor a maximum of 0"""
    t, e = _pairs_table({1: [(-3.5, None)], 2: [(-1.25, 0.5)]}, errors=(0.0,))           # (negative NAVs: a zero from an idle row would be the maximum)
    s = EM.summarise(t, e)
    assert s["all"]["episode_nav_min"] == -3.5 and s["all"]["episode_nav_max"] == -1.25 and s["all"]["agent_episodes"] == 2 and s["all"]["maker_fill_ratio_best"] == 0.5
    assert "all" not in EM.summarise(np.zeros((2, K.EM_AGENT_FIELDS)), np.zeros(K.EM_ENV_FIELDS))


class _ThreadRanks:
    """two Python threads as two ranks: allreduce(rank) is the callable a rank passes to the loops (tensor, op=) - a rendezvous on a Barrier whose timeout turns a
    collective that one rank never enters into BrokenBarrierError on the other instead of a wait"""

    def __init__(self, world=2, timeout=20.0):
        import threading
        self.world, self.barrier, self.slots, self.calls = world, threading.Barrier(world, timeout=timeout), [None] * world, [[] for _ in range(world)]

    def allreduce(self, rank):
        import torch

        def allreduce(t, op="sum"):
            self.calls[rank].append((op, tuple(t.shape)))
            self.slots[rank] = t.clone()
            self.barrier.wait()
            stack = torch.stack(self.slots)
            r = stack.sum(0) if op == "sum" else (stack.min(0).values if op == "min" else stack.max(0).values)
            self.barrier.wait()                                                # (everyone has read the slots before anyone writes the next collective's)
            t.copy_(r)
            return t
        return allreduce

    def run(self, body):
        """body(rank, allreduce) on every rank's thread -> what each returned (an exception that escaped is returned too)"""
        import threading
        out = [None] * self.world

        def target(rank):
            try:
                out[rank] = body(rank, self.allreduce(rank))
            except BaseException as ex:  # noqa: BLE001 - handed to the test's thread
                out[rank] = ex
        threads = [threading.Thread(target=target, args=(r,), daemon=True) for r in range(self.world)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(60.0)
        assert not any(th.is_alive() for th in threads), "a rank is still waiting"
        return out


@pytest.mark.parametrize("strict", [True, False])
def test_a_violation_on_one_rank_stops_every_rank_in_the_same_iteration(strict):
    """log_iteration over two ranks: rank 1's shard holds the one violated episode of iteration 1.  Both ranks merge first, so both see it: strict - both raise
    NavConservationError in iteration 1 with the same message (neither is left waiting in the next collective); lenient - both log it and go on to iteration 2"""
    import torch
    a, b, c = _rank_tables()
    names = ["policy_0", "policy_1", "champion_1", "champion_2"]
    tables = [(a, b), (a, c), (b, a), (b, b)]                                  # per iteration: (rank 0's, rank 1's); c carries the violation
    ranks = _ThreadRanks()

    def body(rank, allreduce):
        history, logged, raised = [], [], None
        for it in range(4):
            t, e = tables[it][rank]
            em = (torch.from_numpy(t.copy()), torch.from_numpy(e.copy()))
            try:
                EM.log_iteration(it, {"iter": it}, em, names, history, logged.append, strict=strict, allreduce=allreduce)
            except EM.NavConservationError as ex:
                raised = (it, str(ex))
                break                                                          # a stopped run enters no further collective
        return history, logged, raised
    out = ranks.run(body)
    assert not any(isinstance(o, BaseException) for o in out), out
    (h0, l0, r0), (h1, l1, r1) = out
    assert h0 == h1 and l0 == l1 and r0 == r1                                  # every rank logs the global figures, to the word
    assert ranks.calls[0] == ranks.calls[1] and [op for op, _ in ranks.calls[0][:3]] == ["sum", "min", "max"]
    if strict:
        assert r0 is not None and r0[0] == 1 and "1 episode(s) during iteration 1" in r0[1] and "= 12.5)" in r0[1] and len(h0) == 2
    else:
        assert r0 is None and len(h0) == 4 and sum("strict_nav_check is off" in m for m in l0) == 1 and "iteration 1" in [m for m in l0 if "strict_nav_check" in m][0]
    want = EM.summarise(*EM.merge_tables([a, c]), module_names=names)
    assert h0[1]["episode_metrics"] == want and want["nav_conservation_violations"] == 1 and want["episodes"] == 4


def test_an_allreduce_that_cannot_take_min_and_max_is_refused_not_summed():
    import torch
    a, b, _ = _rank_tables()
    em = (torch.from_numpy(a[0].copy()), torch.from_numpy(a[1].copy()))
    calls = []

    def sum_only(t):
        calls.append(t)
        return t
    with pytest.raises(TypeError, match="min"):
        EM.log_iteration(0, {}, em, None, [], lambda s: None, allreduce=sum_only)
    with pytest.raises(TypeError, match="min"):
        EM.check_allreduce(lambda t: t)
    assert not calls and _same((em[0].numpy(), em[1].numpy()), a)               # refused before anything travelled
    EM.check_allreduce(lambda t, op="sum": t)
    EM.check_allreduce(lambda t, **kw: t)
    from gym_continuousdoubleauction_amd.parallel import make_grad_allreduce

    class _Dist:                                                               # (torch.distributed's names: what the product's callable maps op= to)
        class ReduceOp:
            SUM, MIN, MAX = "SUM", "MIN", "MAX"

        def __init__(self):
            self.seen = []

        def all_reduce(self, t, op, group=None):
            self.seen.append(op)
    d = _Dist()
    ar = make_grad_allreduce(d)
    EM.check_allreduce(ar)
    out = EM.allreduce_tables(em, ar)                                          # one rank: the merge of one table
    assert d.seen == ["SUM", "MIN", "MAX"] and _same((out[0].numpy(), out[1].numpy()), a)
    ar(torch.zeros(1))
    assert d.seen[-1] == "SUM"                                                 # the gradient's call is unchanged
    with pytest.raises(ValueError):
        ar(torch.zeros(1), op="prod")
