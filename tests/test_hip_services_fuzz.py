"""GPU: the device services fuzzed over random configurations, each against its own specification (tests/fuzz_cases.py service_case draws the cases).

One case = one episode on 24 markets (22 in one case: a ragged last workgroup) in which everything built on the market record runs on the SAME markets: 40 steps of
the case's law against the CPU oracle (one oracle per distinct per-market row), then the book report against book.py, the scripted laws against scripted.py, the tape
reductions against tape.py - all three fed from HOST dumps (get_book, get_state, drain_tape), never from another device reduction -, a snapshot restored into a twin
env and a sub-range into an env of another size, an order stream cut from the oracle's own next steps into the standing book against the oracle's hooks and orders.py,
and 16 more steps of env, twin and oracle.  Trade tape and episode metrics are on throughout.  Integers, record bytes and bit views only: every comparison is exact.

CDA_FUZZ_CASES / CDA_FUZZ_SEED choose another count / stream, as in tests/test_hip_vs_oracle_batch.py; a failure names the case index and its config.  A case takes
0.13 to 0.8 s on an MI355X (the twelve default cases 5 s together), so a soak of hundreds of cases is cheap: CDA_FUZZ_CASES=120 CDA_FUZZ_SEED=..."""
import math
import os
import time

import numpy as np
import pytest
import torch

import fuzz_cases as F
import oracle_lib as O
from gym_continuousdoubleauction_amd import _capi as K
from gym_continuousdoubleauction_amd import book as B
from gym_continuousdoubleauction_amd import orders as OR
from gym_continuousdoubleauction_amd import scripted as S
from gym_continuousdoubleauction_amd import tape as T

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("CDA_FUZZ_SEED", str(F.SERVICE_SEED)))
CASES = int(os.environ.get("CDA_FUZZ_CASES", str(F.SERVICE_CASES)))
LEGS = ("steps", "book_report", "scripted", "tape", "snapshot", "order_stream", "steps_after", "end")      # steps 3 .. 10 of a case
TALLY = {"cases": 0, "legs": {k: 0 for k in LEGS}, "prefilled": 0, "reached_ring": 0, "wrapped": 0, "previous": 0, "seconds": []}
ACTION_KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset")
COUNTERS = ("num_trades_step", "num_passive_fills_step", "order_step_placed", "num_rejected_step")
TAPE_CAPACITY = 4096        # a fill consumes a resting order or ends its taker: at most 2 x 512 prefilled + 2 x (56 steps x 16 agents + 134 messages) < 4096 per market


def _case(index):
    """the generator re-run to the index: a case does not depend on which others ran"""
    return F.service_cases(SEED, index + 1)[index]


# ---------------------------------------------------------------------------------------------------------------- the two sides
def _hip(case, n=None):
    """tests/hip_env.HipEnv over one CDAVecEnv with the case's config and per-market rows, tape and episode metrics on"""
    from hip_env import HipEnv
    from gym_continuousdoubleauction_amd.vec_env import CDAVecEnv
    n = case["n_markets"] if n is None else n
    rows = case["rows"]
    e = HipEnv.__new__(HipEnv)
    e.env = CDAVecEnv(case["cfg"], n_markets=n, device="cuda:0", with_info=True, market_configs=[rows[m % len(rows)] for m in range(n)] if rows else None)
    e.n, e.A = e.env.n_markets, e.env.num_agents
    e.env.enable_tape(TAPE_CAPACITY)
    e.env.enable_episode_metrics(True)
    return e


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

    def place_order(self, m, *a):
        self.of(m).place_order(m, *a)

    def mark_to_mkt(self, m):
        self.of(m).mark_to_mkt(m)

    def flags(self):
        return self._mix([o.flags() for o in self.o])

    def close(self):
        for o in self.o:
            o.close()


def _prefill(case, envs, seed_shift=0):
    """every third market of every env gets the same deep book (fuzz_cases.prefill_book through the state dump)"""
    n, a = case["n_markets"], case["cfg"]["num_of_agents"]
    for m in range(0, n, 3):
        nb, na = F.service_prefill_sizes(case, m + seed_shift)
        for e in envs:
            F.prefill_book(e, m, np.random.default_rng(case["prefill_seed"] + 7 * seed_shift + m + 1), a, nb, na)


def _ring_meta(env, market):
    """(orders in the HBM ring per side, ring base per side) of one market, from a snapshot's section (csrc/cda_snapshot.inc SnapMeta behind the record)"""
    blob = env.snapshot(market, 1).blob.cpu().numpy()
    at = int(blob[256:264].view(np.int64)[0]) + env.state_bytes_per_market()
    meta = blob[at:at + 32].view(np.int32)
    return (int(meta[2]), int(meta[3])), (int(meta[4]), int(meta[5]))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _same_outputs(got, want, ctx):
    for name, g, w in zip(("obs", "reward", "terminated", "truncated"), got[:4], want[:4]):
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), f"{ctx}: {name}, markets {np.flatnonzero((np.asarray(g) != np.asarray(w)).reshape(len(g), -1).any(axis=1))[:8]}"
    for k in want[4]:
        assert np.array_equal(_bits(got[4][k]), _bits(want[4][k])), f"{ctx}: info.{k}"


def _same_market(got, want, m, ctx):
    assert bytes(got.get_state(m)) == bytes(want.get_state(m)), f"{ctx}: state of market {m}"
    for side in (0, 1):
        g, w = got.get_book(m, side), want.get_book(m, side)
        assert g.shape == w.shape and np.array_equal(g, w), f"{ctx}: book of market {m} side {side} ({g.shape} vs {w.shape})"


def _play_hooks(env, market, stream):
    for msg in stream:
        if msg == OR.MARK:
            env.mark_to_mkt(market)
        else:
            tr, typ, side, size, price = msg[:5]
            env.place_order(market, tr, typ, side, size, price if typ != K.T_MARKET else 1)


def _counts(env):
    return {k: v.cpu().numpy().copy() for k, v in env.tape_counts().items()}


# ---------------------------------------------------------------------------------------------------------------- the legs
def _book_report(case, hip, ctx):
    """step 4: the five readers, all markets, against book.py on the HOST dumps; returns the dumps"""
    env, n, a = hip.env, hip.n, hip.A
    books = [hip.get_book(m) for m in range(n)]
    L, sizes = case["levels"], case["impact_sizes"]
    want = B.report_from_books(books, a, L, sizes)
    rows, off = env.book_orders()
    got = {"counts": env.book_counts(), "levels": env.book_levels(L), "impact": env.book_impact(sizes), "agents": env.book_agents(), "orders": rows, "offsets": off}
    for k, v in got.items():
        g = v.cpu().numpy()
        assert g.shape == want[k].shape and g.dtype == want[k].dtype and np.array_equal(g, want[k]), \
            f"{ctx}: book_{k} (L={L}, sizes={sizes}) at {np.argwhere(g != want[k])[:4].tolist() if g.shape == want[k].shape else (g.shape, want[k].shape)}"
    for m in range(n):                                       # ... and the one-side statements on the same dumps
        for s in (0, 1):
            assert np.array_equal(got["counts"][m, s].cpu().numpy(), B.counts_from_orders(books[m][s])), f"{ctx}: counts of market {m} side {s}"
    return books


def _ticks(case, n):
    base = int(case["cfg"].get("tick_size", 1))
    rows = case["rows"]
    return [int(rows[m % len(rows)]["tick_size"]) if rows else base for m in range(n)]


def _scripted(case, hip, books, ctx):
    """step 5: k_script_actions against scripted.py; the views come from book.py on the host dumps, get_state and the rows - no device reduction feeds them"""
    env, n, a = hip.env, hip.n, hip.A
    slots, profiles = case["slots"], case["profiles"]
    env.set_scripted(slots, profiles, seed=case["script_seed"], market_index_base=case["script_base"])
    pix = np.maximum(slots - 1, 0)
    depth = np.array([p.depth_levels for p in profiles])[pix]
    rep = B.report_from_books(books, a, max_levels=S.MAX_DEPTH)
    states = [hip.get_state(m) for m in range(n)]
    pos = [[int(s.acc[j].net_position) for j in range(a)] for s in states]
    views = S.views_from_report(rep["levels"], rep["agents"], pos, [int(s.t_step) for s in states], _ticks(case, n), depth)
    m, j = np.meshgrid(np.arange(n), np.arange(a), indexing="ij")
    draw, counter = case["script_draw"], case["script_counter"]
    want = S.actions_from_views(profiles, pix, views, case["script_seed"], counter, case["script_base"] + m, draw, j)
    got = env.scripted_actions(draw=draw, counter=counter)
    on = slots != 0
    for k, w in zip(ACTION_KEYS, want):
        g = got[k].cpu().numpy()
        assert np.array_equal(g[on].view(np.uint32), w[on].view(np.uint32)), f"{ctx}: scripted {k} at (market, agent) {np.argwhere((g.view(np.uint32) != w.view(np.uint32)) & on)[:4].tolist()}"
    env.clear_scripted()
    assert not env.scripted


def _tape(case, hip, totals, episodes, ctx):
    """step 6: one drain, split per market and labelled by episode (the rows a step wrote belong to the episode the market was in before it); bars, flows and the
    execution report of the current episode - and of the previous one in short-horizon cases - against tape.py on the drained rows.  False: the tape is empty"""
    env, n, a = hip.env, hip.n, hip.A
    rows, off, dropped = env.drain_tape()
    rows, off = rows.cpu().numpy(), off.cpu().numpy()
    assert int(dropped.sum()) == 0, f"{ctx}: the tape dropped records"
    c = _counts(env)
    totals, episodes = np.asarray(totals), np.asarray(episodes)
    assert np.array_equal(totals[-1], c["n_total"]) and np.array_equal(np.diff(off), c["n_total"]), ctx
    bar_steps, n_bars, hz = case["bar_steps"], case["n_bars"], case["horizons"]
    for which in ("current", "previous") if case["short"] else ("current",):
        bars, binfo = (x.cpu().numpy() for x in env.tape_bars(bar_steps, n_bars, episode=which))
        flows, finfo = (x.cpu().numpy() for x in env.tape_flows(episode=which))
        stats, marks, xinfo = (x.cpu().numpy() for x in env.tape_exec(hz, episode=which))
        for m in range(n):
            r = rows[off[m]:off[m + 1]]
            label = np.repeat(episodes[:-1, m], np.diff(totals[:, m]))
            assert len(label) == len(r), f"{ctx}: market {m}"
            x = r[label == c["episode"][m] - (which == "previous")]
            at = f"{ctx}: {which} episode of market {m} ({len(x)} rows)"
            assert int(c["n_episode" if which == "current" else "n_previous"][m]) == len(x), at
            want_bars, beyond = T.bars_from_records(x, bar_steps, n_bars)
            assert np.array_equal(bars[m].reshape(-1), want_bars.view(np.int32)), f"{at}: bars({bar_steps}, {n_bars})"
            assert binfo[m].tolist() == [len(x) - beyond, 0, beyond, 0], f"{at}: bars info {binfo[m].tolist()}"
            assert np.array_equal(flows[m], T.flows_from_records(x, a)) and finfo[m].tolist() == [len(x), 0, 0, 0], f"{at}: flows"
            want_s, want_m = T.exec_from_records(x, a, hz)
            assert np.array_equal(stats[m], want_s), f"{at}: exec stats (horizons {hz}) at {np.argwhere(stats[m] != want_s)[:4].tolist()}"
            assert np.array_equal(marks[m], want_m), f"{at}: mark-outs (horizons {hz}) at {np.argwhere(marks[m] != want_m)[:4].tolist()}"
            assert xinfo[m].tolist() == [len(x), 0, 0, 0], f"{at}: exec info"
        if which == "previous" and int(c["n_previous"].sum()) > 0:
            TALLY["previous"] += 1
    return len(rows) > 0


def _cut_streams(case, src, rng, ctx):
    """step 8's input: the oracle copy plays the law's next steps; every market's decoded orders in execution order, cut (repeated if need be) to the drawn length;
    in two markets one invalid message of each kind is spliced in"""
    n, a = case["n_markets"], case["cfg"]["num_of_agents"]
    la, ex = [], []
    for _ in range(F.STREAM_SOURCE_STEPS):
        acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
        *_, info = src.step(acts, present)
        la.append(info["lob_actions"].copy()); ex.append(src.exec_order())
    la, ex = np.stack(la), np.stack(ex)
    streams = []
    for m in range(n):
        st, want = OR.from_lob_actions(la[:, m], ex[:, m], mark_every=case["mark_every"]), int(case["stream_lengths"][m])
        streams.append((st * (want // len(st) + 1))[:want] if st and want else [])
    for m in case["invalid_markets"]:
        for pos, bad in sorted(zip(rng.integers(0, len(streams[m]) + 1, 5).tolist(), F.invalid_messages(a)), reverse=True):
            streams[m].insert(pos, bad)
    return streams


def _order_stream(case, hip, twin, ora, streams, ctx):
    """step 8: one submit on env and twin (one of them in windows of max_per_launch), the same messages through the oracle's hooks"""
    n, a, clear = hip.n, hip.A, case["clear_step_counters"]
    before = {e: _counts(e.env)["n_total"] for e in (hip, twin)}
    out = {}
    for e in (hip, twin):
        windowed = (e is twin) == case["split_twin"]
        res, summary = e.env.submit_orders([list(s) for s in streams], clear_step_counters=clear, max_per_launch=case["max_per_launch"] if windowed else 65536)
        out[e] = (res.cpu().numpy().view(OR.RESULT_DTYPE).reshape(-1), summary.cpu().numpy())
    off, msgs = OR.pack(streams)
    res, summary = out[hip]
    assert out[twin][0].tobytes() == res.tobytes() and np.array_equal(out[twin][1], summary), f"{ctx}: env and twin (max_per_launch {case['max_per_launch']}) disagree"
    assert len(res) == len(msgs)
    for m in range(n):
        mine = msgs[off[m]:off[m + 1]]
        ok = OR.valid(mine, a)
        _play_hooks(ora, m, [st for st, good in zip(streams[m], ok) if good])
        if clear and ok.any():                               # (a market without a valid message is not touched: csrc/cda_orders.inc)
            s = ora.get_state(m)
            for j in range(a):
                for key in COUNTERS:
                    setattr(s.acc[j], key, 0)
            ora.set_state(m, s)
        at = f"{ctx}: stream of market {m} ({len(mine)} messages)"
        assert np.array_equal(summary[m], OR.summary_of(res[off[m]:off[m + 1]])), f"{at}: summary {summary[m].tolist()}"
        assert summary[m, 2] == int((~ok).sum()) and (OR.check(mine, a) == -1) == (summary[m, 2] == 0), f"{at}: invalid count {summary[m, 2]}"
        if not ok.all():
            assert OR.check(mine, a) == int(np.flatnonzero(~ok)[0]) and (res[off[m]:off[m + 1]]["status"][~ok] == OR.ORD_INVALID).all(), at
        assert summary[m, 0] + summary[m, 1] == int(ok.sum()), at
    for m in case["invalid_markets"]:
        assert summary[m, 2] == 5, f"{ctx}: market {m}"
    for e in (hip, twin):
        grown = _counts(e.env)["n_total"] - before[e]
        assert np.array_equal(grown, summary[:, 3]), f"{ctx}: the tape's new rows {grown.tolist()} vs the summaries' fills {summary[:, 3].tolist()}"
    for m in range(n):
        _same_market(hip, ora, m, f"{ctx}: after the stream, env vs oracle")
        _same_market(twin, hip, m, f"{ctx}: after the stream, twin vs env")
    return len(msgs) > 0


# ---------------------------------------------------------------------------------------------------------------- one case
@pytest.mark.parametrize("index", range(CASES))
def test_services_on_a_random_configuration(index):
    from episode_metrics_util import OracleEpisodeMetrics, assert_tables_equal
    t0 = time.perf_counter()
    case = _case(index)
    cfg, n, a = case["cfg"], case["n_markets"], case["cfg"]["num_of_agents"]
    ctx = f"case {index} (CDA_FUZZ_SEED={SEED}) {cfg} law={case['law']} rows={case['rows']}"
    rng = np.random.default_rng(case["seed"])
    legs = set()

    # 1. both sides (and the oracle copy that will write the order streams), reset on drawn seeds
    hip, ora, src = _hip(case), Oracles(case), Oracles(case)
    assert hip.env.book_capacity == case["tile"] and (not case["small_ring"] or hip.env.book_spill == cfg["book_spill"]), ctx
    seeds = rng.integers(0, 2 ** 63, n).astype(np.uint64)
    obs0 = hip.reset(seeds)
    assert np.array_equal(obs0.view(np.uint32), ora.reset(seeds).view(np.uint32)), f"{ctx}: reset"
    src.reset(seeds)
    em = OracleEpisodeMetrics(n, a, cfg["init_cash"]) if case["short"] else None
    feed = None if em is None else (lambda info, rew, term, trunc: em.feed(info, rew, term, trunc, done_mask_of=lambda i: ora.get_state(i).done_mask))

    # 2. deep books in every third market
    if case["prefill"]:
        _prefill(case, (hip, ora, src))
        TALLY["prefilled"] += 1
        tails = [_ring_meta(hip.env, m) for m in range(0, n, 3)]
        TALLY["reached_ring"] += int(any(t[0] > 0 or t[1] > 0 for t, _ in tails))

    # 3. the law, every output against the oracle
    c = _counts(hip.env)
    totals, episodes = [c["n_total"]], [c["episode"]]

    def law_steps(count, envs, leg):
        for t in range(count):
            acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
            want = ora.step(acts, present, feed)
            if src is not None and leg == "steps":
                src.step(acts, present)
            got = hip.step(*acts, present)
            _same_outputs(got, want, f"{ctx}: {leg} {t}")
            for e in envs:
                _same_outputs(e.step(*acts, present), got, f"{ctx}: {leg} {t}, twin vs env")
            c = _counts(hip.env)
            totals.append(c["n_total"]); episodes.append(c["episode"])

    law_steps(F.SERVICE_STEPS, (), "steps")
    for m in range(n):
        _same_market(hip, ora, m, f"{ctx}: after {F.SERVICE_STEPS} steps")
    if case["short"]:
        assert (np.asarray(episodes)[-1] - np.asarray(episodes)[0] >= 2).all(), f"{ctx}: episodes did not end"
    legs.add("steps")

    # 4. - 6. the readers
    books = _book_report(case, hip, ctx)
    legs.add("book_report")
    _scripted(case, hip, books, ctx)
    legs.add("scripted")
    if _tape(case, hip, totals, episodes, ctx):
        legs.add("tape")

    # 7. snapshot -> a twin that has lived another life, and a sub-range -> an env of another size
    snap = hip.env.snapshot()
    twin = _hip(case)
    twin.reset(rng.integers(0, 2 ** 63, n).astype(np.uint64))
    if case["prefill"]:
        _prefill(case, (twin,), seed_shift=1)
    for t in range(3):
        acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
        twin.step(*acts, present)
    twin.env.obs.fill_(float("nan"))
    twin.env.restore(snap)
    assert torch.equal(twin.env.obs.view(torch.int32), hip.env.obs.view(torch.int32)), f"{ctx}: the restored observation"
    assert torch.equal(twin.env.snapshot().blob, snap.blob), f"{ctx}: the twin's snapshot differs from the one it was restored from"
    fk = case["fork"]
    third = _hip(case, n=fk["n_markets"])
    third.reset(rng.integers(0, 2 ** 63, fk["n_markets"]).astype(np.uint64))
    third.env.restore(snap, first=fk["first"], src_first=fk["src_first"], n=fk["n"])
    lo, so = fk["first"], fk["src_first"]
    assert torch.equal(third.env.obs[lo:lo + fk["n"]].view(torch.int32), hip.env.obs[so:so + fk["n"]].view(torch.int32)), f"{ctx}: fork {fk}"
    for i in range(fk["n"]):
        assert bytes(third.get_state(lo + i)) == bytes(hip.get_state(so + i)), f"{ctx}: fork {fk}, market {i}"
        for side in (0, 1):
            assert np.array_equal(third.get_book(lo + i, side), hip.get_book(so + i, side)), f"{ctx}: fork {fk}, market {i} side {side}"
    third.close()
    for m in range(n):
        _same_market(twin, hip, m, f"{ctx}: restored twin")
    wrapped = 0
    for m in range(0, n, 3):
        tails, bases = _ring_meta(hip.env, m)
        ring = hip.env.book_spill
        wrapped += int(any(tails[s] > 0 and (bases[s] & (ring - 1)) + tails[s] > ring for s in (0, 1)))
    TALLY["wrapped"] += int(wrapped > 0)
    legs.add("snapshot")

    # 8. an order stream into the standing book
    streams = _cut_streams(case, src, rng, ctx)
    src.close()
    src = None
    if _order_stream(case, hip, twin, ora, streams, ctx):
        legs.add("order_stream")

    # 9. the law again: nothing stale behind the stream and the restore
    law_steps(F.SERVICE_STEPS_AFTER, (twin,), "steps_after")
    for m in range(n):
        _same_market(hip, ora, m, f"{ctx}: at the end, env vs oracle")
        _same_market(twin, hip, m, f"{ctx}: at the end, twin vs env")
    legs.add("steps_after")

    # 10. the end of the case
    for e, who in ((hip, "env"), (twin, "twin")):
        assert (e.env.check_invariants().cpu().numpy() == 0).all(), f"{ctx}: invariants of the {who}"
        assert np.array_equal(e.flags(), ora.flags()), f"{ctx}: flags of the {who} {e.flags().tolist()} vs the oracle's {ora.flags().tolist()}"
        _, _, dropped = e.env.drain_tape()
        assert int(dropped.sum()) == 0, f"{ctx}: the {who}'s tape dropped records"
    dev, dev_twin = ([t.cpu().numpy() for t in e.env.collect_episode_metrics()] for e in (hip, twin))
    for x, y in zip(dev, dev_twin):
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), f"{ctx}: episode metrics of env and twin"
    if em is not None:
        ref = em.table()
        assert ref[1][K.EM_ENV_EPISODES] >= 2 * n, ctx
        assert_tables_equal(dev[0], dev[1], *ref, what=ctx)
    legs.add("end")
    hip.close(); twin.close(); ora.close()
    TALLY["cases"] += 1
    for k in legs:
        TALLY["legs"][k] += 1
    TALLY["seconds"].append(time.perf_counter() - t0)
    print(f"services fuzz case {index}: {TALLY['seconds'][-1]:.2f} s, legs {sorted(legs)}")


def test_every_leg_ran_on_almost_every_case():
    """the module's tally: every leg (steps 3 to 10) ran on at least 10 of 12 cases, a prefilled case really reached the HBM ring, and a short-horizon case really
    compared a previous episode.  Only judged when the whole parametrised set ran in this session (not under -k)."""
    if TALLY["cases"] != CASES:
        return
    need = math.ceil(CASES * 10 / 12)
    for leg, count in TALLY["legs"].items():
        assert count >= need, (leg, count, need)
    if SEED == F.SERVICE_SEED and CASES >= F.SERVICE_CASES:
        assert TALLY["prefilled"] >= 1 and TALLY["reached_ring"] >= 1, TALLY
        assert TALLY["previous"] >= 1, TALLY
    print(f"services fuzz: {CASES} cases, seconds per case {[round(s, 2) for s in TALLY['seconds']]}, tally {TALLY}")
