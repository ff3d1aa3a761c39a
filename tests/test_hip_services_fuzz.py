"""GPU: the device services fuzzed over random configurations, each against its own specification (tests/fuzz_cases.py service_case draws the cases,
service_extras what the quotes and schedule legs are run with).

One case = one episode on 24 markets (22 in one case: a ragged last workgroup) in which everything built on the market record runs on the SAME markets.  The ten legs:
steps (40 steps of the case's law against the CPU oracle, one oracle per distinct per-market row), book_report (against book.py), scripted (against scripted.py),
tape (the reductions against tape.py), quotes (the quote tape - series, statistics, meta rows, spread reports - against quotes.py through the host replay of the
recorder, tests/quote_replay.py), snapshot (restored into a twin env that has lived another life, and a sub-range into an env of another size), order_stream (cut
from the oracle's own next steps into the standing book, against the oracle's hooks and orders.py), schedule (an order schedule cut from the same messages, attached
to env and twin, against schedule_util.Scheduled on the oracles), steps_after (16 more steps of env, twin and oracle, the schedule's windows played inside them) and
end; where the quote ring holds more than one pass of its readers (64 records) and the horizon is long, ten more steps follow the schedule leg, so that the
episode holds 66 quotes.  Every specification is fed from HOST dumps (get_book, get_state, drain_tape), never from another device reduction.  Trade tape, quote tape and episode metrics
are on throughout (the fork env runs without quotes).  Integers, record bytes and bit views only: every comparison is exact.

The quote replay is fed, ahead of every step, each market's clock and book from the market's own oracle - behind the window's replay while a schedule is attached:
the recorder runs behind the schedule's launch - and a market is visited iff its episode is not over by ITS OWN row's max_step.  The twin's replay gets the twin's
three steps of another life from host dumps of the twin itself (no oracle follows them) and, behind the restore, the env's rows.  Under auto reset no market is ever
found past its horizon, so in cases with per-market rows the twin's other life also puts some markets' clocks at their own row's horizon, below the config's: the
recorder has to pass them by.  The schedule's kernels ask the same question of the same row, and get it in the schedule leg: behind its sixteen steps,
in looping schedules of cases with rows, every second such market's clock is put - on env, twin and the owning oracle - at or just past its own row's horizon, at
a t_step whose window holds messages, for one launch of the schedule alone (the launch every step issues first): counts, states and books must show that those
markets played nothing.  Where the restored clock coincides with the twin's next expected step the episode rule cannot tell that a restore happened; the
replay applies the same rule and says the same.

Of the schedule's fills column only this is stated: env and twin agree, a market that played nothing has none, and the tape grew by at least as many records over
the leg.  The exact split of the tape's growth into scheduled fills and the steps' own is left out: the oracle's num_trades_step counts both parties of a fill and,
without clear_step_counters, the scheduled fills too.  tests/golden/crosscheck_oracle.py --services does not replay the schedule leg: the windows go through the
oracle's one-order hooks, which the oracle's own tests hold to the reference.

CDA_FUZZ_CASES / CDA_FUZZ_SEED choose another count / stream, as in tests/test_hip_vs_oracle_batch.py; a failure names the case index and its config.  Seconds per
case on an MI355X, the twelve default cases, same machine:
  before the quotes and schedule legs   0.44 0.24 0.13 0.25 0.18 0.15 0.21 0.18 0.26 0.23 0.17 0.18   (2.6 s together; the first case carries the start of the process)
  with them                             0.84 0.32 0.17 0.34 0.26 0.21 0.33 0.26 0.38 0.36 0.30 0.28   (4.1 s together; no case doubles)
(the new cost is host work: about 1,350 get_state / get_book pairs per case and the hook replay of the windows; a profile of it showed np.ctypeslib.as_array
in the oracle's get_book as the largest single cost - now np.frombuffer - and two state dumps per replayed message where one does), so a soak of a hundred cases
stays cheap - 120 cases in 42 s: CDA_FUZZ_CASES=120 CDA_FUZZ_SEED=..."""
import math
import os
import time

import numpy as np
import pytest
import torch

import fuzz_cases as F
import services_fuzz_util as SU
from gym_continuousdoubleauction_amd import _capi as K
from gym_continuousdoubleauction_amd import book as B
from gym_continuousdoubleauction_amd import orders as OR
from gym_continuousdoubleauction_amd import quotes as Q
from gym_continuousdoubleauction_amd import scripted as S
from gym_continuousdoubleauction_amd import tape as T
from quote_replay import QuoteReplay
from services_fuzz_util import TAPE_CAPACITY, Oracles

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("CDA_FUZZ_SEED", str(F.SERVICE_SEED)))
CASES = int(os.environ.get("CDA_FUZZ_CASES", str(F.SERVICE_CASES)))
LEGS = ("steps", "book_report", "scripted", "tape", "quotes", "snapshot", "order_stream", "schedule", "steps_after", "end")      # steps 3 .. 10 of a case
TALLY = {"cases": 0, "legs": {k: 0 for k in LEGS}, "prefilled": 0, "reached_ring": 0, "wrapped": 0, "previous": 0, "seconds": [],
         "quotes_lost": 0, "quotes_previous": 0, "twin_partial": 0, "scored": 0, "long_window": 0, "scheduled_fills": 0, "row_horizons": 0, "passed_by": 0, "second_pass": 0,
         "previous_lost": 0, "schedule_passed_by": 0}
ACTION_KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset")


def _case(index):
    """the generator re-run to the index: a case does not depend on which others ran"""
    return F.service_cases(SEED, index + 1)[index]


# ---------------------------------------------------------------------------------------------------------------- the two sides
def _hip(case, n=None, quote_capacity=None):
    """tests/hip_env.HipEnv over one CDAVecEnv with the case's config and per-market rows, tape and episode metrics on - and, with a capacity, the quote tape"""
    from hip_env import HipEnv
    from gym_continuousdoubleauction_amd.vec_env import CDAVecEnv
    n = case["n_markets"] if n is None else n
    rows = case["rows"]
    e = HipEnv.__new__(HipEnv)
    e.env = CDAVecEnv(case["cfg"], n_markets=n, device="cuda:0", with_info=True, market_configs=[rows[m % len(rows)] for m in range(n)] if rows else None)
    e.n, e.A = e.env.n_markets, e.env.num_agents
    e.env.enable_tape(TAPE_CAPACITY)
    e.env.enable_episode_metrics(True)
    if quote_capacity is not None:
        e.env.enable_quotes(quote_capacity)
    return e


_prefill = SU.prefill


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


def _episode_rows(r, totals, episodes, m, episode):
    """the rows of one episode among market m's drained rows `r` (all of them, since enable_tape): the rows a step - or a stream - wrote belong to the episode the
    market was in before it"""
    label = np.repeat(episodes[:-1, m], np.diff(totals[:, m]))
    assert len(label) == len(r), (m, len(label), len(r))
    return r[label == episode]


def _tape(case, hip, totals, episodes, ctx, drained=None):
    """step 6: one drain, split per market and labelled by episode (the rows a step wrote belong to the episode the market was in before it); bars, flows and the
    execution report of the current episode - and of the previous one in short-horizon cases - against tape.py on the drained rows.  False: the tape is empty.
    drained: a list that receives every market's drained rows"""
    env, n, a = hip.env, hip.n, hip.A
    rows, off, dropped = env.drain_tape()
    rows, off = rows.cpu().numpy(), off.cpu().numpy()
    assert int(dropped.sum()) == 0, f"{ctx}: the tape dropped records"
    c = _counts(env)
    totals, episodes = np.asarray(totals), np.asarray(episodes)
    assert np.array_equal(totals[-1], c["n_total"]) and np.array_equal(np.diff(off), c["n_total"]), ctx
    if drained is not None:
        drained.extend(rows[off[m]:off[m + 1]] for m in range(n))
    bar_steps, n_bars, hz = case["bar_steps"], case["n_bars"], case["horizons"]
    for which in ("current", "previous") if case["short"] else ("current",):
        bars, binfo = (x.cpu().numpy() for x in env.tape_bars(bar_steps, n_bars, episode=which))
        flows, finfo = (x.cpu().numpy() for x in env.tape_flows(episode=which))
        stats, marks, xinfo = (x.cpu().numpy() for x in env.tape_exec(hz, episode=which))
        for m in range(n):
            x = _episode_rows(rows[off[m]:off[m + 1]], totals, episodes, m, c["episode"][m] - (which == "previous"))
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


def _quotes(case, e, replay, tape_of, ctx, who="env", episodes=None, behind_restore=False):
    """The quotes leg, on one env: quote_series, quote_stats and quote_meta of every market against the replay of its recorder (quote_replay.QuoteReplay: quotes.roll
    at the market's clock, quotes.span on the ring's capacity) and - tape_of(which, m) = the market's drained tape rows of that episode - tape_spreads against
    quotes.spreads_from_records on those rows and the held quotes.  episodes: current, and previous in short-horizon cases"""
    env, n, a, cap, hz = e.env, e.n, e.A, replay.capacity, case["horizons"]
    own = SU.horizons(case)
    meta = env.quote_meta().cpu().numpy()
    for m in range(n):
        assert Q.meta_from_words(meta[m]) == replay.rolled(m), f"{ctx}: quote meta of the {who}'s market {m}: {Q.meta_from_words(meta[m])} vs {replay.rolled(m)}"
    for which in episodes or (("current", "previous") if case["short"] else ("current",)):
        rec, cnt, info = (x.cpu().numpy() for x in env.quote_series(cap, episode=which))
        stats, sinfo = (x.cpu().numpy() for x in env.quote_stats(episode=which))
        assert rec.shape == (n, cap, Q.QUOTE_WORDS) and stats.shape == (n, Q.STAT_WORDS), ctx
        if tape_of is not None:
            spreads, pinfo = (x.cpu().numpy() for x in env.tape_spreads(hz, episode=which))
        ends = set()
        for m in range(n):
            rows, count, lost, step0, partial = replay.held(m, which)
            at = f"{ctx}: {which} quote episode of the {who}'s market {m} ({count} held, {lost} lost, from step {step0}, partial {partial}; ring of {cap})"
            assert int(cnt[m]) == count and np.array_equal(rec[m, :count], rows), f"{at}: series, {int(cnt[m])} rows, first difference {np.argwhere(rec[m, :count] != rows)[:3].tolist() if int(cnt[m]) == count else None}"
            assert not rec[m, count:].any(), f"{at}: rows beyond the count"
            assert info[m].tolist() == [count, lost, step0, partial], f"{at}: series info {info[m].tolist()}"
            want = Q.stats_from_quotes(rows)
            assert np.array_equal(stats[m], want), f"{at}: stats {dict(zip(Q.STAT_FIELDS, stats[m].tolist()))} vs {dict(zip(Q.STAT_FIELDS, want.tolist()))}"
            assert sinfo[m].tolist() == [count, lost, step0, partial], f"{at}: stats info {sinfo[m].tolist()}"
            if tape_of is not None:
                x = tape_of(which, m)
                want = Q.spreads_from_records(x, rows, hz, a)
                assert np.array_equal(spreads[m], want), f"{at}: spreads (horizons {hz}, {len(x)} fills) at {np.argwhere(spreads[m] != want)[:4].tolist()}"
                assert pinfo[m].tolist() == [len(x), 0, lost, partial << 1], f"{at}: spreads info {pinfo[m].tolist()}"
                TALLY["scored"] += int(spreads[m][..., Q.SPREAD_FIELDS.index("fills")].any())
            TALLY["quotes_lost"] += int(lost > 0)
            TALLY["second_pass"] += int(count > 64)
            if which == "previous" and count and not partial:
                TALLY["quotes_previous"] += 1
                assert step0 + count <= own[m], f"{at}: beyond the market's own horizon {own[m]}"
                ends.add(step0 + count)
            TALLY["previous_lost"] += int(which == "previous" and lost > 0 and count > 0)      # a previous episode whose head the ring overwrote, its tail held
            if behind_restore and which == "current" and partial:
                TALLY["twin_partial"] += 1
        TALLY["row_horizons"] += int(bool(case["rows"]) and len(ends) > 1)


def _pass_by(case, twin):
    """in the twin's other life: every fourth market whose own row's horizon lies below the config's gets its clock put AT that horizon - over by its row, not by
    the config.  The recorder has to pass it by (the replay, fed from the twin's host dumps, does)"""
    hz, top = SU.horizons(case), int(case["cfg"]["max_step"])
    moved = 0
    for m in range(1, twin.n, 4):
        if hz[m] < top:
            s = twin.get_state(m)
            s.t_step = hz[m]
            twin.set_state(m, s)
            moved += 1
    return moved


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
        ok = SU.stream_into_oracle(ora, m, streams[m], a, clear)
        assert np.array_equal(ok, OR.valid(mine, a)), f"{ctx}: market {m}"
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
    extras = F.service_extras(case)
    cfg, n, a, qcap = case["cfg"], case["n_markets"], case["cfg"]["num_of_agents"], extras["quote_capacity"]
    ctx = f"case {index} (CDA_FUZZ_SEED={SEED}) {cfg} law={case['law']} rows={case['rows']} quote ring {qcap} schedule {extras['schedule']}"
    rng = np.random.default_rng(case["seed"])
    legs = set()

    # 1. both sides (and the oracle copy that will write the order streams), reset on drawn seeds; the quote tape on from the start, and its host replay
    hip, ora, src = _hip(case, quote_capacity=qcap), Oracles(case), Oracles(case)
    assert hip.env.book_capacity == case["tile"] and (not case["small_ring"] or hip.env.book_spill == cfg["book_spill"]), ctx
    assert hip.env.quote_capacity == qcap and hip.env.book_spill == F.granted_ring(cfg), f"{ctx}: ring {hip.env.book_spill}"
    seeds = rng.integers(0, 2 ** 63, n).astype(np.uint64)
    obs0 = hip.reset(seeds)
    assert np.array_equal(obs0.view(np.uint32), ora.reset(seeds).view(np.uint32)), f"{ctx}: reset"
    src.reset(seeds)
    em = OracleEpisodeMetrics(n, a, cfg["init_cash"]) if case["short"] else None
    feed = None if em is None else (lambda info, rew, term, trunc: em.feed(info, rew, term, trunc, done_mask_of=lambda i: ora.get_state(i).done_mask))
    replay, replay_twin = QuoteReplay(n, qcap), QuoteReplay(n, qcap)

    # 2. deep books in every third market
    if case["prefill"]:
        _prefill(case, (hip, ora, src))
        TALLY["prefilled"] += 1
        tails = [_ring_meta(hip.env, m) for m in range(0, n, 3)]
        TALLY["reached_ring"] += int(any(t[0] > 0 or t[1] > 0 for t, _ in tails))

    # 3. the law, every output against the oracle
    c = _counts(hip.env)
    totals, episodes = [c["n_total"]], [c["episode"]]

    def law_steps(count, envs, leg, spec=None):
        for t in range(count):
            acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
            if spec is not None:                               # the windows of this step, through the oracle's hooks
                spec.play_all()
            SU.feed_quotes((replay, replay_twin) if envs else (replay,), ora, case)      # the recorder runs behind the schedule's launch, ahead of the step
            want = ora.step(acts, present, feed)
            if src is not None and leg == "steps":
                src.step(acts, present)
            got = hip.step(*acts, present)
            if spec is not None:                               # the schedule leg's own statement, step by step: what the window's launch counted
                counted = hip.env.order_schedule_counts().cpu().numpy()[:, :3]
                assert np.array_equal(counted, spec.counts[:, :3]), f"{ctx}: {leg} {t}: schedule counts (done, rejected, invalid) at markets {np.flatnonzero((counted != spec.counts[:, :3]).any(axis=1)).tolist()}"
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
    drained = []
    if _tape(case, hip, totals, episodes, ctx, drained):
        legs.add("tape")

    def tape_of(which, m):
        return _episode_rows(drained[m], np.asarray(totals), np.asarray(episodes), m, episodes[-1][m] - (which == "previous"))

    SU.set_clocks(replay, ora, n)
    _quotes(case, hip, replay, tape_of, ctx)
    legs.add("quotes")

    # 7. snapshot -> a twin that has lived another life, and a sub-range -> an env of another size
    snap = hip.env.snapshot()
    twin = _hip(case, quote_capacity=qcap)
    twin.reset(rng.integers(0, 2 ** 63, n).astype(np.uint64))
    if case["prefill"]:
        _prefill(case, (twin,), seed_shift=1)
    for t in range(3):
        acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
        if t == 1 and case["rows"]:
            TALLY["passed_by"] += int(_pass_by(case, twin) > 0)
        SU.feed_quotes((replay_twin,), twin, case)             # host dumps of the twin itself: no oracle follows these steps
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
    SU.set_clocks(replay_twin, twin, n)                         # the restore moved the twin's clocks: its readers roll to them
    _quotes(case, twin, replay_twin, None, f"{ctx}: behind the restore", who="twin", episodes=("current", "previous"), behind_restore=True)
    wrapped = 0
    for m in range(0, n, 3):
        tails, bases = _ring_meta(hip.env, m)
        ring = hip.env.book_spill
        wrapped += int(any(tails[s] > 0 and (bases[s] & (ring - 1)) + tails[s] > ring for s in (0, 1)))
    TALLY["wrapped"] += int(wrapped > 0)
    legs.add("snapshot")

    # 8. an order stream into the standing book (it moves no clock and the recorder does not run: the tape's bookkeeping takes its rows)
    streams, pools = SU.cut_streams(case, src, rng)
    src.close()
    src = None
    if _order_stream(case, hip, twin, ora, streams, ctx):
        legs.add("order_stream")
    c = _counts(hip.env)
    totals.append(c["n_total"]); episodes.append(c["episode"])

    # 9. the law again, an order schedule attached to env and twin: nothing stale behind the stream and the restore, and every step plays its windows first
    sc = extras["schedule"]
    rows = SU.schedule_rows(case, extras, pools)
    assert [[len(w) for w in row] for row in rows] == extras["lengths"], f"{ctx}: the schedule's rows"
    for e in (hip, twin):
        e.env.set_order_schedule(rows, market_schedule=sc["market_schedule"], loop=sc["loop"], clear_step_counters=sc["clear_step_counters"])
    spec = SU.scheduled(case, extras, ora, rows)
    grown = _counts(hip.env)["n_total"]
    law_steps(F.SERVICE_STEPS_AFTER, (twin,), "steps_after", spec)
    for m in range(n):
        _same_market(hip, ora, m, f"{ctx}: at the end, env vs oracle")
        _same_market(twin, hip, m, f"{ctx}: at the end, twin vs env")
    legs.add("steps_after")
    grown = _counts(hip.env)["n_total"] - grown
    counts, counts_twin = (e.env.order_schedule_counts().cpu().numpy() for e in (hip, twin))
    assert np.array_equal(counts[:, :3], spec.counts[:, :3]), f"{ctx}: schedule counts (done, rejected, invalid) at markets {np.flatnonzero((counts[:, :3] != spec.counts[:, :3]).any(axis=1)).tolist()}"
    assert np.array_equal(counts_twin, counts), f"{ctx}: schedule counts of env and twin"
    quiet = counts[:, :3].sum(axis=1) == 0
    assert (counts[quiet, 3] == 0).all() and (counts[:, 3] >= 0).all() and (counts[:, 3] <= grown).all(), f"{ctx}: scheduled fills {counts[:, 3].tolist()} vs the tape's growth {grown.tolist()}"
    assert (counts[sc["market_schedule"] < 0] == 0).all(), f"{ctx}: a market without a row played something"
    # ... and one play past a row's horizon: clocks put, through the state dump, where the market's OWN row says the episode is over and the config's horizon
    # does not (services_fuzz_util.clocks_past_the_row_horizon), on env, twin and the owning oracle; the schedule's launch alone - the launch every step issues
    # first - must pass those markets by, window and all, while the others play their window once more; then the clocks go back
    clocks = SU.clocks_past_the_row_horizon(case, extras)
    if clocks:
        moved = sorted(clocks)
        had = SU.move_clocks((hip, twin, ora), clocks)
        for m in moved:
            r, t = int(sc["market_schedule"][m]), clocks[m]
            assert SU.horizons(case)[m] <= t < cfg["max_step"] and len(rows[r][t % sc["n_windows"]]) > 0, f"{ctx}: market {m}"
        image = {m: (bytes(hip.get_state(m)), hip.get_book(m, 0).tobytes(), hip.get_book(m, 1).tobytes()) for m in moved}
        for e in (hip, twin):
            e.env.play_order_schedule()
        spec.play_all()
        after, after_twin = (e.env.order_schedule_counts().cpu().numpy() for e in (hip, twin))
        assert np.array_equal(after[moved], counts[moved]) and np.array_equal(after_twin[moved], counts[moved]), \
            f"{ctx}: past their own row's horizon, markets {[m for m in moved if (after[m] != counts[m]).any()]} played a window"
        assert np.array_equal(after[:, :3], spec.counts[:, :3]) and np.array_equal(after_twin, after), f"{ctx}: schedule counts behind the play past the row's horizon"
        for m in moved:
            assert image[m] == (bytes(hip.get_state(m)), hip.get_book(m, 0).tobytes(), hip.get_book(m, 1).tobytes()), f"{ctx}: past its row's horizon, market {m} changed"
        SU.move_clocks((hip, twin, ora), had)
        for m in range(n):
            _same_market(hip, ora, m, f"{ctx}: behind the play past the row's horizon, env vs oracle")
            _same_market(twin, hip, m, f"{ctx}: behind the play past the row's horizon, twin vs env")
        c = _counts(hip.env)                                   # (the windows the other markets played wrote tape rows: no step, the episode they are in)
        totals.append(c["n_total"]); episodes.append(c["episode"])
        TALLY["schedule_passed_by"] += 1
    for e in (hip, twin):
        e.env.clear_order_schedule()
        assert not e.env.order_schedule
    if spec.played:
        legs.add("schedule")
        TALLY["long_window"] += int(max(k for *_, k in spec.played) >= 64)
        TALLY["scheduled_fills"] += int(counts[:, 3].sum() > 0)
    if extras["tail_steps"]:                                   # a quote ring that holds more than one pass of its readers: an episode of more than 64 quotes
        law_steps(extras["tail_steps"], (twin,), "tail")
        for m in range(n):
            _same_market(hip, ora, m, f"{ctx}: behind the tail, env vs oracle")
            _same_market(twin, hip, m, f"{ctx}: behind the tail, twin vs env")

    # 10. the end of the case
    second = None
    for e, who in ((hip, "env"), (twin, "twin")):
        assert (e.env.check_invariants().cpu().numpy() == 0).all(), f"{ctx}: invariants of the {who}"
        assert np.array_equal(e.flags(), ora.flags()), f"{ctx}: flags of the {who} {e.flags().tolist()} vs the oracle's {ora.flags().tolist()}"
        more, off, dropped = e.env.drain_tape()
        assert int(dropped.sum()) == 0, f"{ctx}: the {who}'s tape dropped records"
        if e is hip:
            second = (more.cpu().numpy(), off.cpu().numpy())
    drained = [np.concatenate([drained[m], second[0][second[1][m]:second[1][m + 1]]]) for m in range(n)]      # both drains: every row since enable_tape
    assert [len(r) for r in drained] == totals[-1].tolist(), f"{ctx}: the two drains"
    for rp in (replay, replay_twin):
        SU.set_clocks(rp, ora, n)
    _quotes(case, hip, replay, tape_of, f"{ctx}: at the end")
    _quotes(case, twin, replay_twin, None, f"{ctx}: at the end", who="twin")
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
    """the module's tally: every leg (steps 3 to 10) ran on at least 10 of 12 cases, a prefilled case really reached the HBM ring, a short-horizon case really
    compared a previous episode - and the two new legs really met what they are there for.  Only judged when the whole parametrised set ran in this session (not
    under -k)."""
    if TALLY["cases"] != CASES:
        return
    need = math.ceil(CASES * 10 / 12)
    for leg, count in TALLY["legs"].items():
        assert count >= need, (leg, count, need)
    if SEED == F.SERVICE_SEED and CASES >= F.SERVICE_CASES:
        assert TALLY["prefilled"] >= 1 and TALLY["reached_ring"] >= 1, TALLY
        assert TALLY["previous"] >= 1, TALLY
        assert TALLY["quotes_lost"] >= 1, TALLY                # a quote ring wrapped
        assert TALLY["quotes_previous"] >= 1, TALLY            # a previous quote episode was compared
        assert TALLY["twin_partial"] >= 1, TALLY               # a twin showed a partial current episode behind the restore
        assert TALLY["scored"] >= 1, TALLY                     # a tape_spreads cell with scored fills
        assert TALLY["long_window"] >= 1, TALLY                # a scheduled window of 64 or more messages was played
        assert TALLY["scheduled_fills"] >= 1, TALLY
        assert TALLY["row_horizons"] >= 1, TALLY               # with per-market rows, markets left the recorder at different horizons of their own
        assert TALLY["passed_by"] >= 1, TALLY                  # a clock at its row's horizon, below the config's
        assert TALLY["second_pass"] >= 1, TALLY                # an episode of more than 64 held quotes: the readers' second pass
        assert TALLY["previous_lost"] >= 1, TALLY              # a previous quote episode whose head the ring had overwritten (short episodes on a small ring)
        assert TALLY["schedule_passed_by"] >= 1, TALLY         # the schedule passed by markets over by their own row's horizon, below the config's
    print(f"services fuzz: {CASES} cases, seconds per case {[round(s, 2) for s in TALLY['seconds']]}, tally {TALLY}")
