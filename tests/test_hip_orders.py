"""GPU: order streams (include/cda.h cda_submit_orders; CDAVecEnv.submit_orders / seed_books; gym_continuousdoubleauction_amd/orders.py) - a whole per-market
list of explicit messages played in one launch must leave every market exactly where the one-order hooks (cda_place_order, cda_mark_to_mkt) leave it, and where
the CPU oracle's own hooks leave the oracle.  Integers and record bytes only: every comparison is exact."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import golden_util as G
import oracle_lib as O
from gym_continuousdoubleauction_amd import _capi as K
from gym_continuousdoubleauction_amd import orders as OR

pytestmark = pytest.mark.gpu

A = 4
LENGTHS = (0, 1, 63, 64, 65, 130)                   # the chunk is 64 messages: none, one, one short of it, exactly it, one over, two chunks and a bit
SEEDS = np.arange(700, 706, dtype=np.uint64)
COUNTERS = ("num_trades_step", "num_passive_fills_step", "order_step_placed", "num_rejected_step")


def _cfg(cap, **kw):
    return dict({"num_of_agents": A, "init_cash": 20000, "max_step": 256, "is_render": False, "book_capacity": cap}, **kw)


def _law(rng, n, a):
    """random actions with every order type well represented (the shape of tests/test_hip_bigbook.py's law)"""
    cat = rng.choice([1, 1, 2, 2, 2, 3, 3, 4, 5, 5, 6, 6, 6, 7, 7, 8, 0], (n, a)).astype(np.int32)
    price = rng.choice([0, 0, 0, 1, 2, 5, 9], (n, a)).astype(np.int32)
    off = rng.choice([2, 2, 1, 0], (n, a)).astype(np.int32)
    mean = rng.uniform(-0.3, 0.3, (n, a)).astype(np.float32)                # (sizes up to a few hundred: some orders exceed what the account can pay)
    sigma = rng.uniform(0, 1, (n, a)).astype(np.float32)
    return cat, mean, sigma, price, off


@functools.lru_cache(maxsize=None)
def _streams(a=A, n_hist=4):
    """Six markets' streams, cut from an oracle random-agent run's decoded orders in that run's execution order (another seed per market), a mark behind every 4
    orders.  Computed once per (agents, history depth) (CPU only) and shared; never modified."""
    n, steps = len(LENGTHS), 70
    src = O.OracleEnv(_cfg(256, num_of_agents=a, n_hist=n_hist), n)
    src.reset(SEEDS)
    rng = np.random.default_rng(17)
    la, ex = [], []
    for t in range(steps):
        _, _, _, _, info = src.step(*_law(rng, n, a))
        la.append(info["lob_actions"].copy())
        ex.append(np.array([[src.trace[i].exec_order[j] for j in range(a)] for i in range(n)]))
    src.close()
    la, ex = np.stack(la), np.stack(ex)                                  # [T, n, A, 4], [T, n, A]
    out = []
    for i, want in enumerate(LENGTHS):
        st = OR.from_lob_actions(la[:, i], ex[:, i], mark_every=4)
        assert len(st) >= want, (i, len(st))
        out.append(tuple(st[:want]))
    return tuple(out)


def _play_hooks(env, market, stream):
    """the stream through the one-order hooks (HipEnv and OracleEnv share the call shapes)"""
    for m in stream:
        if m == OR.MARK:
            env.mark_to_mkt(market)
        else:
            tr, typ, side, size, price = m[:5]
            env.place_order(market, tr, typ, side, size, price if typ != K.T_MARKET else 1)


def _same_market(got, want, i, j=None, tag=""):
    j = i if j is None else j
    assert bytes(got.get_state(i)) == bytes(want.get_state(j)), (tag, i)
    for side in (0, 1):
        g, w = got.get_book(i, side), want.get_book(j, side)
        assert g.shape == w.shape and np.array_equal(g, w), (tag, i, side, g.shape, w.shape)


def _envs(cap, n=len(LENGTHS), oracle=True, **kw):
    from hip_env import HipEnv
    hip = HipEnv(_cfg(cap, **kw), n)
    ora = O.OracleEnv(_cfg(cap, **kw), n) if oracle else None
    seeds = SEEDS[:n] if n <= len(SEEDS) else np.arange(700, 700 + n, dtype=np.uint64)
    for e in (hip, ora):
        if e is not None:
            e.reset(seeds)
    return hip, ora


def _np(t):
    return t.cpu().numpy()


# The kernel's message stage lies in LDS behind CDA_WPB x lds_bytes_per_wave(num_agents, n_hist): 3 agents at depth 1 put it nearest, 16 agents at depth 16 farthest;
# the stream source is the same oracle recipe with that agent count.  (The first two rows are the module's A = 4 at the default depth.)
@pytest.mark.parametrize("cap,a,n_hist", [(256, A, 4), (512, A, 4)] + [(cap, a, h) for a in (3, 16) for h in (1, 16) for cap in (256, 512)],
                         ids=["256", "512"] + [f"{cap}-A{a}-h{h}" for a in (3, 16) for h in (1, 16) for cap in (256, 512)])
def test_a_stream_equals_the_hooks_and_the_oracle_at_the_chunk_edges(cap, a, n_hist):
    streams = _streams(a, n_hist)
    shape = {} if (a, n_hist) == (A, 4) else {"num_of_agents": a, "n_hist": n_hist}
    hip, ora = _envs(cap, **shape)
    hooks, _ = _envs(cap, oracle=False, **shape)
    assert hip.env.book_capacity == cap and hip.env.num_agents == a and hip.env.n_hist == n_hist
    empty_before = (bytes(hip.get_state(0)), hip.get_book(0, 0).tobytes(), hip.get_book(0, 1).tobytes(), hip.raw_snapshot()[0].tobytes())
    res, summary = hip.env.submit_orders([list(s) for s in streams])
    for i, st in enumerate(streams):
        _play_hooks(ora, i, st)
        _play_hooks(hooks, i, st)
    for i in range(len(streams)):
        _same_market(hip, ora, i, tag="oracle")
        _same_market(hip, hooks, i, tag="hooks")
    assert empty_before == (bytes(hip.get_state(0)), hip.get_book(0, 0).tobytes(), hip.get_book(0, 1).tobytes(), hip.raw_snapshot()[0].tobytes())
    assert np.array_equal(hip.raw_snapshot(), hooks.raw_snapshot())                   # (the level aggregation is recomputed from the same books)
    res, summary = _np(res).view(OR.RESULT_DTYPE).reshape(-1), _np(summary)
    assert len(res) == sum(LENGTHS) and summary.shape == (len(LENGTHS), 4)
    assert np.array_equal(summary[:, :3].sum(axis=1), np.array(LENGTHS)) and (summary[:, 2] == 0).all()
    # the streams exercise what they are meant to: fills, rejections, and every order type
    assert summary[:, 3].sum() > 20 and summary[:, 1].sum() > 0
    assert {m[1] for st in streams for m in st if m != OR.MARK} == {0, 1, 2, 3}
    assert (hip.flags() == 0).all() and (_np(hip.env.check_invariants()) == 0).all()
    hip.close(); hooks.close(); ora.close()


def test_a_stream_crosses_the_tile_and_the_ring():
    """tile 256: 300 bids at rising prices (each the new best: the OLDEST orders end up deepest, in the HBM ring), then a cancel, an in-place modify and a re-priced
    modify of orders that live in the ring, a limit sell that sweeps more than the tile holds in one message, and a mark; market 1 stops after 40 messages."""
    big = [(k % A, K.T_LIMIT, K.S_BID, 2 + k % 7, 9000 + k) for k in range(300)]
    big += [(2, K.T_CANCEL, K.S_BID, 1, 9002),                     # k = 2: in the ring
            (0, K.T_MODIFY, K.S_BID, 1, 9000),                     # trader 0's oldest (k = 0, price 9000, size 2): same price, smaller -> in place
            (1, K.T_MODIFY, K.S_BID, 3, 9500),                     # trader 1's oldest (k = 1, price 9001) moves to 9500
            (3, K.T_LIMIT, K.S_ASK, 5000, 9020),                   # sweeps every bid >= 9020 (about 280 orders) and rests
            OR.MARK]
    streams = [big, big[:40]]
    hip, ora = _envs(256, n=2, init_cash=10 ** 12)
    _, summary = hip.env.submit_orders(streams, results=False)
    for i, st in enumerate(streams):
        _play_hooks(ora, i, st)
    for i in range(2):
        _same_market(hip, ora, i)
    s0 = hip.get_state(0)
    assert np.array_equal(_np(hip.env.book_peak()), ora.book_peak()) and _np(hip.env.book_peak())[0] == 300
    assert s0.n_asks == 1 and 0 < s0.n_bids < 25 and hip.get_state(1).n_bids == 40
    assert _np(summary).tolist() == [[305, 0, 0, _np(summary)[0, 3]], [40, 0, 0, 0]] and _np(summary)[0, 3] > 256
    assert (hip.flags() == 0).all() and (_np(hip.env.check_invariants()) == 0).all()
    hip.close(); ora.close()


def test_result_records_equal_the_specification():
    """the 65-message market: every result record against orders.expected_results, fed from a hook-by-hook replay on a tape-enabled twin"""
    streams = _streams()
    mkt = LENGTHS.index(65)
    hip, _ = _envs(256, oracle=False)
    res, summary = hip.env.submit_orders([list(s) for s in streams])
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    res = _np(res).view(OR.RESULT_DTYPE).reshape(-1)
    twin, _ = _envs(256, oracle=False)
    twin.env.enable_tape(1024)
    _, msgs = OR.pack([list(streams[mkt])])
    assert OR.check(msgs, A) == -1

    def snap():
        return twin.get_state(mkt), int(twin.env.tape_counts()["n_total"][mkt].item()), int(_np(twin.env.book_counts(mkt, 1))[0, :, 0].sum())

    snaps = [snap()]
    for m in streams[mkt]:
        _play_hooks(twin, mkt, [m])
        snaps.append(snap())
    want = OR.expected_results(msgs, A, [s[0] for s in snaps], [s[1] for s in snaps], [s[2] for s in snaps])
    got = res[off[mkt]:off[mkt + 1]]
    for f in OR.RESULT_DTYPE.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (f, bad[:8], got[bad[:4]], want[bad[:4]])
    assert (want["n_fills"] > 0).any() and (want["resting_delta"] < 0).any() and (want["resting_delta"] > 0).any() and (want["position_delta"] != 0).any()
    summary = _np(summary)
    for i in range(len(LENGTHS)):
        assert np.array_equal(summary[i], OR.summary_of(res[off[i]:off[i + 1]])), i
    hip.close(); twin.close()


def test_invalid_messages_are_skipped_and_reported():
    good = list(_streams()[LENGTHS.index(63)])[:30]
    bad = [(A, 1, 0, 5, 50, 0), (0, 5, 0, 5, 50, 0), (0, 1, 2, 5, 50, 0), (0, 1, 0, 0, 50, 0), (0, 1, 0, 5, 0, 0)]     # trader = A, type 5, side 2, size 0, price 0 on a limit
    mixed = list(good)
    for pos, b in sorted(zip([3, 9, 10, 17, 29], bad), reverse=True):
        mixed.insert(pos, b)
    bad_idx = [i for i, m in enumerate(mixed) if m in bad]
    assert len(bad_idx) == 5 and len(mixed) == 35
    hip, _ = _envs(256, n=1, oracle=False)
    ref, ora = _envs(256, n=1)
    res, summary = hip.env.submit_orders([mixed])
    res_ref, summary_ref = ref.env.submit_orders([good])
    _play_hooks(ora, 0, good)
    _same_market(hip, ref, 0, tag="without them")
    _same_market(hip, ora, 0, tag="oracle")
    res, res_ref = _np(res).view(OR.RESULT_DTYPE).reshape(-1), _np(res_ref).view(OR.RESULT_DTYPE).reshape(-1)
    assert (res[bad_idx]["status"] == OR.ORD_INVALID).all()
    for f in ("n_fills", "position_delta", "resting_delta"):
        assert (res[bad_idx][f] == 0).all(), f
    keep = np.setdiff1d(np.arange(len(mixed)), bad_idx)
    assert res[keep].tobytes() == res_ref.tobytes() and (res_ref["status"] != OR.ORD_INVALID).all()
    summary, summary_ref = _np(summary), _np(summary_ref)
    assert summary[0, 2] == 5 and summary_ref[0, 2] == 0 and np.array_equal(summary[0, [0, 1, 3]], summary_ref[0, [0, 1, 3]])
    # the two host statements of the rule name the same first bad message
    _, msgs = OR.pack([mixed])
    from gym_continuousdoubleauction_amd._lib import lib
    for start in [0] + [i + 1 for i in bad_idx]:
        first_bad = C.c_int64(-7)
        tail = np.ascontiguousarray(msgs[start:])
        assert lib().cda_order_msgs_check_host(hip.env._h, tail.ctypes.data, len(tail), C.byref(first_bad)) == 0
        assert first_bad.value == OR.check(tail, A), start
    assert OR.check(msgs, A) == bad_idx[0] == 3
    hip.close(); ref.close(); ora.close()


def _tape_fixture(name):
    with np.load(os.path.join(G.GOLD, f"tape_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_tape_holds_what_the_hooks_would_have_written():
    """the decoded orders of the first steps of a committed trace, in the trace's execution order, a mark behind every step: ONE stream on a tape-enabled env writes
    the reference's own tape (tests/golden/tape_aggr_s23.npz: every field but the step index - no env step is taken), as the hook sequence does"""
    from hip_env import HipEnv
    name, steps = "aggr_s23", 48
    r, fx = G.load(name), _tape_fixture(name)
    stream = []
    for t in range(steps):
        for tr in r["exec_order"][t][: int(r["n_acts"][t])]:
            tr = int(tr)
            typ, side, size, price = (int(r[k][t, tr]) for k in ("dec_type", "dec_side", "dec_size", "dec_price"))
            stream.append((tr, typ, side, size, price if typ != 0 else 0))
        stream.append(OR.MARK)
    envs = []
    for _ in range(2):
        e = HipEnv(r["config"], n_markets=1)
        e.env.enable_tape(1024)
        e.reset(np.array([int(r["seed"])], np.uint64))
        envs.append(e)
    env, hooks = envs
    res, summary = env.env.submit_orders([stream])
    _play_hooks(hooks, 0, stream)
    n_fills = int(fx["tape_len"][steps - 1])
    assert n_fills > 40
    counts, counts_h = ({k: _np(v) for k, v in e.env.tape_counts().items()} for e in (env, hooks))
    for k in counts:
        assert np.array_equal(counts[k], counts_h[k]), k
    assert int(counts["n_episode"][0]) == n_fills == int(_np(summary)[0, 3]) == int(_np(res)[:, 1].sum())
    rows, rows_h = _np(env.env.drain_tape()[0]), _np(hooks.env.drain_tape()[0])
    want = fx["rows"][:n_fills].copy()
    want[:, 7] &= 3
    for j, f in enumerate(("time", "price", "quantity", "counter_id", "counter_order_id", "counter_left", "init_id", "sides_step")):
        assert np.array_equal(rows[:, j], want[:, j]), f
        assert np.array_equal(rows[:, j], rows_h[:, j]), f
    _same_market(env, hooks, 0)
    env.close(); hooks.close()


INFO_KEYS = ("num_trades", "net_position", "num_trades_step", "num_passive_fills_step", "order_step_placed", "num_rejected_step", "lob_actions", "is_pass_action")


@pytest.mark.parametrize("cap", [256, 512])
@pytest.mark.parametrize("clear", [True, False])
def test_the_next_step_sees_the_book_and_the_cleared_counters(cap, clear):
    streams = _streams()
    hip, ora = _envs(cap)
    hip.env.submit_orders([list(s) for s in streams], clear_step_counters=clear, results=False)
    touched = 0
    for i, st in enumerate(streams):
        _play_hooks(ora, i, st)
        s = ora.get_state(i)
        touched += sum(getattr(s.acc[a], k) for a in range(A) for k in COUNTERS)
        if clear:
            for a in range(A):
                for k in COUNTERS:
                    setattr(s.acc[a], k, 0)
            ora.set_state(i, s)
    assert touched > 50                                                                # the flag has something to clear
    for i in range(len(streams)):
        _same_market(hip, ora, i, tag="before the step")
    acts = _law(np.random.default_rng(23), len(streams), A)
    ho, hr, ht, htr, hi = hip.step(*acts)
    oo, orw, ot, otr, oi = ora.step(*acts)
    assert np.array_equal(ho.view(np.uint32), oo.view(np.uint32)), np.nonzero((ho != oo).any(axis=1))[0]
    assert np.array_equal(hr.view(np.uint64), orw.view(np.uint64))
    assert np.array_equal(ht, ot) and np.array_equal(htr, otr)
    for k in INFO_KEYS:
        assert np.array_equal(hi[k], oi[k]), k
    assert np.array_equal(hi["nav"].view(np.uint8), oi["nav"].view(np.uint8))
    assert np.array_equal(hi["reward_terms"].view(np.uint64), oi["reward_terms"].view(np.uint64))
    for i in range(len(streams)):
        _same_market(hip, ora, i, tag="after the step")
    hip.close(); ora.close()


def test_ranges_splitting_and_a_side_stream():
    streams = [list(s) for s in _streams()]
    sub = [streams[5], streams[3], streams[4]]                                         # markets 2, 3, 4 get 130, 64 and 65 messages
    hip, ora = _envs(256)
    before = {i: (bytes(hip.get_state(i)), hip.get_book(i, 0).tobytes(), hip.get_book(i, 1).tobytes()) for i in (0, 1, 5)}
    res, summary = hip.env.submit_orders(sub, first_market=2, n_markets=3)
    for j, st in enumerate(sub):
        _play_hooks(ora, 2 + j, st)
        _same_market(hip, ora, 2 + j, tag="range")
    for i in (0, 1, 5):
        assert before[i] == (bytes(hip.get_state(i)), hip.get_book(i, 0).tobytes(), hip.get_book(i, 1).tobytes()), i
    assert _np(summary)[:, :3].sum(axis=1).tolist() == [130, 64, 65]
    # successive launches of at most 16 messages per market: the same state, the same results
    split, _ = _envs(256, oracle=False)
    res_s, summary_s = split.env.submit_orders(sub, first_market=2, n_markets=3, max_per_launch=16)
    for i in range(len(LENGTHS)):
        _same_market(split, hip, i, tag="split")
    assert np.array_equal(_np(res_s), _np(res)) and np.array_equal(_np(summary_s), _np(summary))
    split.close()
    # the same call on a side stream, a step behind it on that stream, no host synchronisation in between
    acts = _law(np.random.default_rng(29), len(LENGTHS), A)
    ho, hr, *_ = hip.step(*acts)
    side, _ = _envs(256, oracle=False)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res_a, summary_a = side.env.submit_orders(sub, first_market=2, n_markets=3)
        obs, rew, _, _, _ = side.env.step(*acts)
    s.synchronize()
    assert np.array_equal(_np(obs).view(np.uint32), ho.view(np.uint32)) and np.array_equal(_np(rew).view(np.uint64), hr.view(np.uint64))
    assert np.array_equal(_np(res_a), _np(res)) and np.array_equal(_np(summary_a), _np(summary))
    for i in range(len(LENGTHS)):
        _same_market(side, hip, i, tag="side stream")
    # offsets that are no stream: that market runs nothing and says so
    off, msgs = OR.pack(sub)
    off[2] = off[1] - 1
    bad, _ = _envs(256, oracle=False)
    fresh = bytes(bad.get_state(3))
    _, summary_b = bad.env.submit_orders(offsets=off, msgs=msgs, first_market=2, n_markets=3, results=False, max_len=130)
    assert _np(summary_b)[1].tolist() == [0, 0, -1, 0] and bytes(bad.get_state(3)) == fresh
    side.close(); bad.close(); hip.close(); ora.close()


def test_seed_books_rebuilds_a_dumped_book_in_every_market():
    from hip_env import HipEnv
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 256, "is_render": False}
    src = HipEnv(cfg, 1)
    src.reset(np.array([5], np.uint64))
    src.env.run_random(30, action_seed=41)
    bids, asks = src.get_book(0)
    assert len(bids) >= 5 and len(asks) >= 5
    src.close()
    n = 8
    hip = HipEnv(cfg, n)
    hip.reset(np.arange(900, 900 + n, dtype=np.uint64))
    res, summary = hip.env.seed_books(bids, asks)
    assert _np(summary).tolist() == [[len(bids) + len(asks), 0, 0, 0]] * n
    for i in range(n):
        b, a = hip.get_book(i)
        assert np.array_equal(b[:, :3], bids[:, :3]) and np.array_equal(a[:, :3], asks[:, :3]), i
        s = hip.get_state(i)
        assert all(getattr(s.acc[j], k) == 0 for j in range(A) for k in COUNTERS), i
    assert (_np(hip.env.check_invariants()) == 0).all() and (hip.flags() == 0).all()
    one = HipEnv(cfg, 3)
    one.reset(np.arange(3, dtype=np.uint64))
    one.env.seed_books(bids, asks, market=1)
    assert np.array_equal(one.get_book(1, 0)[:, :3], bids[:, :3]) and one.get_state(0).n_bids == 0 and one.get_state(2).n_asks == 0
    hip.close(); one.close()
