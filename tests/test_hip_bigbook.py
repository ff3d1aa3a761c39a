"""GPU parity of the book's HBM tier (csrc/cda_book.inc, "The HBM tier of the book"): the reference's OrderTree is unbounded
(orderbook/ordertree.py:5-58) and a limit order that does not cross always rests (orderbook.py:162-194), so the product keeps the
top of a market's book in its LDS tile and everything behind it in an HBM spill ring.  These tests drive books FAR beyond the
tile - through the C-ABI, like every GPU test - and compare with the unbounded CPU oracle order for order; the golden replays of
the reference's own big books (trace_bigbook_*) run in tests/test_hip_golden.py with all the other traces."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from gym_continuousdoubleauction_amd import _capi as K

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


def _trend(rng, n, a, t, waves):
    """the "trend" / "trend_waves" laws of tests/golden/make_goldens.py, batched"""
    cat = rng.choice([2, 2, 2, 2, 2, 6, 6, 6, 1, 1, 1, 5, 3, 7, 4, 8, 0], (n, a)).astype(np.int32)
    if waves and (t // waves) % 2 == 1:
        cat = np.where(cat == 0, 0, np.where(cat <= 4, cat + 4, cat - 4)).astype(np.int32)
    price = rng.choice([0, 0, 0, 1, 2, 5, 9], (n, a)).astype(np.int32)
    off = rng.choice([2, 2, 1, 0], (n, a)).astype(np.int32)
    mean = rng.uniform(-0.004, 0.004, (n, a)).astype(np.float32)
    sigma = rng.uniform(0, 1, (n, a)).astype(np.float32)
    return cat, mean, sigma, price, off


def _same_books(hip, ora, markets):
    for i in markets:
        for side in (0, 1):
            g, w = hip.get_book(i, side), ora.get_book(i, side)
            assert g.shape == w.shape and np.array_equal(g, w), (i, side, g.shape, w.shape)


@pytest.mark.parametrize("agents,waves,steps", [(4, 0, 900), (8, 300, 900), (16, 0, 700), (16, 320, 960)])
def test_books_far_beyond_the_tile_equal_the_unbounded_oracle(agents, waves, steps):
    from hip_env import HipEnv
    n = 24
    cfg = {"num_of_agents": agents, "init_cash": 1000000, "max_step": steps, "is_render": False}
    hip, ora = HipEnv(cfg, n), O.OracleEnv(cfg, n)
    tile = hip.env.book_capacity
    assert hip.env.book_spill >= agents * steps            # automatic: a side cannot outgrow it inside an episode
    seeds = np.arange(300, 300 + n, dtype=np.uint64)
    assert np.array_equal(hip.reset(seeds), ora.reset(seeds))
    rng = np.random.default_rng(11 + agents)
    for t in range(steps):
        acts = _trend(rng, n, agents, t, waves)
        ho, hr, ht, htr, hi = hip.step(*acts)
        oo, orw, ot, otr, oi = ora.step(*acts)
        assert np.array_equal(ho.view(np.uint32), oo.view(np.uint32)), f"obs, step {t}: markets {np.nonzero((ho != oo).any(axis=1))[0][:8]}"
        assert np.array_equal(hr.view(np.uint64), orw.view(np.uint64)), f"reward, step {t}"
        assert np.array_equal(ht, ot) and np.array_equal(htr, otr)
        for k in ("num_trades", "net_position", "num_trades_step", "num_passive_fills_step", "order_step_placed", "num_rejected_step", "lob_actions"):
            assert np.array_equal(hi[k], oi[k]), (k, t)
        assert np.array_equal(hi["nav"].view(np.uint8), oi["nav"].view(np.uint8)), f"NAV, step {t}"
        if t % 150 == 149:
            _same_books(hip, ora, range(0, n, 5))
    peak = hip.env.book_peak().cpu().numpy()
    assert np.array_equal(peak, ora.book_peak()) and peak.max() > tile, (peak.max(), tile)
    assert (hip.flags() == 0).all() and (ora.flags() == 0).all()
    assert (hip.env.check_invariants().cpu().numpy() == 0).all()
    _same_books(hip, ora, range(n))
    for i in range(n):
        sg, so = hip.get_state(i), ora.get_state(i)
        assert bytes(sg) == bytes(so), i
    hip.close(); ora.close()


def test_deep_orders_are_found_modified_and_cancelled_where_they_lie():
    """One market, built order by order through the place_order hook (Trader.place_order, trader.py:49-106): 700 resting bids and
    500 resting asks at distinct prices (tile: 256), then cancels, in-place and moving modifies and upserts aimed at orders deep in
    the HBM tail, sweeps that consume the tile and refill it, and inserts at every depth - the oracle must agree after each."""
    from hip_env import HipEnv
    cfg = {"num_of_agents": 4, "init_cash": 10 ** 12, "max_step": 64, "is_render": False}
    hip, ora = HipEnv(cfg, 1), O.OracleEnv(cfg, 1)
    both = (hip, ora)
    for e in both:
        e.reset(np.array([5], np.uint64))
    rng = np.random.default_rng(3)

    def do(tr, typ, side, size, price):
        for e in both:
            e.place_order(0, tr, typ, side, size, price)

    def same(tag):
        _same_books(hip, ora, [0])
        assert bytes(hip.get_state(0)) == bytes(ora.get_state(0)), tag
        assert hip.flags()[0] == 0

    for k in range(700):                                                      # bids 10000, 9999, ... (best first)
        do(k % 4, K.T_LIMIT, K.S_BID, 1 + k % 7, 10000 - k)
    for k in range(500):
        do((k + 1) % 4, K.T_LIMIT, K.S_ASK, 1 + k % 5, 10100 + k)
    same("built")
    assert hip.get_state(0).n_bids == 700 and hip.get_state(0).n_asks == 500
    for k in rng.permutation(700)[:60]:                                       # cancels at every depth (Trader._cancel_limit_order)
        do(int(k) % 4, K.T_CANCEL, K.S_BID, 1, 10000 - int(k))
    same("cancels")
    for k in rng.permutation(500)[:40]:                                       # upserts: same price, smaller (in place) or larger (re-queued) size
        do((int(k) + 1) % 4, K.T_LIMIT, K.S_ASK, int(rng.integers(1, 9)), 10100 + int(k))
    same("upserts")
    for j in range(30):                                                       # modify = the trader's OLDEST order moves (it lies deep)
        do(j % 4, K.T_MODIFY, K.S_BID, 3, 10000 - int(rng.integers(0, 900)))
        do(j % 4, K.T_MODIFY, K.S_ASK, 2, 10100 + int(rng.integers(0, 700)))
    same("modifies")
    for j in range(12):                                                       # sweeps through tile and tail, then new orders behind them
        do(j % 4, K.T_MARKET, K.S_ASK, 90 + 40 * j, 1)
        do((j + 1) % 4, K.T_LIMIT, K.S_BID, 5, 9000 + 13 * j)
        do((j + 2) % 4, K.T_MARKET, K.S_BID, 70 + 30 * j, 1)
        same(f"sweep {j}")
    for j in range(40):                                                       # inserts at random depths, both sides, equal prices included
        do(j % 4, K.T_LIMIT, K.S_BID, 2, int(rng.integers(8800, 9900)))
        do((j + 3) % 4, K.T_LIMIT, K.S_ASK, 2, int(rng.integers(10200, 10900)))
    same("inserts")
    do(0, K.T_LIMIT, K.S_BID, 10 ** 6, 11000)                                 # a crossing limit order that eats EVERY ask and rests
    same("sweep of a whole side")
    assert hip.get_state(0).n_asks == 0
    assert (hip.env.check_invariants().cpu().numpy() == 0).all()
    hip.close(); ora.close()


def test_restored_big_book_and_fused_episodes():
    """cda_set_state splits a restored book between tile and ring; cda_run_random (whole episodes in one launch) then plays on
    top of 2 x 400 far-away resting orders per market - tile evictions, refills and level aggregation across the tile's end
    inside the fused loop - and equals the oracle's run on the same stream."""
    from hip_env import HipEnv
    n, a = 12, 8
    cfg = {"num_of_agents": a, "init_cash": 10 ** 9, "max_step": 4000, "is_render": False, "initial_price_min": 5000, "initial_price_max": 6000}
    hip, ora = HipEnv(cfg, n), O.OracleEnv(cfg, n)
    seeds = np.arange(40, 40 + n, dtype=np.uint64)
    hip.reset(seeds); ora.reset(seeds)
    for e in (hip, ora):
        for i in range(n):
            s = e.get_state(i)
            lp = s.last_price
            s.n_bids = s.n_asks = 400
            for k in range(400):
                b, q = s.bids[k], s.asks[k]
                # levels of four orders each, away from the touch on both sides; the accounts below carry the matching escrow
                b.price, b.qty, b.owner, b.order_id, b.timestamp = max(1, lp - 1 - k // 4), 1 + k % 3, k % a, 2 * k + 1, 2 * k + 1
                q.price, q.qty, q.owner, q.order_id, q.timestamp = lp + 1 + k // 4, 1 + k % 3, (k + 3) % a, 2 * k + 2, 2 * k + 2
            s.lob_time = s.next_order_id = 800
            hold = [0] * a
            for k in range(400):
                hold[k % a] += s.bids[k].price * s.bids[k].qty
                hold[(k + 3) % a] += s.asks[k].price * s.asks[k].qty
            from decimal import Decimal
            for j in range(a):
                s.acc[j].cash_on_hold = K.decimal_to_dec(Decimal(hold[j]) * Decimal("1.0"))
                s.acc[j].cash = K.decimal_to_dec(Decimal(10 ** 9 - hold[j]) * Decimal("1.0"))
            e.set_state(i, s)
    _same_books(hip, ora, range(n))
    assert (hip.env.check_invariants().cpu().numpy() == 0).all()
    obs, ret, term, trunc, steps = hip.env.run_random(300, action_seed=77)
    ora.run_random(0, 300, action_seed=77)
    assert np.array_equal(obs.cpu().numpy().view(np.uint32), ora.obs.view(np.uint32))
    _same_books(hip, ora, range(n))
    for i in range(n):
        assert bytes(hip.get_state(i)) == bytes(ora.get_state(i)), i
    assert (hip.flags() == 0).all() and (hip.env.check_invariants().cpu().numpy() == 0).all()
    # ... and the per-step path continues from there
    rng = np.random.default_rng(9)
    for t in range(120):
        acts = _trend(rng, n, a, t, 60)
        ho, hr, *_ = hip.step(*acts)
        oo, orw, *_ = ora.step(*acts)
        assert np.array_equal(ho.view(np.uint32), oo.view(np.uint32)) and np.array_equal(hr.view(np.uint64), orw.view(np.uint64)), t
    _same_books(hip, ora, range(n))
    hip.close(); ora.close()


def test_a_full_ring_is_flagged_never_silent():
    """book_spill = 64: tile (256) + ring (64 per side) is all a market holds; what fits neither is dropped and the market flagged
    (CDA_FLAG_BOOK_OVERFLOW) - and the book that is there stays consistent."""
    from hip_env import HipEnv
    cfg = {"num_of_agents": 4, "init_cash": 10 ** 12, "max_step": 64, "is_render": False, "book_spill": 64}
    hip = HipEnv(cfg, 1)
    assert hip.env.book_spill == 64 and hip.env.book_capacity == 256
    hip.reset(np.array([1], np.uint64))
    for k in range(400):
        hip.place_order(0, k % 4, K.T_LIMIT, K.S_BID, 1, 10000 - k)
    st = hip.get_state(0)
    assert hip.flags()[0] & K.FLAG_BOOK_OVERFLOW
    assert 256 <= st.n_bids <= 256 + 64 and st.n_asks == 0
    inv = int(hip.env.check_invariants().cpu().numpy()[0])
    assert inv == 0, inv                  # sorted, uncrossed, positive - and the escrow of a dropped order was never taken
    hip.close()
    # an env WITHOUT the tier drops at the tile (the round-2 behaviour), an automatic one never does
    none, auto = HipEnv(dict(cfg, book_spill=-1), 1), HipEnv(dict(cfg, book_spill=0), 1)
    assert none.env.book_spill == 0 and auto.env.book_spill >= 1024
    for e in (none, auto):
        e.reset(np.array([1], np.uint64))
        for k in range(300):
            e.place_order(0, k % 4, K.T_LIMIT, K.S_BID, 1, 10000 - k)
    assert none.flags()[0] & K.FLAG_BOOK_OVERFLOW and none.get_state(0).n_bids == 256
    assert auto.flags()[0] == 0 and auto.get_state(0).n_bids == 300
    none.close(); auto.close()


# ---- the host's view of a record (cda_get_book, cda_get_state, cda_set_state) on a ring whose base has moved ------------------------------------
_RING_CFG = {"num_of_agents": 2, "init_cash": 10 ** 12, "max_step": 64, "is_render": False, "book_spill": 64}


def _ring_market(with_oracle=True):
    """1 market, 2 agents, tile 256, ring 64.  280 resting bids at falling prices fill the tile and start the tail behind it (ring base 0); a bid
    above all of them then enters a full tile, whose last 32 orders are PREPENDED to the tail (tile_push_to_tail: base - 32, slots that wrap around the
    ring's end); a market sell takes the top few.  The side: 225 - few orders in the tile, 56 in a ring that starts at slot 32 of 64."""
    from hip_env import HipEnv
    envs = [HipEnv(_RING_CFG, 1)] + ([O.OracleEnv(_RING_CFG, 1)] if with_oracle else [])
    assert envs[0].env.book_spill == 64 and envs[0].env.book_capacity == 256
    for e in envs:
        e.reset(np.array([7], np.uint64))
        for k in range(280):
            e.place_order(0, k % 2, K.T_LIMIT, K.S_BID, 1 + k % 7, 10000 - k)
        e.place_order(0, 1, K.T_LIMIT, K.S_BID, 3, 10001)
        e.place_order(0, 0, K.T_MARKET, K.S_ASK, 3 + 1 + 2 + 3 + 2, 1)          # the orders at 10001 .. 9998 and part of the one at 9997
    assert envs[0].flags()[0] == 0
    return envs


def _raw_get_book(hip, side, max_orders):
    import ctypes as C
    from gym_continuousdoubleauction_amd._lib import lib
    n = C.c_int32(-1)
    buf = (K.Order * max(max_orders, 1))()
    rc = lib().cda_get_book(hip.env._h, 0, side, C.cast(buf, C.c_void_p) if max_orders else None, max_orders, C.byref(n))
    assert rc == 0, rc
    return np.ctypeslib.as_array(buf).view(np.int32).reshape(-1, 5)[:min(max_orders, n.value)].copy(), n.value


def test_get_book_prefixes_on_a_ring_whose_base_has_moved():
    hip, ora = _ring_market()
    want = ora.get_book(0, K.S_BID)
    total = len(want)
    assert total == 281 - 4 and len(ora.get_book(0, K.S_ASK)) == 0
    # nothing; inside the tile; one short of the tile's least (221) and most (256) possible count; between tile and total; the total; more than there is
    for m in (0, 1, 10, 220, 257, total - 30, total - 1, total, total + 9):
        got, n = _raw_get_book(hip, K.S_BID, m)
        assert n == total, (m, n)
        assert got.shape == want[:m].shape and np.array_equal(got, want[:m]), m
    assert _raw_get_book(hip, K.S_ASK, 5)[1] == 0
    assert (hip.env.check_invariants().cpu().numpy() == 0).all()
    hip.close(); ora.close()


def test_a_refused_set_state_changes_nothing():
    import ctypes as C
    from gym_continuousdoubleauction_amd._lib import lib
    (hip,) = _ring_market(with_oracle=False)
    before = bytes(hip.get_state(0))

    def state(n_bids, bad_owner_at):
        s = hip.get_state(0)
        s.n_bids, s.n_asks = n_bids, 0
        for k in range(n_bids):
            b = s.bids[k]
            b.price, b.qty, b.owner, b.order_id, b.timestamp = 20000 - k, 1, k % 2, k + 1, k + 1
        if bad_owner_at is not None:
            s.bids[bad_owner_at].owner = 2                                    # two agents: owners 0 and 1
        return s

    cases = {"owner out of range in the tile part": state(10, 3),
             "owner out of range in the ring part": state(300, 290),          # 256 in the tile, 44 in the ring
             "a tail longer than the ring": state(400, None)}                 # 256 in the tile, 144 > 64 behind it
    for tag, s in cases.items():
        assert lib().cda_set_state(hip.env._h, 0, C.byref(s)) == K.ERR_INVALID, tag
        assert bytes(hip.get_state(0)) == before, tag
        assert (hip.env.check_invariants().cpu().numpy() == 0).all(), tag
    hip.close()


def test_get_state_set_state_is_the_identity_on_a_moved_ring():
    hip, ora = _ring_market()
    s0 = hip.get_state(0)
    assert bytes(s0) == bytes(ora.get_state(0))
    hip.set_state(0, s0)                                                      # (re-split: 256 in the tile, the rest in a ring that starts at slot 0 again)
    assert bytes(hip.get_state(0)) == bytes(s0)
    _same_books(hip, ora, [0])
    assert (hip.env.check_invariants().cpu().numpy() == 0).all()
    acts = _trend(np.random.default_rng(5), 1, 2, 0, 0)
    ho, hr, ht, htr, _ = hip.step(*acts)
    oo, orw, ot, otr, _ = ora.step(*acts)
    assert np.array_equal(ho.view(np.uint32), oo.view(np.uint32)) and np.array_equal(hr.view(np.uint64), orw.view(np.uint64))
    assert np.array_equal(ht, ot) and np.array_equal(htr, otr)
    _same_books(hip, ora, [0])
    assert bytes(hip.get_state(0)) == bytes(ora.get_state(0))
    assert hip.flags()[0] == 0 and (hip.env.check_invariants().cpu().numpy() == 0).all()
    hip.close(); ora.close()
