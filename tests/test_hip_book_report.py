"""GPU parity of the book report (csrc/cda_book_report.inc; CDAVecEnv.book_counts / book_levels / book_impact / book_agents / book_orders).  Every reader is
compared three ways: against the specification (gym_continuousdoubleauction_amd/book.py) applied to the device's own get_book(), against the specification applied
to the CPU oracle's get_book() for the same orders, and book_orders() row for row against both.  The shapes are the smallest at which the walk - 64 orders per
pass, a carry from pass to pass, the tile and then the ring - can go wrong."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from gym_continuousdoubleauction_amd import _capi as K
from gym_continuousdoubleauction_amd import book as B

pytestmark = pytest.mark.gpu

RICH = 10 ** 12
SIZES = (1, 2, 7, 33, 150, 10 ** 6)


def _pair(cfg, n):
    from hip_env import HipEnv
    hip, ora = HipEnv(cfg, n), O.OracleEnv(cfg, n)
    seeds = np.arange(500, 500 + n, dtype=np.uint64)
    assert np.array_equal(hip.reset(seeds), ora.reset(seeds))
    return hip, ora


def _device_report(env, levels, sizes, first=0, n=None):
    rows, off = env.book_orders(first, n)
    out = {"counts": env.book_counts(first, n), "levels": env.book_levels(levels, first, n), "impact": env.book_impact(sizes, first, n),
           "agents": env.book_agents(first, n), "orders": rows, "offsets": off}
    assert out["counts"].dtype == torch.int32 and out["orders"].dtype == torch.int32 and all(out[k].dtype == torch.int64 for k in ("levels", "impact", "agents", "offsets"))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, tag):
    for k in ("counts", "levels", "impact", "agents", "offsets", "orders"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k, np.argwhere(got[k] != want[k])[:4] if got[k].shape == want[k].shape else (got[k].shape, want[k].shape))


def check(hip, ora, levels=12, sizes=SIZES, first=0, n=None, tag=""):
    """the three-way comparison for markets [first, first + n); returns the device's report"""
    n = hip.n - first if n is None else n
    got = _device_report(hip.env, levels, sizes, first, n)
    for who, e in (("own get_book", hip), ("oracle", ora)):
        _same(got, B.report_from_books([e.get_book(i) for i in range(first, first + n)], hip.A, levels, sizes), (tag, who))
    return got


def _boundary_sizes(side):
    """[1, exact boundary, boundary + 1, total, total + 1] at the first order's end and at the end of the first pass of 64 orders"""
    cq = np.cumsum(side[:, 1].astype(np.int64))
    picks = {1}
    if len(cq):
        for b in (cq[0], cq[min(63, len(cq) - 1)], cq[-1]):
            picks |= {int(b), int(b) + 1}
    return sorted(picks)


def _ring_meta(env, market):
    """(tail orders per side, ring base per side) of one market, read from a snapshot's section (csrc/cda_snapshot.inc SnapMeta behind the record)"""
    blob = env.snapshot(market, 1).blob.cpu().numpy()
    at = int(blob[256:264].view(np.int64)[0]) + env.state_bytes_per_market()
    meta = blob[at:at + 32].view(np.int32)
    return (int(meta[2]), int(meta[3])), (int(meta[4]), int(meta[5]))


def test_chunk_edges():
    """Books built order by order: an empty side, one order, 64 and 65 orders at one price (a level that ends at / crosses the end of the first pass), 63 + 2,
    130 distinct prices, sixteen agents whose orders interleave.  A trader's second limit order at a price it already quotes replaces the first
    (trader.py:189-235), so a level of more than sixteen orders is built by MODIFY: it moves the trader's oldest order to the level's tail."""
    A = 16
    hip, ora = _pair({"num_of_agents": A, "init_cash": RICH, "max_step": 64, "is_render": False}, 4)

    def do(m, tr, typ, side, size, price):
        for e in (hip, ora):
            e.place_order(m, tr, typ, side, size, price)

    def one_level(m, side, count, price, park):
        for k in range(count):                                       # distinct parking prices first, worse than `price` ...
            do(m, k % A, K.T_LIMIT, side, 1 + k % 5, park - k if side == K.S_BID else park + k)
        for k in range(count):                                       # ... then every trader's oldest order, one after the other, joins the level
            do(m, k % A, K.T_MODIFY, side, 1 + k % 5, price)

    check(hip, ora, tag="all empty")
    do(0, 3, K.T_LIMIT, K.S_ASK, 7, 10100)                           # market 0: no bids, one ask
    one_level(1, K.S_BID, 64, 9500, 9000)                            # market 1: 64 bids and 65 asks at one price each
    one_level(1, K.S_ASK, 65, 10500, 11000)
    one_level(2, K.S_BID, 63, 9500, 9000)                            # market 2: 63 + 2 bids, 130 asks at distinct prices
    do(2, 0, K.T_LIMIT, K.S_BID, 4, 9499); do(2, 1, K.T_LIMIT, K.S_BID, 2, 9499)
    for k in range(130):
        do(2, k % A, K.T_LIMIT, K.S_ASK, 1 + k % 3, 10100 + k)
    for k in range(100):                                             # market 3: levels of sixteen / five orders, every agent in turn
        do(3, k % A, K.T_LIMIT, K.S_BID, 1 + k % 4, 9900 - k // A)
    for k in range(70):
        do(3, (k * 7) % A, K.T_LIMIT, K.S_ASK, 2 + k % 3, 10100 + k // 5)
    got = check(hip, ora, tag="built")
    assert got["counts"].tolist() == [[[0, 0], [1, 1]], [[64, 1], [65, 1]], [[65, 2], [130, 130]], [[100, 7], [70, 14]]]
    for L in (1, 2, 129, 130, 131):                                  # fewer rows than levels, exactly as many, more
        check(hip, ora, levels=L, tag=f"L={L}")
    for m in range(4):
        for s in (0, 1):
            check(hip, ora, levels=3, sizes=_boundary_sizes(ora.get_book(m, s)), first=m, n=1, tag=f"sizes of market {m} side {s}")
    assert (hip.flags() == 0).all() and (hip.env.check_invariants().cpu().numpy() == 0).all()
    # the range checks that need an env: a range outside it is refused, nothing is launched
    from gym_continuousdoubleauction_amd._lib import lib
    buf = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    for first, n in ((0, 5), (4, 1), (3, 2)):
        assert lib().cda_book_counts(hip.env._h, first, n, buf.data_ptr(), None) == K.ERR_INVALID
        assert lib().cda_book_offsets(hip.env._h, first, n, buf.data_ptr(), None) == K.ERR_INVALID
    with pytest.raises(ValueError):
        hip.env.book_levels(4097)
    with pytest.raises(ValueError):
        hip.env.book_impact([3, 0])
    with pytest.raises(ValueError):
        hip.env.book_agents(2, 3)
    hip.close(); ora.close()


@pytest.mark.parametrize("tile,per_side", [(256, 300), (512, 600)])
def test_tile_to_ring(tile, per_side):
    """Both sides pushed past their share of the tile: levels of one to sixteen orders, so that the tile's end falls inside a level (asserted from the
    ring counts a snapshot reports); ladders shorter and longer than the level count; sizes that end in the tile, at its end and in the ring."""
    A = 16
    hip, ora = _pair({"num_of_agents": A, "init_cash": RICH, "max_step": 64, "is_render": False, "book_capacity": tile}, 3)
    assert hip.env.book_capacity == tile
    for m in range(3):                                               # market m: level k holds 1 + (k + 5 m) % 16 orders, best level first on both sides
        placed = level = 0
        while placed < per_side:                                     # (the two sides grow together, level by level)
            width = min(1 + (level + 5 * m) % A, per_side - placed)
            for side, price in ((K.S_BID, 20000 - level), (K.S_ASK, 30000 + level)):
                for j in range(width):
                    for e in (hip, ora):
                        e.place_order(m, j, K.T_LIMIT, side, 1 + (placed + j) % 6, price)
            placed += width; level += 1
    got = check(hip, ora, levels=8, tag="built")
    assert (got["counts"][:, :, 0] == per_side).all()
    straddles = 0
    for m in range(3):
        tails, _ = _ring_meta(hip.env, m)
        assert tails[0] > 0 and tails[1] > 0, (m, tails)             # both sides continue in the ring
        for s in (0, 1):
            side, t = ora.get_book(m, s), per_side - tails[s]        # t = orders of the side in the tile
            straddles += int(side[t - 1, 0] == side[t, 0])
            cq = np.cumsum(side[:, 1].astype(np.int64))
            check(hip, ora, levels=4, sizes=[int(cq[t - 2]), int(cq[t - 1]), int(cq[t - 1]) + 1, int(cq[t]), int(cq[-1]), int(cq[-1]) + 1], first=m, n=1, tag=("tile end", m, s))
    assert straddles >= 1                                            # a level whose orders lie on both sides of the tile's end
    n_levels = int(got["counts"][:, :, 1].max())
    for L in (n_levels - 1, n_levels, n_levels + 3):
        check(hip, ora, levels=L, tag=f"L={L}")
    assert (hip.flags() == 0).all() and (hip.env.check_invariants().cpu().numpy() == 0).all()
    hip.close(); ora.close()


def test_ring_wrap():
    """book_spill = 64: a ring of 64 slots per side behind the 256-order tile.  The ring is filled, the top of the book consumed so that the tile refills from
    it, new orders rest behind, and better orders then push the tile's last orders back in front of the ring's.  The oracle's book is unbounded for a config
    with book_spill >= 0 (oracle/cda_oracle.c); the orders are chosen so that nothing is dropped: flags() stays 0 on both."""
    cfg = {"num_of_agents": 4, "init_cash": RICH, "max_step": 64, "is_render": False, "book_spill": 64}
    hip, ora = _pair(cfg, 1)
    assert hip.env.book_spill == 64 and hip.env.book_capacity == 256

    def do(tr, typ, side, size, price):
        for e in (hip, ora):
            e.place_order(0, tr, typ, side, size, price)

    for k in range(256):                                             # the tile: 256 bids at even prices, one unit each
        do(k % 4, K.T_LIMIT, K.S_BID, 1, 20000 - 2 * k)
    through_ring = 0
    for k in range(64):                                              # worse than every tile order of a full pool: they start and fill the ring (cda_book.inc cold_insert)
        do(k % 4, K.T_LIMIT, K.S_BID, 2, 10000 - k)
    through_ring += 64
    assert _ring_meta(hip.env, 0)[0] == (64, 0)
    check(hip, ora, levels=40, tag="ring full")
    do(0, K.T_MARKET, K.S_ASK, 230, 1)                               # a sell eats the 230 best bids: 26 < TILE_LOW are left, cold_rebalance pops the ring into the tile
    assert _ring_meta(hip.env, 0)[0] == (0, 0)
    check(hip, ora, levels=40, tag="refilled")
    for k in range(166 + 24):                                        # new orders behind: 166 fill the pool again, the other 24 go to the ring
        do(k % 4, K.T_LIMIT, K.S_BID, 3, 9000 - k)
    through_ring += 24
    for k in range(6):                                               # better than most of the full tile: each insert needs room, the first makes it by handing the
        do(k % 4, K.T_LIMIT, K.S_BID, 1, 19001 - 2 * k)              # tile's last 32 orders to the ring's head (tile_push_to_tail: base -= 32)
    through_ring += 32
    tails, bases = _ring_meta(hip.env, 0)
    # How this knows the live window wraps: order i of the tail sits in slot (base + i) & 63 (Tail::slot).  The snapshot reports base and count as the kernels
    # left them; the window [base, base + n) crosses the ring's end exactly when (base & 63) + n > 64.  Prepending moved base below the slot the 24 appended
    # orders start at, so the 56 orders run over slot 63 into slot 0.
    assert tails[0] == 56 and (bases[0] & 63) + tails[0] > 64, (tails, bases)
    assert through_ring > 64
    got = check(hip, ora, levels=300, sizes=[1, 25, 26, 27, 400, 401, 10 ** 5], tag="wrapped")
    assert got["counts"][0, 0, 0] == 26 + 64 + 190 + 6
    do(1, K.T_MARKET, K.S_ASK, 472, 1)                               # 200 orders eaten, 30 < TILE_LOW left in the tile: the wrapped window is popped into it
    assert _ring_meta(hip.env, 0)[0] == (0, 0)
    check(hip, ora, levels=300, tag="popped")
    assert (hip.flags() == 0).all() and (ora.flags() == 0).all() and (hip.env.check_invariants().cpu().numpy() == 0).all()
    hip.close(); ora.close()


@pytest.mark.parametrize("agents,tile", [(4, 256), (4, 512), (8, 256), (8, 512)])
def test_played_books(agents, tile):
    """64 markets under the trending action law of tests/test_hip_bigbook.py, six of them on top of 2 x 330 prefilled orders (beyond either tile); every market
    against the oracle after 200 steps, and a sub-range against the slice of the full call."""
    from fuzz_cases import prefill_book
    from test_hip_bigbook import _trend
    n, steps = 64, 200
    hip, ora = _pair({"num_of_agents": agents, "init_cash": 10 ** 9, "max_step": 4096, "is_render": False, "book_capacity": tile}, n)
    for i in range(0, n, 11):
        for e in (hip, ora):
            prefill_book(e, i, np.random.default_rng(90 + i), agents, 330, 330)
    rng = np.random.default_rng(11 + agents)
    for t in range(steps):
        acts = _trend(rng, n, agents, t, 0)
        ho, *_ = hip.step(*acts)
        oo, *_ = ora.step(*acts)
        if t % 50 == 49:
            assert np.array_equal(ho.view(np.uint32), oo.view(np.uint32)), t
    full = check(hip, ora, levels=16, tag="played")
    assert full["counts"][:, :, 0].sum(axis=1).max() > tile                 # books beyond the tile are among them
    part = _device_report(hip.env, 16, SIZES, 5, 17)
    for k in ("counts", "levels", "impact", "agents"):
        assert np.array_equal(part[k], full[k][5:22]), k
    lo, hi = full["offsets"][10], full["offsets"][44]
    assert np.array_equal(part["offsets"], full["offsets"][10:45] - lo) and np.array_equal(part["orders"], full["orders"][lo:hi])
    assert (hip.flags() == 0).all() and (hip.env.check_invariants().cpu().numpy() == 0).all()
    hip.close(); ora.close()


def test_against_the_other_kernels():
    """256 markets, 50 random steps: after every step the ladder's first ten levels are the raw snapshot (agg_LOB_raw, k_raw_snapshot) of the same book - the
    identity "ladder before the step == raw snapshot after it" does not hold for the reference, see tests/test_book_report_host.py -, the counts are the
    differences of the dump's offsets, an agent's resting notional is its cash_on_hold, and the invariant kernel agrees."""
    from decimal import Decimal

    from gym_continuousdoubleauction_amd import CDAVecEnv
    from test_book_report_host import raw_from_ladders
    n, a = 256, 4
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 4096, "is_render": False}, n_markets=n, device="cuda:0")
    env.reset(seed=77)
    acts = env.random_actions_device(0, 50, action_seed=5)
    checked = 0
    for t in range(50):
        _, _, term, trunc, _ = env.step(*(x[t] for x in acts))
        live = ~(term | trunc)
        want = torch.from_numpy(raw_from_ladders(env.book_levels(10).cpu().numpy())).to(env.device)
        assert torch.equal(want[live], env.raw_snapshot()[live]), t
        checked += int(live.sum())
    assert checked > 25 * n
    counts, (rows, off), agents = env.book_counts().cpu().numpy(), env.book_orders(), env.book_agents().cpu().numpy()
    assert np.array_equal(counts[:, :, 0].reshape(-1), np.diff(off.cpu().numpy())) and rows.shape[0] == counts[:, :, 0].sum() > n
    for i in range(0, n, 32):
        st = env.get_state(i)
        for j in range(a):
            assert K.dec_to_decimal(st.acc[j].cash_on_hold) == Decimal(int(agents[i, 0, j, 2] + agents[i, 1, j, 2])), (i, j)
    assert (env.check_invariants().cpu().numpy() == 0).all()
    env.close()


@pytest.mark.parametrize("groups", [1, 2])
def test_a_reader_behind_a_pipelined_step_sees_the_stepped_book(groups):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a = 512, 4
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 4096, "is_render": False}, n_markets=n, device="cuda:0", groups=groups)
    env.reset(seed=3)
    acts = env.random_actions_device(0, 12, action_seed=8)
    for t in range(11):
        env.step(*(x[t] for x in acts), pipelined=True)
    pre = env.book_levels(6).clone()
    torch.cuda.synchronize()
    env.step(*(x[11] for x in acts), pipelined=True)
    at_once = (env.book_counts(), env.book_levels(6), env.book_impact([1, 50]), env.book_agents(), *env.book_orders())     # no synchronisation in between
    torch.cuda.synchronize()
    later = (env.book_counts(), env.book_levels(6), env.book_impact([1, 50]), env.book_agents(), *env.book_orders())
    for x, y in zip(at_once, later):
        assert torch.equal(x, y)
    assert not torch.equal(pre, later[1])                            # the step moved the books
    env.close()
