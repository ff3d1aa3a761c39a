"""GPU: cda_check_invariants (k_check_invariants / BookView, csrc/cda_hip.hip) against the plain restatement of tests/invariants_ref.py.

About thirty GPU tests end in `check_invariants() == 0`; these tests show that the checker can say something else, and says the
right thing: every state is SEEDED through cda_set_state (which validates counts, owners and order ids, so tile and ring indices
stay in bounds whatever prices, quantities and accounts say), read by check_invariants / get_state / get_book only - never
stepped, never handed to place_order or a report kernel - and the WHOLE word of every market is compared:
device == invariants_ref(what get_book and get_state read back) == the word the case was built for.  Violating markets sit at
odd indices between valid ones that must read 0 (per-market indexing of record and spill region).

Stricter than Decimal: the kernel accepts a hold only at exponent -18 .. 0.  A numerically correct hold written at exponent -19
or +1 - which the ledger never produces: holds are sums of price x qty at exponent -1 - is flagged CDA_INV_ESCROW although
Decimal equality holds.  Those two markets are pinned in asserts of their own, apart from the reference comparison.

Left out: CDA_INV_OWNER and CDA_INV_BOOK_COUNT.  cda_set_state refuses an owner >= num_agents and counts beyond tile + ring;
forcing them would take a raw write of counts other kernels index with.  (tests/test_invariants_ref_host.py covers the
restatement's OWNER rule on the host.)

The last test of the module tallies the expected words actually compared: every reachable bit alone in at least two markets and
in combination in at least one.  It counts what the tests above it checked, so it is meant to run with the whole module."""
from decimal import Decimal

import numpy as np
import pytest

from gym_continuousdoubleauction_amd import _capi as K
from invariants_ref import accounts_of, big_book_state, invariants_ref

pytestmark = pytest.mark.gpu

D = Decimal
INIT_CASH = 10 ** 12
BITS = (K.INV_BIDS_SORTED, K.INV_ASKS_SORTED, K.INV_CROSSED, K.INV_QTY, K.INV_ESCROW, K.INV_NET_POSITION)
TALLY = []            # every expected word that was compared with the device and the reference
GROUPS = set()


def _side(s, sd):
    return s.bids if sd == 0 else s.asks


def _seed_book(s, a, nb, na, mid=10000, owners=None):
    """a valid book of distinct prices: bids mid-1, mid-2, ... and asks mid+1, mid+2, ... in queue order"""
    owners = a if owners is None else owners
    for k in range(nb):
        o = s.bids[k]
        o.price, o.qty, o.owner, o.order_id, o.timestamp = mid - 1 - k, 1 + k % 3, k % owners, 2 * k + 1, 2 * k + 1
    for k in range(na):
        o = s.asks[k]
        o.price, o.qty, o.owner, o.order_id, o.timestamp = mid + 1 + k, 1 + k % 3, (k + 3) % owners, 2 * k + 2, 2 * k + 2
    s.n_bids, s.n_asks = nb, na
    s.lob_time = s.next_order_id = 2 * max(nb, na) + 2


def _resting(s, a):
    v = [0] * a
    for sd in (0, 1):
        rows = _side(s, sd)
        for k in range(s.n_bids if sd == 0 else s.n_asks):
            v[rows[k].owner] += rows[k].price * rows[k].qty
    return v


def _at_exp(value, e):
    """the integer `value` as a Decimal written at exponent e"""
    coeff = abs(value) * 10 ** (-e) if e <= 0 else abs(value) // 10 ** e
    x = D((int(value < 0), tuple(int(c) for c in str(coeff)), e))
    assert x == value                                  # (exact: Decimal comparison does not round)
    return x


def _set_hold(s, j, x):
    s.acc[j].cash_on_hold = K.decimal_to_dec(x)


def _hold(s, j):
    return K.dec_to_decimal(s.acc[j].cash_on_hold)


def _fit_holds(s, a):
    for j, v in enumerate(_resting(s, a)):
        _set_hold(s, j, _at_exp(v, -1))
        s.acc[j].cash = K.decimal_to_dec(_at_exp(INIT_CASH - v, -1))


def _swap_px(sd, k):
    def f(s):
        r = _side(s, sd)
        r[k].price, r[k + 1].price = r[k + 1].price, r[k].price
    return f


def _put(sd, k, field, v):
    def f(s):
        setattr(_side(s, sd)[k], field, v)
    return f


def _both(*fs):
    def f(s):
        for g in fs:
            g(s)
    return f


def _pos(*vals):
    def f(s):
        for j, v in enumerate(vals):
            s.acc[j].net_position = v
    return f


def _hold_add(j, x):
    return lambda s: _set_hold(s, j, _hold(s, j) + x)


def _run_cases(group, agents, nb, na, cases, **seed_kw):
    """cases: (name, edit of the book or None, edit of the accounts or None, expected word, compare with the reference?).  Market
    2j is valid, market 2j + 1 carries case j; the holds are fitted to the EDITED book, so a book edit fires its own rule only.
    Returns {name: device word} of the cases that are not compared with the reference."""
    from hip_env import HipEnv
    n = 2 * len(cases)
    assert n <= 64
    hip = HipEnv({"num_of_agents": agents, "init_cash": INIT_CASH, "max_step": 64, "is_render": False}, n)
    hip.reset(np.arange(n, dtype=np.uint64))
    want = []
    for i in range(n):
        name, book_edit, acc_edit, word, _cmp = cases[i // 2] if i % 2 else ("valid", None, None, 0, True)
        s = hip.get_state(i)
        kw = dict(seed_kw)
        if name.startswith("nothing resting"):
            kw["owners"] = agents - 1
        if name.startswith("big"):
            kw["mid"] = (1 << 24) - 500
        _seed_book(s, agents, nb, na, **kw)
        if book_edit:
            book_edit(s)
        _fit_holds(s, agents)
        if acc_edit:
            acc_edit(s)
        hip.set_state(i, s)
        want.append((name, word, _cmp))
    dev = hip.env.check_invariants().cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    apart = {}
    for i, (name, word, cmp_) in enumerate(want):
        bids, asks = hip.get_book(i)
        s = hip.get_state(i)
        assert len(bids) == nb == s.n_bids and len(asks) == na == s.n_asks, (i, name)
        ref = invariants_ref(bids, asks, accounts_of(s, agents), agents)
        if cmp_:
            assert int(dev[i]) == ref == word, (group, i, name, hex(int(dev[i])), hex(ref), hex(word))
            TALLY.append(word)
        else:
            apart[name] = (int(dev[i]), ref)
    assert (hip.flags() == 0).all()
    hip.close()
    GROUPS.add(group)
    return apart


AGENTS = [4, 8, 16]               # tile 256 (4 and 8 agents) and tile 512 (16 agents)


@pytest.mark.parametrize("agents", AGENTS)
def test_tile_only_books_one_violation_per_odd_market(agents):
    B, A_, X, Q, N = K.INV_BIDS_SORTED, K.INV_ASKS_SORTED, K.INV_CROSSED, K.INV_QTY, K.INV_NET_POSITION
    n = 40
    cases = [
        ("bids swapped at the top", _swap_px(0, 0), None, B, True),
        ("bids swapped in the middle", _swap_px(0, 19), None, B, True),
        ("bids swapped at the last order", _swap_px(0, n - 2), None, B, True),
        ("asks swapped at the top", _swap_px(1, 0), None, A_, True),
        ("asks swapped in the middle", _swap_px(1, 19), None, A_, True),
        ("asks swapped at the last order", _swap_px(1, n - 2), None, A_, True),
        ("an equal-price run of bids", _both(*[_put(0, k, "price", 10000 - 11) for k in range(10, 15)]), None, 0, True),
        ("an equal-price run of asks", _both(*[_put(1, k, "price", 10000 + 15) for k in range(10, 15)]), None, 0, True),
        ("best bid == best ask", _put(0, 0, "price", 10001), None, X, True),
        ("best bid above best ask", _put(0, 0, "price", 10006), None, X, True),
        ("best bid == best ask - 1", _both(_put(0, 0, "price", 10001), _put(1, 0, "price", 10002)), None, 0, True),
        ("qty 0", _put(0, 5, "qty", 0), None, Q, True),
        ("qty -1", _put(1, 7, "qty", -1), None, Q, True),
        ("price 0", _put(0, n - 1, "price", 0), None, Q, True),
        ("net position +1", None, _pos(1), N, True),
        ("net position -(2^31 - 1) over two agents", None, _pos(-(2 ** 30), -(2 ** 30 - 1)), N, True),
        ("net position -2^32 over two agents", None, _pos(-(2 ** 31), -(2 ** 31)), N, True),      # zero to an int32 accumulator
    ]
    _run_cases("tile", agents, n, n, cases)


@pytest.mark.parametrize("agents", AGENTS)
def test_escrow_edges_per_agent(agents):
    """... and the two holds the kernel refuses although Decimal equality holds (see the module docstring): exponent -19 and +1."""
    E = K.INV_ESCROW
    n = 40

    def rewrite(e):
        def f(s):
            for j, v in enumerate(_resting(s, agents)):
                _set_hold(s, j, _at_exp(v, e))
        return f

    def big(s):                                            # order values of 2^55: a hold's coefficient passes 2^64 (w[2]) well above exponent -18
        for sd in (0, 1):
            for k in range(0, n, 4):
                _side(s, sd)[k].qty = 2 ** 31 - 1

    def w2_only(s):                                        # the hold of agent 0 differs from the truth in w[2] alone
        rewrite(-8)(s)
        s.acc[0].cash_on_hold.w[2] += 1

    cases = [
        ("hold one tick too high", None, _hold_add(1, D("0.1")), E, True),
        ("hold one tick too low", None, _hold_add(2, D("-0.1")), E, True),
        ("hold correct but negative", None, lambda s: _set_hold(s, 0, -_hold(s, 0)), E, True),
        ("nothing resting, hold -0.0", None, lambda s: _set_hold(s, agents - 1, D("-0.0")), 0, True),
        ("holds at exponent 0", None, rewrite(0), 0, True),
        ("holds at exponent -1", None, rewrite(-1), 0, True),
        ("holds at exponent -18", None, rewrite(-18), 0, True),
        ("big values, holds at exponent -8", big, rewrite(-8), 0, True),
        ("big values, one hold wrong in w[2] only", big, w2_only, E, True),
        ("hold ten times the truth", None, lambda s: _set_hold(s, 3, _hold(s, 3) * 10), E, True),
        ("a shortfall offset by another agent's excess", None, _both(_hold_add(0, D(-7)), _hold_add(1, D(7))), E, True),
        ("stricter: exponent -19", None, rewrite(-19), E, False),
        ("stricter: exponent +1", _both(*[_put(sd, k, "qty", 10) for sd in (0, 1) for k in range(n)]), rewrite(1), E, False),
    ]
    apart = _run_cases("escrow", agents, n, n, cases)
    # numerically these holds ARE the value of the resting orders (the restatement says 0); the kernel's exponent window says ESCROW
    assert apart["stricter: exponent -19"] == (K.INV_ESCROW, 0)
    assert apart["stricter: exponent +1"] == (K.INV_ESCROW, 0)


@pytest.mark.parametrize("agents", AGENTS)
def test_books_that_continue_in_the_ring_and_combinations(agents):
    """400 + 400 orders: cda_set_state shares the tile evenly (128 + 128 of 256, 256 + 256 of 512) and the rest of each side lies in
    the HBM ring.  Violations at the last tile order, the first ring order, across that boundary and at the ring's last order."""
    B, A_, X, Q, E, N = BITS
    n, T = 400, (256 if agents <= 8 else 512) // 2

    def ring_order_unpaid(sd, k):                          # the owner's hold misses exactly the value of one ring-resident order
        def f(s):
            o = _side(s, sd)[k]
            _set_hold(s, o.owner, _hold(s, o.owner) - o.price * o.qty)
        return f

    cases = []
    for sd, bit, nm in ((0, B, "bids"), (1, A_, "asks")):
        cases += [
            (f"{nm} swapped at the last tile order", _swap_px(sd, T - 2), None, bit, True),
            (f"{nm} swapped across the tile's end", _swap_px(sd, T - 1), None, bit, True),
            (f"{nm} swapped at the first ring order", _swap_px(sd, T), None, bit, True),
            (f"{nm} swapped at the ring's last order", _swap_px(sd, n - 2), None, bit, True),
            (f"{nm} qty 0 at the last tile order", _put(sd, T - 1, "qty", 0), None, Q, True),
            (f"{nm} qty -1 at the first ring order", _put(sd, T, "qty", -1), None, Q, True),
            (f"{nm} ring's last order", _put(sd, n - 1, "price", 0) if sd == 0 else _put(sd, n - 1, "qty", 0), None, Q, True),
            (f"{nm} a ring order's value missing from the hold", None, ring_order_unpaid(sd, T + 5), E, True),
        ]
    cases += [
        ("combination of three", _both(_swap_px(0, T - 1), _put(1, n - 1, "qty", 0)), _pos(1), B | Q | N, True),
        ("combination of four", _both(_swap_px(1, 0), _put(0, 0, "price", 10002)), _both(_hold_add(2, D("0.1")), _pos(0, -3)), A_ | X | E | N, True),
        ("combination of five", _both(_swap_px(0, n - 2), _swap_px(1, T), _put(0, T + 9, "qty", -1)),
         _both(_hold_add(1, D(-1)), _pos(5, 5)), B | A_ | Q | E | N, True),
    ]
    _run_cases("ring", agents, n, n, cases)


DEEP = 600            # enough that a side still holds more than CDA_BOOK_CAP_MAX orders after the random play below


def wrapped_ring_book(env, i, a):
    """Market i (holding the 2 x 400 book of big_book_state, 100 ticks off last_price) is driven through the place_order hook until
    its bid ring has moved at both ends: DEEP bids behind the book (appended to the ring), 150 better bids than any (each lands in
    the full tile and pushes the tile's last order onto the ring's FRONT: the base goes below zero and wraps), one market order
    that eats 260 bids - more than the tile holds - so the tile is refilled from the ring's head (the base moves forward), and 30
    more bids at the front.  Returns the market's last_price."""
    lp = env.get_state(i).last_price
    for j in range(DEEP):
        env.place_order(i, j % a, K.T_LIMIT, K.S_BID, 1 + j % 2, lp - 201 - j)
    for j in range(150):
        env.place_order(i, j % a, K.T_LIMIT, K.S_BID, 1, lp - 99 + j // a)
    env.place_order(i, 1, K.T_MARKET, K.S_ASK, 150 + sum(1 + k % 3 for k in range(110)), 1)
    for j in range(30):
        env.place_order(i, j % a, K.T_LIMIT, K.S_BID, 2, lp - 60 + j // a)
    for j in range(40):
        env.place_order(i, (j + 1) % a, K.T_LIMIT, K.S_ASK, 1, lp + 99 - j // a)
    return lp


@pytest.mark.parametrize("agents", AGENTS)
def test_a_wrapped_ring_and_the_keep_book_path(agents):
    from hip_env import HipEnv
    n, a = 3, agents
    tile = 256 if a <= 8 else 512
    cfg = {"num_of_agents": a, "init_cash": 10 ** 9, "max_step": 4000, "is_render": False, "initial_price_min": 5000, "initial_price_max": 6000,
           "mkt_max_size": 4, "limit_size_multiple": 2}
    hip = HipEnv(cfg, n)
    hip.reset(np.arange(40, 40 + n, dtype=np.uint64))
    for i in range(n):
        hip.set_state(i, big_book_state(hip.get_state(i), a, 10 ** 9, gap=100))
        lp = wrapped_ring_book(hip, i, a)
        bids = hip.get_book(i, 0)
        assert len(bids) == 400 + DEEP + 150 - 260 + 30 and len(hip.get_book(i, 1)) == 440
        # the tile was refilled: the sweep ate more orders than the tile can hold, so what leads the book now came out of the ring
        assert 260 > tile // 2 and bids[30, 0] == lp - 100 - 110 // 4 and bids[30, 3] == 2 * 110 + 1
    assert (hip.env.book_peak().cpu().numpy() == 800 + DEEP + 150).all()

    def compare(want):
        dev = hip.env.check_invariants().cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        for i in range(n):
            s = hip.get_state(i)
            b, q = hip.get_book(i)
            assert s.n_bids == len(b) > K.BOOK_CAP_MAX and s.n_asks == len(q), (i, s.n_bids, s.n_asks)
            ref = invariants_ref(b, q, accounts_of(s, a), a)
            assert int(dev[i]) == ref == want[i], (i, hex(int(dev[i])), hex(ref), hex(want[i]))
            TALLY.append(want[i])

    compare([0] * n)
    hip.env.run_random(200, action_seed=31)                # evictions and refills inside the fused loop move the base further
    assert (hip.flags() == 0).all()
    compare([0] * n)
    # the keep-book path of cda_set_state (counts above CDA_BOOK_CAP_MAX): only the accounts change, the book stays where it lies
    want = [K.INV_ESCROW, K.INV_NET_POSITION, K.INV_ESCROW | K.INV_NET_POSITION]
    for i in range(n):
        s = hip.get_state(i)
        if want[i] & K.INV_ESCROW:
            _set_hold(s, 2, _hold(s, 2) + D("0.1"))
        if want[i] & K.INV_NET_POSITION:
            s.acc[1].net_position += 1
        hip.set_state(i, s)
    compare(want)
    hip.close()
    GROUPS.add("wrap")


def test_tally_every_reachable_bit_fired_alone_and_in_combination():
    assert GROUPS == {"tile", "escrow", "ring", "wrap"}, GROUPS
    for bit in BITS:
        alone = sum(1 for w in TALLY if w == bit)
        combined = sum(1 for w in TALLY if w & bit and w != bit)
        assert alone >= 2 and combined >= 1, (hex(bit), alone, combined)
    assert sum(1 for w in TALLY if w == 0) >= len(TALLY) // 2      # and every second market was a valid one that read 0
    assert not any(w & (K.INV_OWNER | K.INV_BOOK_COUNT) for w in TALLY)
