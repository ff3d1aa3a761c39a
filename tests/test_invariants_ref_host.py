"""CPU: the plain restatement of the structural invariants (tests/invariants_ref.py) that tests/test_hip_invariants.py holds the
device's checker against.  Two halves: hand-built books on which every CDA_INV_* bit must come out alone and in combination, and
valid states the restatement did not produce itself - books and ledgers the CPU oracle reaches by playing - on which it must say 0.
The second half is what keeps the GPU comparison honest: a restatement that cried wolf on a valid book would make
`device == reference` meaningless."""
import os
import re
from decimal import Decimal

import numpy as np
import pytest

import oracle_lib as O
from gym_continuousdoubleauction_amd import _capi as K
from invariants_ref import accounts_of, big_book_state, invariants_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = Decimal


def test_inv_constants_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "cda.h")).read()
    defs = {name: int(val, 16) for name, val in re.findall(r"#define CDA_INV_([A-Z_]+)\s+(0x[0-9a-fA-F]+)u", hdr)}
    assert len(defs) == 8, defs
    for name, val in defs.items():
        assert getattr(K, "INV_" + name) == val, name
    flags = {name: int(val, 16) for name, val in re.findall(r"#define CDA_FLAG_([A-Z_]+)\s+(0x[0-9a-fA-F]+)u", hdr)}
    assert len(flags) == 4, flags
    for name, val in flags.items():
        assert getattr(K, "FLAG_" + name) == val, name


def _book():
    """a valid two-agent book: (price, qty, owner, order_id, timestamp)"""
    bids = [[100, 2, 0, 1, 1], [99, 1, 1, 2, 2], [99, 3, 0, 3, 3], [95, 1, 1, 4, 4]]
    asks = [[101, 1, 1, 5, 5], [101, 2, 0, 6, 6], [104, 4, 1, 7, 7]]
    return bids, asks


def _accounts(bids, asks, n=2):
    hold = [0] * n
    for p, q, o, *_ in bids + asks:
        hold[o] += p * q
    return [[D(h) * D("1.0"), 0] for h in hold]


def _check(mutate, want):
    bids, asks = _book()
    acc = _accounts(bids, asks)
    mutate(bids, asks, acc)
    got = invariants_ref(np.array(bids, np.int32).reshape(-1, 5), np.array(asks, np.int32).reshape(-1, 5), [tuple(a) for a in acc], 2)
    assert got == want, (hex(got), hex(want))


def _set(rows, i, col, v):
    """edit one field of one order"""
    rows[i][col] = v


def _refit(bids, asks, acc):
    for a, (h, _n) in zip(acc, _accounts(bids, asks)):
        a[0] = h


def test_a_valid_book_reads_zero():
    _check(lambda b, a, acc: None, 0)
    _check(lambda b, a, acc: (b.clear(), a.clear(), _refit(b, a, acc)), 0)                         # empty book, zero holds
    _check(lambda b, a, acc: (a.clear(), _refit(b, a, acc)), 0)                                    # one side only: nothing to cross
    _check(lambda b, a, acc: (_set(b, 0, 0, 100), _set(a, 0, 0, 101)), 0)                          # bid == ask - 1
    _check(lambda b, a, acc: acc.__setitem__(0, [acc[0][0].quantize(D("1.000000000000000000")), 0]), 0)   # the same hold at exponent -18
    _check(lambda b, a, acc: (b.clear(), a.clear(), acc.__setitem__(0, [D("-0.0"), 0]), acc.__setitem__(1, [D("0E+3"), 0])), 0)
    _check(lambda b, a, acc: (acc[0].__setitem__(1, 2 ** 31 - 1), acc[1].__setitem__(1, -(2 ** 31 - 1))), 0)


@pytest.mark.parametrize("name,mutate,want", [
    ("bids top", lambda b, a, acc: (_set(b, 0, 0, 98), _refit(b, a, acc)), K.INV_BIDS_SORTED),
    ("bids last", lambda b, a, acc: (_set(b, 3, 0, 100), _refit(b, a, acc)), K.INV_BIDS_SORTED),
    ("asks top", lambda b, a, acc: (_set(a, 0, 0, 102), _refit(b, a, acc)), K.INV_ASKS_SORTED),
    ("asks last", lambda b, a, acc: (_set(a, 2, 0, 101), _set(a, 1, 0, 102), _refit(b, a, acc)), K.INV_ASKS_SORTED),
    ("crossed equal", lambda b, a, acc: (_set(b, 0, 0, 101), _refit(b, a, acc)), K.INV_CROSSED),
    ("crossed through", lambda b, a, acc: (_set(b, 0, 0, 103), _refit(b, a, acc)), K.INV_CROSSED),
    ("qty 0", lambda b, a, acc: (_set(b, 1, 1, 0), _refit(b, a, acc)), K.INV_QTY),
    ("qty -1", lambda b, a, acc: (_set(a, 2, 1, -1), _refit(b, a, acc)), K.INV_QTY),
    ("price 0", lambda b, a, acc: (_set(b, 3, 0, 0), _refit(b, a, acc)), K.INV_QTY),
    ("hold high", lambda b, a, acc: acc[0].__setitem__(0, acc[0][0] + D("0.1")), K.INV_ESCROW),
    ("hold low", lambda b, a, acc: acc[1].__setitem__(0, acc[1][0] - D("0.1")), K.INV_ESCROW),
    ("hold negative", lambda b, a, acc: acc[1].__setitem__(0, -acc[1][0]), K.INV_ESCROW),
    ("hold offset", lambda b, a, acc: (acc[0].__setitem__(0, acc[0][0] - 7), acc[1].__setitem__(0, acc[1][0] + 7)), K.INV_ESCROW),
    ("net +1", lambda b, a, acc: acc[0].__setitem__(1, 1), K.INV_NET_POSITION),
    ("net big", lambda b, a, acc: (acc[0].__setitem__(1, -(2 ** 30)), acc[1].__setitem__(1, -(2 ** 30 - 1))), K.INV_NET_POSITION),
    ("net 2^32", lambda b, a, acc: (acc[0].__setitem__(1, -(2 ** 31)), acc[1].__setitem__(1, -(2 ** 31))), K.INV_NET_POSITION),   # zero in int32 arithmetic
    ("owner", lambda b, a, acc: (_set(b, 3, 2, 2), _refit_owned(b, a, acc)), K.INV_OWNER),
])
def test_every_bit_alone(name, mutate, want):
    _check(mutate, want)


def _refit_owned(bids, asks, acc):
    hold = [0, 0]
    for p, q, o, *_ in bids + asks:
        if o < 2:
            hold[o] += p * q
    for a, h in zip(acc, hold):
        a[0] = D(h)


def test_combinations_hide_nothing():
    _check(lambda b, a, acc: (_set(b, 0, 0, 98), _set(a, 1, 1, 0), acc[0].__setitem__(1, 5)),
           K.INV_BIDS_SORTED | K.INV_QTY | K.INV_ESCROW | K.INV_NET_POSITION)
    _check(lambda b, a, acc: (_set(a, 0, 0, 106), _set(b, 0, 0, 106), _refit(b, a, acc), acc[1].__setitem__(0, acc[1][0] + 1)),
           K.INV_ASKS_SORTED | K.INV_CROSSED | K.INV_ESCROW)
    _check(lambda b, a, acc: (_set(b, 1, 0, 120), _set(a, 2, 0, 0), _set(b, 2, 2, 3), _refit_owned(b, a, acc), acc[0].__setitem__(1, -1)),
           K.INV_BIDS_SORTED | K.INV_ASKS_SORTED | K.INV_QTY | K.INV_OWNER | K.INV_NET_POSITION)


def _all_zero(ora, n, a):
    for i in range(n):
        bids, asks = ora.get_book(i)
        s = ora.get_state(i)
        assert s.n_bids == len(bids) and s.n_asks == len(asks)
        assert invariants_ref(bids, asks, accounts_of(s, a), a) == 0, i


@pytest.mark.parametrize("agents", [4, 8, 16])
def test_states_the_oracle_plays_itself_into_read_zero(agents):
    n = 8
    ora = O.OracleEnv({"num_of_agents": agents, "init_cash": 1000000, "max_step": 400, "is_render": False}, n)
    ora.reset(np.arange(900, 900 + n, dtype=np.uint64))
    for t0 in (0, 100, 200):                                   # looked at on the way, not only at the end
        ora.run_random(t0, 100, action_seed=5 + agents)
        _all_zero(ora, n, agents)
    assert max(sum(ora.book_size(i)) for i in range(n)) > 0 and any(ora.get_state(i).has_trade for i in range(n))
    assert any(ora.get_state(i).acc[a].net_position != 0 for i in range(n) for a in range(agents))
    ora.close()


def test_the_restored_big_book_and_what_is_played_on_it_read_zero():
    n, a = 2, 8
    cfg = {"num_of_agents": a, "init_cash": 10 ** 9, "max_step": 4000, "is_render": False, "initial_price_min": 5000, "initial_price_max": 6000}
    ora = O.OracleEnv(cfg, n)
    ora.reset(np.arange(40, 40 + n, dtype=np.uint64))
    for i in range(n):
        ora.set_state(i, big_book_state(ora.get_state(i), a, 10 ** 9))
    _all_zero(ora, n, a)
    ora.run_random(0, 300, action_seed=77)
    _all_zero(ora, n, a)
    assert all(sum(ora.book_size(i)) > 512 for i in range(n))
    ora.close()
