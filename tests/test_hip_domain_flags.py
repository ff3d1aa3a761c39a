"""GPU: CDA_FLAG_INT_OVERFLOW and CDA_FLAG_DEC_DOMAIN observed set, each at the edge its comparison in the code draws and one step
inside it.  Device only (the oracle raises neither INT_OVERFLOW nor the float(Decimal) case).  Every state is seeded with
cda_set_state and driven with the place_order / mark_to_mkt hooks or step(); all of it is integer and decimal arithmetic on
in-bounds memory - no array is indexed by the out-of-domain value.

Every site that raises one of the two bits:

  site                                              bit           tested / why not
  ------------------------------------------------  ------------  ------------------------------------------------------------------
  cda_book.inc settle_fill, |position| > 2^31 - 1   INT_OVERFLOW  test_position_edge: +-(2^31 - 1) is exact and clean, one more unit flags
  cda_book.inc place_order, next_oid >= 2^27        INT_OVERFLOW  test_order_id_edge: id 2^27 - 1 is the last clean one (cda_set_state accepts
                                                                  order ids below 2^27: the id shares a word with the owner nibble)
  cda_kernels.inc step_market, price >= 2^24        INT_OVERFLOW  test_price_clamp_edge: 2^24 - 1 decodes clean, 2^24 is clamped to 2^24 - 1
                                                                  and flagged ("prices live below 2^24", include/cda.h CDA_TICK_MAX)
  cda_kernels.inc step_market, size > 1e9           INT_OVERFLOW  unreachable: |mean| <= 1 and sigma <= 1 are clamped and cda_create bounds
                                                                  mkt_max_size x limit_size_multiple + min_size by 2^21, so the size would
                                                                  need a standard normal beyond 10^9
  cda_dec.hpp d_to_double, exponent outside          DEC_DOMAIN    test_float_of_a_ledger_value_edge, through the reward's float(nav - prev_nav)
    [-109, 0] (cda_kernels.inc step_loaded and                     of step(): exponents 0 and -109 convert clean, +1 and -110 flag.  The
    run_random_part raise it from the same ferr)                   same wrapper and comparison serve the info tensors and cda_run_random
  cda_market.hpp st_dec, exponent outside int16,    DEC_DOMAIN    test_stored_exponent_edge: cash + cash_on_hold of 28 digits each at exponent
    raised in cda_book.inc mark_to_mkt                            32767 carries into exponent 32768 (flagged); without the carry it stays clean
  the same st_dec in cda_book.inc settle_fill and   DEC_DOMAIN    unreachable from an in-domain state: both add an order or trade value
    place_order (cash / hold transfers)                           (exponent -1, below 2^59) to an account field.  A sum's exponent is never
                                                                  below the smaller operand's, and it rises only when the sum carries into a
                                                                  29th digit - impossible against a field at exponent ~32767, next to which
                                                                  the value vanishes in the rounding; the VWAP division lowers an exponent
                                                                  by at most 28 from that of a sum which is at least about -30

The header's words and the code's comparisons agree at every edge tested; no kernel was changed.
A raised bit is sticky across a following clean step and cleared by reset (include/cda.h "Per-market sticky flag bits"):
test_price_clamp_edge pins that too."""
from decimal import Decimal

import numpy as np
import pytest

from gym_continuousdoubleauction_amd import _capi as K

pytestmark = pytest.mark.gpu

D = Decimal
CASH = 10 ** 12


def _env(n, agents=4, with_info=True, **cfg):
    from hip_env import HipEnv
    hip = HipEnv(dict({"num_of_agents": agents, "init_cash": CASH, "max_step": 1000, "is_render": False}, **cfg), n, with_info=with_info)
    hip.reset(np.arange(7, 7 + n, dtype=np.uint64))
    return hip


def _dec(x):
    return K.decimal_to_dec(D(x))


def test_position_edge():
    hip = _env(1)
    big = 2 ** 31 - 2
    s = hip.get_state(0)
    s.has_trade, s.last_trade_price, s.last_price = 1, 100, 100
    for j, pos in ((0, big), (1, -big)):                     # agent 0 long, agent 1 short, both opened at 100.0; matching ledger rows
        acc = s.acc[j]
        acc.net_position = pos
        acc.vwap = _dec("100.0")
        acc.position_val = K.decimal_to_dec(D("100.0") * big)
        acc.cash = K.decimal_to_dec(D(CASH) - D("100.0") * big)
        acc.nav = acc.prev_nav = acc.max_nav = _dec(f"{CASH}.0")
    hip.set_state(0, s)

    def cross_one_unit():
        hip.place_order(0, 1, K.T_LIMIT, K.S_ASK, 1, 100)    # the short agent offers one more unit
        hip.place_order(0, 0, K.T_LIMIT, K.S_BID, 1, 100)    # the long agent takes it

    cross_one_unit()
    s = hip.get_state(0)
    assert hip.flags()[0] == 0
    assert (s.acc[0].net_position, s.acc[1].net_position) == (2 ** 31 - 1, -(2 ** 31 - 1)) and s.n_bids == s.n_asks == 0
    assert K.dec_to_decimal(s.acc[0].vwap) == 100 and K.dec_to_decimal(s.acc[0].position_val) == 100 * (2 ** 31 - 1)
    cross_one_unit()
    assert hip.flags()[0] == K.FLAG_INT_OVERFLOW
    hip.close()


def test_order_id_edge():
    hip = _env(1)
    s = hip.get_state(0)
    s.next_order_id = (1 << 27) - 2
    hip.set_state(0, s)
    hip.place_order(0, 0, K.T_LIMIT, K.S_BID, 1, 50)         # takes id 2^27 - 1, the last one of the domain
    assert hip.flags()[0] == 0
    assert hip.get_state(0).next_order_id == (1 << 27) - 1 and hip.get_book(0, 0)[0, 3] == (1 << 27) - 1
    hip.place_order(0, 1, K.T_MARKET, K.S_BID, 1)            # the next id, 2^27 (nothing to match, nothing rests)
    assert hip.flags()[0] == K.FLAG_INT_OVERFLOW
    assert hip.get_state(0).next_order_id == 1 << 27
    hip.close()


def test_price_clamp_edge():
    top = (1 << 24) - 1
    hip = _env(2)
    for i in range(2):
        s = hip.get_state(i)
        assert s.n_bids == s.n_asks == 0
        s.last_price = top - 1                               # an empty ask side decodes level l as last_price + (l + 1) ticks
        hip.set_state(i, s)
    n, a = 2, 4
    cat = np.zeros((n, a), np.int32)
    level = np.zeros((n, a), np.int32)
    cat[:, 0] = 6                                            # agent 0: a limit ask
    level[1, 0] = 1                                          # market 0 decodes 2^24 - 1, market 1 2^24
    zeros = np.zeros((n, a), np.float32)
    off = np.ones((n, a), np.int32)                          # price_offset 1 = no offset
    _obs, _rew, _term, _trunc, info = hip.step(cat, zeros, zeros, level, off)
    assert list(info["lob_actions"][:, 0, 3]) == [top, top]  # one tick inside as decoded; 2^24 clamped to 2^24 - 1
    assert list(hip.flags()) == [0, K.FLAG_INT_OVERFLOW]
    for i in range(2):
        asks = hip.get_book(i, 1)
        assert len(asks) == 1 and asks[0, 0] == top and asks[0, 1] == 1
    # sticky across a clean step (everybody passes) ...
    hip.step(np.zeros((n, a), np.int32), zeros, zeros, np.zeros((n, a), np.int32), off)
    assert list(hip.flags()) == [0, K.FLAG_INT_OVERFLOW]
    # ... and cleared by reset
    hip.reset(np.array([1, 2], np.uint64), mask=np.array([0, 1], np.uint8))
    assert list(hip.flags()) == [0, 0]
    assert (hip.env.check_invariants().cpu().numpy() == 0).all()
    hip.close()


def test_float_of_a_ledger_value_edge():
    """float(nav - prev_nav) of the reward (Decimal.__float__): the exact paths cover exponents -109 .. 0 (csrc/cda_dec.hpp)."""
    exps = [0, 1, -109, -110]
    want = [0, K.FLAG_DEC_DOMAIN, 0, K.FLAG_DEC_DOMAIN]
    hip = _env(len(exps), with_info=False)                   # (no info tensors: the reward's conversion is the only one of the step)
    for i, e in enumerate(exps):
        s = hip.get_state(i)
        assert s.has_trade == 0                              # mark_to_mkt leaves nav alone
        for j in range(4):
            s.acc[j].nav = s.acc[j].max_nav = K.decimal_to_dec(D((0, (1, 0, 0, 0, 0, 3), e)))
            s.acc[j].prev_nav = K.decimal_to_dec(D((0, (1, 0, 0, 0, 0, 1), e)))
        hip.set_state(i, s)
    n, a = len(exps), 4
    zi, zf = np.zeros((n, a), np.int32), np.zeros((n, a), np.float32)
    _obs, rew, *_ = hip.step(zi, zf, zf, zi, zi)             # everybody passes
    assert list(hip.flags()) == want
    assert (rew[0] == 2.0).all() and (rew[2] == 2e-109).all()          # the in-domain conversions are the correctly rounded doubles
    hip.close()


def test_stored_exponent_edge():
    """nav = (cash + cash_on_hold) + position_val in mark_to_mkt: a cda_dec stores its exponent as int16."""
    hip = _env(2)
    for i, lead in enumerate((4, 9)):                        # 4999...9 + 4999...9 keeps 28 digits; 9999...9 + 9999...9 carries into a 29th
        s = hip.get_state(i)
        s.has_trade, s.last_trade_price = 1, 100
        big = K.decimal_to_dec(D((0, (lead,) + (9,) * 27, 32767)))
        s.acc[0].cash = s.acc[0].cash_on_hold = big
        hip.set_state(i, s)
        hip.mark_to_mkt(i)
    assert list(hip.flags()) == [0, K.FLAG_DEC_DOMAIN]
    sign, coeff, exp = K.dec_to_int_exp(hip.get_state(0).acc[0].nav)
    assert (sign, coeff, exp) == (0, 10 ** 28 - 2, 32767)    # Decimal: 4.99..9E+32794 twice = 9.99..8E+32794, exact in 28 digits
    hip.close()
