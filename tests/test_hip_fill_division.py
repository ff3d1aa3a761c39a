"""GPU: the VWAP division of a fill (d_div_pos_leaf behind d_div_u32, selftest op 3) against CPython `Decimal` on fill-shaped
operands: the dividend is |pos| * VWAP +- trade value (a 28-digit VWAP times a position, plus or minus price * quantity), the
divisor the new position size.  Covers exact quotients at the ideal exponent and below it (trailing zeros stripped), quotients
that round up to 10^28, divisors next to every power of ten and next to 2^30 (the leaf's limit: larger ones take the general
routine)."""
import random
from decimal import Decimal as D, getcontext

import pytest

import oracle_lib as O
from gym_continuousdoubleauction_amd import _capi as K

pytestmark = pytest.mark.gpu


def _vwap(rng):
    """a VWAP as the ledger holds it: a tick price 'p.0', or a 28-digit quotient around it"""
    p = rng.randint(1, 20000)
    if rng.random() < 0.2:
        return D(p) * D("1.0")
    e = -27 + len(str(p))
    return D((0, tuple(int(ch) for ch in str(rng.randint(10 ** 27, 10 ** 28 - 1))), e)) if rng.random() < 0.1 else \
        D(p) + D(rng.randint(0, 10 ** 24)).scaleb(-24)


def _divisor(rng):
    r = rng.random()
    if r < 0.45:
        return rng.randint(1, 3000)                                  # the positions the workloads build
    if r < 0.65:
        return max(1, min((1 << 30) + 8, 10 ** rng.randint(0, 9) + rng.randint(-3, 3)))    # next to every power of ten
    if r < 0.75:
        return (1 << 30) + rng.randint(-6, 6)                        # next to the leaf's limit, on both sides
    if r < 0.85:
        return min((2 ** rng.randint(0, 20)) * (5 ** rng.randint(0, 6)), (1 << 30) - 1)     # exact at some scale
    return rng.randint(1, (1 << 30) - 1)


def _cases(rng, n):
    A, B = [], []
    getcontext().prec = 28
    while len(A) < n:
        r = rng.random()
        d = _divisor(rng)
        if r < 0.55:                                                 # |pos| * VWAP +- trade value
            pos = rng.randint(1, 5000)
            tv = D(rng.randint(1, 20000) * rng.randint(1, 500)) * D("1.0")
            a = pos * _vwap(rng)
            a = a + tv if rng.random() < 0.6 else a - tv
        elif r < 0.7:                                                # exact at the ideal exponent
            a = D(d * rng.randint(0, 10 ** rng.randint(1, 18))).scaleb(-rng.randint(0, 6))
        elif r < 0.8:                                                # rounds up to 10^28 (a quotient just below 10^28 - 1/2)
            a = D(d * (10 ** 28 - 1) + d - 1 - rng.randint(0, d // 3)).scaleb(-rng.randint(0, 30)) if d * (10 ** 28) < 10 ** 37 else D(10 ** 28 - 1)
            a = +a                                                   # (rounded to 28 digits like any ledger value)
        else:                                                        # anything 28-digit
            a = D((rng.randint(0, 1), tuple(int(ch) for ch in str(rng.randint(1, 10 ** rng.randint(1, 28) - 1))), rng.randint(-30, 2)))
        if rng.random() < 0.15:
            a = -a
        A.append(a); B.append(D(d))
    return A, B


def test_fill_division_matches_cpython():
    from gym_continuousdoubleauction_amd.vec_env import selftest_dec
    rng = random.Random(2024)
    A, B = _cases(rng, 200000)
    A += [D(0), D("-0E-5"), D("9999999999999999999999999999"), D("0.5"), D("1E-28")]
    B += [D(7), D(3), D(1), D(1 << 29), D((1 << 30) - 1)]
    a, b = O.dec_array(A), O.dec_array(B)
    out = selftest_dec(3, a, b)
    getcontext().prec = 28
    bad = []
    for i in range(len(A)):
        got = K.dec_to_decimal(out[i]).as_tuple()
        want = (A[i] / B[i]).as_tuple()
        if got != want:
            bad.append((A[i], B[i], want, got))
    assert not bad, (len(bad), bad[:5])
