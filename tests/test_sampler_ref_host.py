"""CPU: tests/sampler_ref.py - the host restatement of the policy kernels' action sampler - has to earn its place before tests/test_hip_sampler.py compares
a kernel with it: its mixer against the two statements of splitmix64 the suite already trusts, the float32 facts about the uniforms it models, and EVERY
statistical threshold of the device's law tests met by the restatement's own samples at the same keys and sizes (the keys are fixed: a device test with
these thresholds cannot flake, it can only be wrong)."""
import numpy as np
import pytest

import sampler_ref as R


def test_mix64_is_the_finaliser_the_suite_already_states():
    """the random module restated on R.mix64 equals tests/test_oracle_book.py's numpy statement and the library's host entry point (same finaliser)"""
    from gym_continuousdoubleauction_amd import _lib
    from test_oracle_book import _host_actions
    n, a, step, seed, base = 41, 6, 13, 0xFEEDFACE12345678, 900
    mk = np.arange(n)[:, None] + base
    mine = R.random_module(seed, mk, step, np.arange(a)[None, :])
    theirs = _host_actions(step, n, a, seed, base)
    for x, y in zip(mine, theirs):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    cat, price, off = (np.zeros((n, a), np.int32) for _ in range(3))
    mean, sigma = (np.zeros((n, a), np.float32) for _ in range(2))
    assert _lib.lib().cda_random_actions_host(seed, base, step, n, a, cat.ctypes.data, mean.ctypes.data, sigma.ctypes.data, price.ctypes.data, off.ctypes.data) == 0
    for x, y in zip(mine, (cat, mean, sigma, price, off)):
        assert np.array_equal(x, y)
    # the integer and the array form agree, at the ends of the range as well
    for z in (0, 1, R.M64, 0x8000000000000000, 0x0123456789abcdef):
        assert int(R.mix64(np.array([z], np.uint64))[0]) == R.mix64(z)
    assert R.mix64(0) == 0xe220a8397b1dcdaf                          # splitmix64's first output for seed 0 (Vigna's reference implementation)
    # the key: counter and draw enter mod 2^64, cda_policy_sample's key is the draw-0 key
    assert R.rollout_key(R.M64, 1 << 40, (1 << 31) - 1) == R.mix64((R.M64 + (1 << 40) * R.K_COUNTER + ((1 << 31) - 1) * R.K_DRAW) % (1 << 64))
    assert R.rollout_key(7, 5, 0) == R.mix64((7 + 5 * R.K_COUNTER) % (1 << 64)) != R.rollout_key(7, 5, 1)


def test_the_float32_uniform_and_where_it_leaves_the_intended_one():
    """u_f32 = u_exact for k < 2^23; above, off by at most 2^-25 (k + 1/2 rounds to even); 1.0 iff k = 2^24 - 1; u_device clamps that one value only"""
    top = np.arange((1 << 24) - 4096, 1 << 24)
    rest = np.arange(0, 1 << 24, 251)
    for k in (top, rest, np.array([0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1])):
        f, e, d = R.u_f32(k), R.u_exact(k), R.u_device(k)
        assert f.dtype == np.float32 and d.dtype == np.float32
        low = k < (1 << 23)
        assert np.array_equal(f[low].astype(np.float64), e[low])
        assert (np.abs(f.astype(np.float64) - e) <= 2.0 ** -25).all()
        assert np.array_equal(f == np.float32(1.0), k == R.TOP)
        assert (e > 0).all() and (e < 1).all() and (d > 0).all() and (d < np.float32(1.0)).all()
        assert np.array_equal(d[k != R.TOP], f[k != R.TOP]) and (d[k == R.TOP] == np.float32(R.U_MAX)).all()
        hi = ~low
        assert ((f[hi].astype(np.float64) * 16777216.0) % 2 == 0).all()                     # the even 24-bit values only
    assert np.float32(R.U_MAX) == np.nextafter(np.float32(1.0), np.float32(0.0))


def test_draws_use_five_different_half_words():
    key = R.rollout_key(3, 1, 2)
    i = np.arange(1000)
    w0, w1, w2 = R.words(key, i)
    k = R.draws24(key, i)
    assert np.array_equal(k["category"], ((w0 & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.int64))
    assert np.array_equal(k["price"], (w0 >> np.uint64(40)).astype(np.int64))
    assert np.array_equal(k["price_offset"], ((w1 & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.int64))
    assert np.array_equal(k["radius"], (w1 >> np.uint64(40)).astype(np.int64)) and np.array_equal(k["angle"], ((w2 & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.int64))
    assert int(w0[5]) == R.mix64((key + 5) % (1 << 64)) and int(w1[5]) == R.mix64(int(w0[5])) and int(w2[5]) == R.mix64(int(w1[5]))
    assert all(0 <= int(v.min()) and int(v.max()) <= R.TOP for v in k.values())


def test_heads_intervals_modes_and_log_probabilities():
    l = np.array([0.0, np.log(3.0), -100.0, 0.0], np.float32)                              # p = 1/5, 3/5, 0, 1/5
    h = R.Head(l)
    assert np.allclose(h.bounds, [0.2, 0.8, 0.8], atol=1e-7)
    assert h.interval(np.array([0.1, 0.2 - 1e-6, 0.2 + 1e-6, 0.79, 0.8 + 1e-6, 1 - 1e-9])).tolist() == [0, 0, 1, 1, 3, 3]
    assert np.allclose(h.distance_to_boundary(np.array([0.1, 0.5, 0.95])), [0.1, 0.3, 0.15], atol=1e-7)
    assert np.allclose(np.exp(h.log_prob(np.array([0, 1, 3]))), [0.2, 0.6, 0.2], atol=1e-7)
    lo, hi = h.neighbours(np.array([0.2, 0.5, 0.8]), 1e-5)
    assert lo.tolist() == [0, 1, 1] and hi.tolist() == [1, 1, 3]                           # across a dead class: its two live neighbours
    assert int(R.Head(np.array([1.0, 2.0, 2.0, 0.0], np.float32)).mode()) == 1             # a tie: the lowest index
    o = np.zeros(27, np.float32); o[22:24] = (0.3, -0.2)
    m = R.mode(o, np.array([-0.5, -0.7], np.float32))
    assert (int(m["category"]), int(m["price"]), int(m["price_offset"])) == (0, 0, 0)
    assert abs(float(m["logp"]) - (-np.log(9) - np.log(10) - np.log(3) + 0.5 + 0.7 - np.log(2 * np.pi))) < 1e-7
    s = R.sample(R.rollout_key(1, 2, 3), np.arange(50), o, np.array([-0.5, -0.7], np.float32))
    assert np.allclose(s["logp"], R.logp_of(o, np.array([-0.5, -0.7], np.float32), s["category"], s["price"], s["price_offset"], s["a_cont"]), atol=1e-9)


def test_the_table_of_top_draws_is_recomputed_not_trusted():
    """for each of the five uniforms a (seed, i) with k = 2^24 - 1 at counter 0, draw 0 inside 65536 samples - what the device's edge tests start from"""
    for name in R.UNIFORMS:
        hit = R.find_top_draw(name, 65536, seeds=range(1200))
        assert hit is not None, name
        seed, i = hit
        assert int(R.draws24(R.rollout_key(seed, 0, 0), np.array([i]))[name][0]) == R.TOP and R.u_f32(R.TOP) == np.float32(1.0)


@pytest.fixture(scope="module")
def law_draws():
    i = np.arange(R.LAW_N, dtype=np.int64)
    k = R.draws24(R.rollout_key(R.LAW_SEED, R.LAW_COUNTER, R.LAW_DRAW), i)
    n0, n1 = R.box_muller(k["radius"], k["angle"])
    return k, n0, n1


@pytest.mark.parametrize("name", sorted(R.law_distributions()))
def test_the_restatement_meets_every_threshold_of_the_law_tests(law_draws, name):
    """the device's law tests (tests/test_hip_sampler.py) at the same key and size, on the restatement's own samples - and its float32 twin agrees with it on
    every decided sample and leaves fewer than UNDECIDED_CAP undecided"""
    k, n0, n1 = law_draws
    logits = R.law_distributions()[name]
    acts = {}
    for head, lo, hi in R.HEADS:
        h = R.Head(logits[lo:hi])
        u = R.u_exact(k[head])
        acts[head] = h.interval(u)
        decided = h.distance_to_boundary(u) > R.EPS
        assert 1.0 - decided.mean() <= R.UNDECIDED_CAP / 3, (head, 1.0 - decided.mean())
        sl = slice(0, 1 << 20)                                           # the float32 twin on the first million
        twin = R.sample_head_f32(logits[lo:hi], R.u_device(k[head][sl]))
        assert np.array_equal(twin[decided[sl]], acts[head][sl][decided[sl]]), head
        a, b = h.neighbours(u[sl], R.EPS)
        assert ((twin >= a) & (twin <= b)).all(), head
    res = R.law_checks(logits, acts["category"], acts["price"], acts["price_offset"], n0, n1)
    bad = {key: v for key, (v, ok) in res.items() if not ok}
    assert not bad, (name, bad)


def test_the_restatement_meets_the_serial_thresholds():
    """the same sample at draws t, t + 1; samples i, i + 1 at one draw; the same (i, draw) at counters c, c + 1: independent categories; equal keys, equal bits"""
    logits = R.law_distributions()["linspace"]
    h = R.Head(logits[:R.N_CAT])
    i = np.arange(R.LAW_N, dtype=np.int64)
    cat = lambda counter, draw: h.interval(R.u_exact(R.draws24(R.rollout_key(R.LAW_SEED, counter, draw), i)["category"]))      # noqa: E731
    base = cat(R.LAW_COUNTER, R.LAW_DRAW)
    assert R.serial_p(base, cat(R.LAW_COUNTER, R.LAW_DRAW + 1)) > R.P_MIN
    assert R.serial_p(base, cat(R.LAW_COUNTER + 1, R.LAW_DRAW)) > R.P_MIN
    assert R.serial_p(base[:-1], base[1:]) > R.P_MIN
    assert np.array_equal(base, cat(R.LAW_COUNTER, R.LAW_DRAW))


def test_random_logits_leave_few_samples_undecided_and_the_float32_twin_agrees():
    """rows of random logits (the scale of a trained policy's, and a sharper one): the float32 twin = the float64 restatement outside the EPS band, share inside under the cap"""
    rng = np.random.default_rng(5)
    for scale in (1.0, 4.0):
        m = 200000
        o = (rng.standard_normal((m, 24)) * scale).astype(np.float32)
        k = R.draws24(R.rollout_key(9, 1, 0), np.arange(m))
        undecided = np.zeros(m, bool)
        for head, lo, hi in R.HEADS:
            h = R.Head(o[:, lo:hi])
            u = R.u_exact(k[head])
            a = h.interval(u)
            dec = h.distance_to_boundary(u) > R.EPS
            undecided |= ~dec
            twin = R.sample_head_f32(o[:, lo:hi], R.u_device(k[head]))
            assert np.array_equal(twin[dec], a[dec]), (scale, head)
            x, y = h.neighbours(u, R.EPS)
            assert ((twin >= x) & (twin <= y)).all(), (scale, head)
        assert undecided.mean() <= R.UNDECIDED_CAP, (scale, undecided.mean())
