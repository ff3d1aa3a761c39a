"""CPU: the label tap's host side (include/cda.h cda_label_*, scripted.mix_draw / mix_played / label_spec, imitate.DaggerBuffer and the --dagger flags).  The mixing
draw against its Python statement and its own domain; label_spec on a hand-written table; every new entry point's argument checks, which answer before a device is
touched; the built kernel's registers; the command line; the aggregate's fill order.  No GPU."""
import ctypes as C
import dataclasses
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gym_continuousdoubleauction_amd import scripted as S  # noqa: E402
from test_scripted_host import IMB, MAKER, PASS, TAKER, view  # noqa: E402

INVALID = -1
NEW_SYMBOLS = ["cda_label_actions", "cda_label_mix_host", "cda_label_tap_attach", "cda_label_tap_attached", "cda_label_tap_detach", "cda_label_tap_epoch",
               "cda_scripted_step_actions"]


@pytest.fixture(scope="module")
def hip_lib():
    import __graft_entry__ as g
    g.build_hip()
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib(), _lib


def mix_host(L, seed, counter, market, draw, agent, q):
    n = len(market)
    market, draw, agent = np.ascontiguousarray(market, np.uint64), np.ascontiguousarray(draw, np.uint32), np.ascontiguousarray(agent, np.uint32)
    out = np.full(n, -7, np.int32)
    rc = L.cda_label_mix_host(seed, counter, market.ctypes.data, draw.ctypes.data, agent.ctypes.data, n, q, out.ctypes.data)
    return rc, out


def test_the_mix_draw_has_a_domain_of_its_own():
    hdr = open(os.path.join(ROOT, "include", "cda_scripted_agents.h")).read()
    assert re.search(r"#define CDA_SCRIPT_MIX_DOMAIN\s+0x%xULL" % S.MIX_DOMAIN, hdr) and S.MIX_DOMAIN == 0xa4093822299f31d0 and S.MIX_DOMAIN != S.DOMAIN
    rng = np.random.default_rng(3)
    for _ in range(500):
        seed, counter, market = int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 40))
        draw, agent = int(rng.integers(0, 1 << 31)), int(rng.integers(0, 16))
        w, wt = S.mix_draw(seed, counter, market, draw, agent), S.taker_draw(seed, counter, market, draw, agent)
        assert w != wt and (w & 0xffffffff) != (wt & 0xffffffff)
    # the construction is taker_draw's: equal after the seeds' domains are swapped
    assert S.mix_draw(5 ^ S.MIX_DOMAIN ^ S.DOMAIN, 2, 11, 3, 4) == S.taker_draw(5, 2, 11, 3, 4)


def test_mix_host_equals_mix_played(hip_lib):
    L, _ = hip_lib
    n = 20000
    rng = np.random.default_rng(17)
    market, draw, agent = rng.integers(0, 1 << 40, n), rng.integers(0, 1 << 31, n), rng.integers(0, 16, n)
    seed, counter = 0xfedcba9876543210, 4321
    for q in (0, 1, 1 << 30, 1 << 31, (1 << 32) - 1, 1 << 32):
        rc, got = mix_host(L, seed, counter, market, draw, agent, q)
        assert rc == 0 and set(got.tolist()) <= {0, 1}
        if q in (1 << 30, 1 << 31):
            assert np.array_equal(got, S.mix_played(seed, counter, market, draw, agent, q)), q
        if q == 0:
            assert not got.any()                                         # never plays
        if q == 1 << 32:
            assert got.all()                                             # always plays
        if q == 1 << 31:
            freq, sd = float(got.mean()), (0.25 / n) ** 0.5
            assert abs(freq - 0.5) <= 4 * sd, (freq, sd)
    assert not S.mix_played(seed, counter, market[:50], draw[:50], agent[:50], 0).any() and S.mix_played(seed, counter, market[:50], draw[:50], agent[:50], 1 << 32).all()
    assert S.mix_q32_of(0.0) == 0 and S.mix_q32_of(1.0) == 1 << 32 and S.mix_q32_of(0.5) == 1 << 31
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            S.mix_q32_of(bad)
    with pytest.raises(ValueError):
        S.mix_played(0, 0, [0], [0], [0], (1 << 32) + 1)


def test_label_spec_on_a_hand_written_table():
    """one market, four slots: 0 labelled by the maker (not attached: mixable), 1 attached AND labelled (the imbalance trader's label; never mixed), 2 attached only,
    3 in neither table"""
    profiles = [MAKER, IMB, dataclasses.replace(TAKER, p_trade_q32=1 << 32)]
    slot_label = np.array([[1, 2, 0, 0]], np.int32)
    slot_script = np.array([[0, 1, 3, 0]], np.int32)
    views = np.zeros((1, 4), S.VIEW_DTYPE)
    views[0, 0] = view(t_step=0, best_bid=100, best_ask=110, tick=1)     # maker, agent 0, even step: bid, inside the wide spread
    views[0, 1] = view(vol=(31, 20))                                     # imbalance 3 : 2 exceeded: buy
    agent = np.arange(4)[None, :]
    for q in (0, 1 << 31, 1 << 32):
        (cat, mean, sigma, price, off), labelled, played = S.label_spec(profiles, slot_label, views, seed=9, counter=2, market=7, draw=3, agent=agent, mix_q32=q,
                                                                        slot_script=slot_script)
        assert labelled.tolist() == [[True, True, False, False]]
        assert (cat[0, 0], float(mean[0, 0]), float(sigma[0, 0]), price[0, 0], off[0, 0]) == (2, 0.25, 0.125, 0, 2)
        assert (cat[0, 1], float(mean[0, 1]), float(sigma[0, 1]), price[0, 1], off[0, 1]) == (1, 0.5, 0.25, 0, 1)
        want0 = int((S.mix_draw(9, 2, 7, 3, 0) & 0xffffffff) < q)
        assert played.tolist() == [[want0, 0, 0, 0]] and played.dtype == np.int32
        # the same numbers straight from the specification of the laws
        direct = S.actions_from_views(profiles, np.array([[0, 1, 0, 0]]), views, 9, 2, 7, 3, agent)
        assert all(np.array_equal(a[labelled].view(np.uint32), b[labelled].view(np.uint32)) for a, b in zip((cat, mean, sigma, price, off), direct))
    # without the attached table slot 1 is mixable too
    _, _, played = S.label_spec(profiles, slot_label, views, seed=9, counter=2, market=7, draw=3, agent=agent, mix_q32=1 << 32)
    assert played.tolist() == [[1, 1, 0, 0]]
    # a value outside 1 .. n_profiles names no profile
    _, labelled, _ = S.label_spec([PASS], np.array([[1, 2, 0, -1]]), views, agent=agent)
    assert labelled.tolist() == [[True, False, False, False]]


def test_the_new_entry_points_are_the_header_s_and_refuse_bad_arguments_before_touching_a_device(hip_lib):
    L, _lib = hip_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cda.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(cda_[a-z_0-9]+)\s*\(", hdr)) if n.startswith("cda_label_") or n == "cda_scripted_step_actions")
    assert declared == NEW_SYMBOLS and [n for n in sorted(_lib.SYMBOLS) if n in NEW_SYMBOLS] == NEW_SYMBOLS
    assert sorted(_lib.IMITATE_SYMBOLS) == ["cda_bc_loss_records", "cda_bc_records"]
    for name in NEW_SYMBOLS:
        assert getattr(L, name).argtypes, name

    def zero(t):
        return None if t is C.c_void_p else 0
    for name in NEW_SYMBOLS:                                             # every argument NULL / 0
        fn = getattr(L, name)
        assert fn(*[zero(t) for t in fn.argtypes]) == (0 if name in ("cda_label_tap_attached", "cda_label_tap_epoch") else INVALID), name
    one, odd2, odd4 = C.c_void_p(64), C.c_void_p(66), C.c_void_p(68)     # non-NULL, never dereferenced: validation fails first (66: not 4-byte, 68: not 8-byte aligned)
    # a zeroed record in the env's place: no device behind it, no market (n_markets 0), nothing attached - whatever passes the pointer checks fails on the range
    blank = C.create_string_buffer(1 << 20)
    env = C.cast(blank, C.c_void_p)

    def attach(e=env, slot=one, prof=one, n=1, mix=one, rows=4, cat=one, mean=one, sigma=one, price=one, off=one, played=one):
        return L.cda_label_tap_attach(e, slot, prof, n, 0, 0, mix, rows, cat, mean, sigma, price, off, played)
    assert attach(e=None) == INVALID and attach(slot=None) == INVALID and attach(prof=None) == INVALID and attach(mix=None) == INVALID
    assert attach(n=0) == INVALID and attach(n=17) == INVALID and attach(rows=0) == INVALID and attach(rows=-1) == INVALID
    assert attach(slot=odd2) == INVALID and attach(prof=odd4) == INVALID and attach(mix=odd4) == INVALID
    for k in ("cat", "mean", "sigma", "price", "off", "played"):
        assert attach(**{k: None}) == INVALID and attach(**{k: odd2}) == INVALID, k
    assert attach() == INVALID                                           # (the blank record has no agents)
    assert L.cda_label_tap_attached(env) == 0 and L.cda_label_tap_epoch(env) == 0          # ... and nothing changed

    def step(e=env, first=0, n=1, ctr=None, t=0, cat=one, rec=None):
        return L.cda_scripted_step_actions(e, first, n, ctr, t, cat, one, one, one, one, None, None, rec, None)
    assert step(e=None) == INVALID and step(t=-1) == INVALID and step(cat=None) == INVALID and step(first=-1) == INVALID and step(n=0) == INVALID
    assert step(rec=odd4) == INVALID and step(ctr=odd4) == INVALID and step() == INVALID        # (no market in the blank record: out of range)

    def label(e=env, first=0, n=1, slot=one, prof=one, n_prof=1, ctr=None, cat=one, off=one):
        return L.cda_label_actions(e, first, n, slot, prof, n_prof, 0, 0, ctr, 0, cat, one, one, one, off, None)
    assert label(e=None) == INVALID and label(slot=None) == INVALID and label(prof=None) == INVALID and label(n_prof=0) == INVALID and label(n_prof=17) == INVALID
    assert label(slot=odd2) == INVALID and label(prof=odd4) == INVALID and label(ctr=odd4) == INVALID and label(cat=None) == INVALID and label(off=odd2) == INVALID
    assert label(first=-1) == INVALID and label(n=0) == INVALID and label() == INVALID
    assert L.cda_label_tap_detach(None) == INVALID

    rc, out = mix_host(L, 1, 2, [3], [4], [5], (1 << 32) + 1)
    assert rc == INVALID and out[0] == -7
    ok = np.zeros(1, np.uint64)
    assert L.cda_label_mix_host(0, 0, None, ok.ctypes.data, ok.ctypes.data, 1, 0, ok.ctypes.data) == INVALID
    assert L.cda_label_mix_host(0, 0, ok.ctypes.data, ok.ctypes.data, ok.ctypes.data, -1, 0, ok.ctypes.data) == INVALID
    assert L.cda_label_mix_host(0, 0, ok.ctypes.data, ok.ctypes.data, ok.ctypes.data, 1, 0, None) == INVALID


def test_the_label_kernel_exists_once_and_keeps_everything_in_registers():
    from test_kernel_resources import _kernels
    ks, bodies = _kernels()
    inst = {n: v for n, v in ks.items() if "k_script_label" in n}
    assert len(inst) == 1, sorted(inst)
    (n, v), = inst.items()
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 128, (n, v)
    body = bodies[n]
    assert not any("global_atomic" in l or "flat_atomic" in l for l in body), n
    assert not any("scratch_" in l or "ds_read" in l or "ds_write" in l for l in body), n          # no scratch, no LDS memory (the shuffles' ds_bpermute holds none)
    assert not any(stem in n for stem in ("k_script_actions", "k_stepILb", "k_tstepILb", "k_policy_step", "k_tape_"))
    assert len([k for k in ks if "k_script_actions" in k]) == 1          # the sibling is still there, once


def test_the_command_line():
    from gym_continuousdoubleauction_amd import imitate
    a = imitate.main(["--dagger", "--label-expert", "maker", "--opponent", "taker", "--opponent", "imbalance:depth_levels=3", "--beta", "0.75", "--beta-decay", "0.25",
                      "--aggregate", "3", "--iters", "5"], parse_only=True)
    assert a.dagger and a.label_expert == "maker" and a.opponent == ["taker", "imbalance:depth_levels=3"] and a.beta == 0.75 and a.beta_decay == 0.25
    assert a.aggregate == 3 and a.iters == 5
    d = imitate.main(["--dagger", "--label-expert", "maker"], parse_only=True)
    assert d.opponent is None and d.beta == 1.0 and d.beta_decay == 0.5 and d.aggregate is None
    for bad in (["--dagger"], ["--dagger", "--opponent", "taker"], ["--dagger", "--label-expert", "maker", "--expert", "maker"],
                ["--dagger", "--label-expert", "maker", "--demos", "x.npz"], ["--label-expert", "maker", "--expert", "maker"], ["--expert", "maker", "--opponent", "taker"]):
        with pytest.raises(SystemExit):
            imitate.main(bad, parse_only=True)
    # the flags of before, as before
    e = imitate.main(["--expert", "maker", "--iters", "2"], parse_only=True)
    assert not e.dagger and e.expert == ["maker"] and e.label_expert is None
    with pytest.raises(SystemExit):
        imitate.main([], parse_only=True)


def _block(rows, A, obs_dim, n_markets, seed):
    from gym_continuousdoubleauction_amd.imitate import Demonstrations
    g = torch.Generator().manual_seed(seed)
    rec = torch.randn((rows, A, 8), generator=g)
    rec[..., 5] = (torch.rand((rows, A), generator=g) < 0.6).float() * torch.randint(1, 4, (rows, A), generator=g).float()      # weights 0 .. 3
    return Demonstrations(torch.randn((rows, obs_dim), generator=g), rec, n_markets)


def test_the_dagger_buffer_fills_in_order_and_wraps():
    from gym_continuousdoubleauction_amd.imitate import DaggerBuffer, Demonstrations
    rows, A, obs_dim, n_markets, K = 12, 3, 5, 4, 3
    buf = DaggerBuffer(K, rows, A, obs_dim, n_markets)
    d0 = buf.demos
    assert d0.R == K * rows and d0.weight_sum == 0.0 and d0.count == 0 and buf.filled == 0
    with pytest.raises(ValueError):
        d0.loss_scale                                                    # nothing counted yet
    blocks = [_block(rows, A, obs_dim, n_markets, s) for s in range(5)]
    held = [None] * K
    for j, blk in enumerate(blocks):
        assert buf.add(blk) == j % K                                     # fill order, then wrap-around: the oldest block goes
        held[j % K] = blk
        d = buf.demos
        assert buf.filled == min(j + 1, K) and d.R == K * rows and d.A == A and d.n_markets == n_markets
        for q in range(K):
            sl = slice(q * rows, (q + 1) * rows)
            if held[q] is None:                                          # not yet filled: weight 0 everywhere
                assert float(d.rec[sl].abs().sum()) == 0.0 and float(d.obs[sl].abs().sum()) == 0.0
            else:
                assert torch.equal(d.obs[sl], held[q].obs) and torch.equal(d.rec[sl], held[q].rec)
        live = [b for b in held if b is not None]
        cat = Demonstrations(torch.cat([b.obs for b in live]), torch.cat([b.rec for b in live]), n_markets)
        assert d.weight_sum == pytest.approx(cat.weight_sum, rel=0, abs=1e-9) and d.count == cat.count
        # ... and they are what the records themselves say
        assert d.weight_sum == float(d.rec[..., 5].double().sum()) and d.count == int((d.rec[..., 5] > 0).sum())
        assert d.loss_scale == pytest.approx(K * rows * A / cat.weight_sum)
    with pytest.raises(ValueError):
        buf.add(_block(rows + n_markets, A, obs_dim, n_markets, 9))
    with pytest.raises(ValueError):
        DaggerBuffer(0, rows, A, obs_dim, n_markets)
    with pytest.raises(ValueError):
        DaggerBuffer(2, rows + 1, A, obs_dim, n_markets)
