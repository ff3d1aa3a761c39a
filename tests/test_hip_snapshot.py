"""GPU: device snapshots of whole markets (include/cda.h cda_snapshot_*, csrc/cda_snapshot.inc; CDAVecEnv.snapshot / restore).

A snapshot taken, the env stepped on, the snapshot restored and the same steps taken again must give the same bits: observations, rewards, flags,
info tensors, state dumps, whole books (HBM rings included, wrapped windows too) and the episode-metric tallies.  Restores into other envs (forks,
other ring sizes) continue identically; restores that cannot fit are refused before any byte of the env is written."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_continuousdoubleauction_amd import _capi as K
from gym_continuousdoubleauction_amd._lib import CDAError, lib
from gym_continuousdoubleauction_amd.vec_env import CDAVecEnv

pytestmark = pytest.mark.gpu


def _actions(rng, n, a, dev):
    cat = torch.from_numpy(rng.integers(0, 9, (n, a)).astype(np.int32)).to(dev)
    mean = torch.from_numpy(rng.uniform(-1, 1, (n, a)).astype(np.float32)).to(dev)
    sigma = torch.from_numpy(rng.uniform(0, 1, (n, a)).astype(np.float32)).to(dev)
    price = torch.from_numpy(rng.integers(0, 10, (n, a)).astype(np.int32)).to(dev)
    off = torch.from_numpy(rng.integers(0, 3, (n, a)).astype(np.int32)).to(dev)
    return cat, mean, sigma, price, off


def _run(env, acts):
    out = []
    for a in acts:
        obs, rew, term, trunc, info = env.step(*a)
        rec = [obs.clone(), rew.clone(), term.clone(), trunc.clone()]
        rec += [v.clone() for _, v in sorted((info or {}).items())]
        out.append(rec)
    torch.cuda.synchronize()
    return out


def _same_runs(x, y):
    assert len(x) == len(y)
    for t, (a, b) in enumerate(zip(x, y)):
        for k, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), (t, k)


def _dump(env, markets):
    return [(bytes(env.get_state(i)), env.get_book(i)) for i in markets]


def _same_dumps(x, y):
    for (s1, (b1, a1)), (s2, (b2, a2)) in zip(x, y):
        assert s1 == s2 and np.array_equal(b1, b2) and np.array_equal(a1, a2)


def _round_trip(n, a, shape):
    cfg = dict({"num_of_agents": a, "init_cash": 1000000, "max_step": 320, "is_render": False, "auto_reset": True}, **shape)
    env = CDAVecEnv(cfg, n_markets=n, device="cuda:0", with_info=True)
    env.reset(seed=17)
    env.enable_episode_metrics(True)
    env.run_random(300, action_seed=5)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    acts = [_actions(rng, n, a, env.device) for _ in range(40)]             # crosses the episode end at step 320: auto resets + credited episodes
    obs0 = env.obs.clone()
    snap = env.snapshot()
    # compact: the header, the offset table and per market one 256-byte aligned section = record + 32 bytes of ring metadata + the metric rows (csrc/cda_snapshot.inc;
    # random agents' books stay inside the tile, so no ring window follows) - at 4 agents well below the record + 4096 bytes
    pad = lambda x: -(-x // 256) * 256      # noqa: E731
    section = pad(env.state_bytes_per_market() + 32 + 8 * (a * K.EM_AGENT_FIELDS + K.EM_ENV_FIELDS))
    assert len(snap) == n and snap.nbytes == 256 + pad(8 * (n + 1)) + n * section and (a > 4 or snap.nbytes < n * (env.state_bytes_per_market() + 4096))
    sample = list(range(0, n, 97 if n > 97 else 7))
    first = _run(env, acts)
    dump1 = _dump(env, sample)
    em1 = [t.clone() for t in env.collect_episode_metrics()]
    assert em1[1][K.EM_ENV_EPISODES].item() > 0
    env.obs.fill_(float("nan"))
    env.restore(snap)
    assert torch.equal(env.obs.view(torch.int32), obs0.view(torch.int32))     # re-emitted from the history frames
    again = env.snapshot()
    assert torch.equal(again.blob, snap.blob)                                  # byte for byte
    second = _run(env, acts)
    _same_runs(first, second)
    _same_dumps(dump1, _dump(env, sample))
    em2 = env.collect_episode_metrics()
    assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(em1, em2))
    env.close()


def test_round_trip_is_bit_exact():
    _round_trip(1024, 4, {})


@pytest.mark.parametrize("a,n_hist", [(3, 1), (16, 16)])
def test_round_trip_is_bit_exact_at_the_smallest_and_the_largest_record(a, n_hist):
    """test_round_trip_is_bit_exact where the section sizes, the metric rows and the re-emitted observation are smallest and largest: 3 agents at history depth 1,
    16 agents (tile 512) at depth 16; 96 markets"""
    _round_trip(96, a, {"n_hist": n_hist})


def _deep_env(tile, spill, n=3):
    cfg = {"num_of_agents": 4, "init_cash": 10 ** 12, "max_step": 4096, "is_render": False, "book_capacity": tile, "book_spill": spill, "auto_reset": True}
    return CDAVecEnv(cfg, n_markets=n, device="cuda:0", with_info=True)


def _ring_words(env, snap):
    """(bid count, bid base, ring size) of every market as the blob holds them (its section's metadata behind the record)"""
    raw = snap.blob.cpu().numpy()
    stride = env.state_bytes_per_market()
    out = []
    for k in range(len(snap)):
        off = int(raw[256 + 8 * k: 264 + 8 * k].view(np.int64)[0])
        meta = raw[off + stride: off + stride + 32].view(np.int32)
        out.append((int(meta[2]), int(meta[4]), int(meta[6])))
    return out


def _grow_deep_books(env, n_orders):
    """bids at ever worse prices: once the tile is full its worst orders are evicted to the head of the ring (base < 0, slots near spill_cap) and every
    later, still worse bid is appended behind them - the window runs past the ring's last slot and wraps"""
    for m in range(env.n_markets):
        for k in range(n_orders):
            env.place_order(m, k % 4, K.T_LIMIT, K.S_BID, 1 + k % 3, 20000 - k - 3 * m)
        for k in range(n_orders // 3):
            env.place_order(m, (k + 1) % 4, K.T_LIMIT, K.S_ASK, 2, 30000 + k)


@pytest.mark.parametrize("tile", [256, 512])
def test_deep_books_restore_into_another_ring(tile):
    src = _deep_env(tile, 1024)
    src.reset(seed=4)
    _grow_deep_books(src, 1100 if tile == 256 else 1300)
    for m in range(src.n_markets):
        assert len(src.get_book(m, 0)) > tile + 600
    snap = src.snapshot()
    for m, (n0, base0, cap) in enumerate(_ring_words(src, snap)):           # the bid window really wraps: it starts near the ring's end and runs past it
        assert cap == 1024 and n0 > 600 and (base0 & (cap - 1)) + n0 > cap, (m, n0, base0)
    # the same ring size: the window goes back to its saved slots (restore into the env itself, after it has moved on)
    books0 = [src.get_book(m) for m in range(src.n_markets)]
    rng0 = np.random.default_rng(21)
    acts0 = [_actions(rng0, src.n_markets, 4, src.device) for _ in range(25)]
    ahead = _run(src, acts0)
    dump_ahead = _dump(src, range(src.n_markets))
    src.restore(snap)
    for m in range(src.n_markets):
        for sd in (0, 1):
            assert np.array_equal(src.get_book(m, sd), books0[m][sd]), (m, sd)
    assert torch.equal(src.snapshot().blob, snap.blob)                     # the saved bases included: byte for byte
    _same_runs(ahead, _run(src, acts0))
    _same_dumps(dump_ahead, _dump(src, range(src.n_markets)))
    src.restore(snap)
    bigger = _deep_env(tile, 4096)
    bigger.reset(seed=99)
    bigger.restore(snap)
    for m in range(src.n_markets):
        for sd in (0, 1):
            assert np.array_equal(src.get_book(m, sd), bigger.get_book(m, sd)), (m, sd)
    assert bigger.snapshot().nbytes == snap.nbytes
    rng = np.random.default_rng(8)
    acts = [_actions(rng, src.n_markets, 4, src.device) for _ in range(30)]
    a, b = _run(src, acts), _run(bigger, acts)
    _same_runs(a, b)
    _same_dumps(_dump(src, range(src.n_markets)), _dump(bigger, range(src.n_markets)))
    # a ring too small for the live window: refused, the target unchanged
    small = _deep_env(tile, 256)
    small.reset(seed=1)
    before = _dump(small, range(small.n_markets))
    with pytest.raises(CDAError):
        small.restore(snap)
    _same_dumps(before, _dump(small, range(small.n_markets)))
    for e in (src, bigger, small):
        e.close()


def test_fork_into_an_env_of_another_size():
    cfg = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 200, "is_render": False, "auto_reset": True}
    a = CDAVecEnv(cfg, n_markets=64, device="cuda:0", with_info=True)
    b = CDAVecEnv(cfg, n_markets=40, device="cuda:0", with_info=True)
    a.reset(seed=2); b.reset(seed=500)
    a.run_random(120, action_seed=1); b.run_random(50, action_seed=2)
    torch.cuda.synchronize()
    obs_a = a.obs.clone()
    snap = a.snapshot(8, 16)
    b.restore(snap, first=20)
    assert torch.equal(b.obs[20:36].view(torch.int32), obs_a[8:24].view(torch.int32))
    rng = np.random.default_rng(6)
    for t in range(60):
        acts_a = _actions(rng, 64, 4, a.device)
        acts_b = [torch.zeros((40, 4), dtype=x.dtype, device=x.device) for x in acts_a]
        for x, y in zip(acts_a, acts_b):
            y[20:36] = x[8:24]
        oa, ra, ta, tra, _ = a.step(*acts_a)
        ob, rb, tb, trb, _ = b.step(*acts_b)
        assert torch.equal(oa[8:24].view(torch.int32), ob[20:36].view(torch.int32)), t
        assert torch.equal(ra[8:24].view(torch.int64), rb[20:36].view(torch.int64)), t
        assert torch.equal(ta[8:24], tb[20:36]) and torch.equal(tra[8:24], trb[20:36])
    a.close(); b.close()


@pytest.mark.parametrize("change", ["num_of_agents", "n_hist", "book_capacity", "max_step", "tick_size", "metrics", "header"])
def test_refusals_leave_the_env_untouched(change):
    base = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 200, "is_render": False, "auto_reset": True}
    src = CDAVecEnv(base, n_markets=8, device="cuda:0", with_info=False)
    src.reset(seed=1)
    src.run_random(30, action_seed=1)
    snap = src.snapshot()
    tcfg = dict(base)
    if change == "num_of_agents":
        tcfg["num_of_agents"] = 5
    elif change == "n_hist":
        tcfg["n_hist"] = 2
    elif change == "book_capacity":
        tcfg["book_capacity"] = 512
    elif change == "max_step":
        tcfg["max_step"] = 201
    elif change == "tick_size":
        tcfg["tick_size"] = 2
    dst = CDAVecEnv(tcfg, n_markets=8, device="cuda:0", with_info=False)
    dst.reset(seed=7)
    dst.run_random(10, action_seed=4)
    if change == "metrics":
        dst.enable_episode_metrics(True)
    torch.cuda.synchronize()
    before = _dump(dst, range(8))
    if change == "header":
        snap.blob[0] ^= 0xFF                                                   # the magic word
    # the C entry point itself refuses (the Python side checks first and names the field)
    rc = lib().cda_snapshot_restore(dst._h, 0, snap.blob.data_ptr(), snap.nbytes, 0, 8, dst.obs.data_ptr(), None)
    assert rc == -1
    with pytest.raises((ValueError, CDAError)):
        dst.restore(snap)
    _same_dumps(before, _dump(dst, range(8)))
    src.close(); dst.close()


def test_bad_ranges_are_refused():
    env = CDAVecEnv({"num_of_agents": 4, "max_step": 64, "is_render": False}, n_markets=4, device="cuda:0", with_info=False)
    env.reset(seed=0)
    snap = env.snapshot()
    off = torch.zeros(8, dtype=torch.int64, device=env.device)
    L = lib()
    assert L.cda_snapshot_offsets(env._h, 2, 3, off.data_ptr(), None) == -1
    assert L.cda_snapshot_offsets(env._h, 0, 0, off.data_ptr(), None) == -1
    assert L.cda_snapshot_offsets(env._h, 0, 4, None, None) == -1
    assert L.cda_snapshot_pack(env._h, 0, 4, off.data_ptr(), None, 4096, None) == -1
    assert L.cda_snapshot_restore(env._h, 0, snap.blob.data_ptr(), snap.nbytes, 2, 3, None, None) == -1     # beyond the blob's markets
    assert L.cda_snapshot_restore(env._h, 3, snap.blob.data_ptr(), snap.nbytes, 0, 2, None, None) == -1     # beyond the env's markets
    assert L.cda_snapshot_restore(env._h, 0, snap.blob.data_ptr(), 100, 0, 1, None, None) == -1
    with pytest.raises(ValueError):
        env.snapshot(3, 2)
    env.close()


@pytest.mark.parametrize("n", [4096, 2500])
def test_checkpoint_size_snapshot_equals_its_ranges_and_restores_every_market(n):
    """A checkpoint's snapshot of a whole env of 4096 / 2500 markets: k_snap_offsets' threads then size 4 / 3 markets each.  Deep books (HBM ring in use) grown
    in markets on both sides of the chunk boundaries: the offset table and every section equal those of the snapshots of ranges of at most 1024 markets (one
    market per thread), and a fresh env restored from it holds every market's state and book and steps on bit for bit."""
    cfg = {"num_of_agents": 4, "init_cash": 10 ** 12, "max_step": 4096, "is_render": False, "book_capacity": 256, "book_spill": 1024, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=n, device="cuda:0", with_info=False)
    env.reset(seed=n)
    env.run_random(12, action_seed=3)
    deep = [0, 2, 3, 4, 1022, 1023, 1024, n - 1]                        # (chunks of 4 / 3 markets: 2 | 3, 3 | 4, 1022 | 1023, 1023 | 1024 are boundaries)
    for m in deep:                                                       # _grow_deep_books' orders, in these markets only
        for k in range(1100):
            env.place_order(m, k % 4, K.T_LIMIT, K.S_BID, 1 + k % 3, 20000 - k - 3 * m)
        for k in range(1100 // 3):
            env.place_order(m, (k + 1) % 4, K.T_LIMIT, K.S_ASK, 2, 30000 + k)
    torch.cuda.synchronize()
    snap = env.snapshot()
    assert len(snap) == n
    raw = snap.blob.cpu().numpy()
    off = raw[256:256 + 8 * (n + 1)].view(np.int64)
    assert off[n] == snap.nbytes and (np.diff(off) > 0).all()
    stride = env.state_bytes_per_market()
    for m in deep:                                                       # the ring holds a live window in every deep market, none in the others
        meta = raw[off[m] + stride: off[m] + stride + 32].view(np.int32)
        # (the 366 asks above every bid always rest: the ask ring holds > 100; the random agents' asks absorb a market-dependent share of the bids)
        assert meta[3] > 100 and meta[2] >= 0, (m, meta.tolist(), len(env.get_book(m, 0)), len(env.get_book(m, 1)), env.book_capacity, env.book_spill)
    sizes = np.diff(off)
    assert len(set(sizes[np.setdiff1d(np.arange(n), deep)].tolist())) == 1 and (sizes[deep] > sizes[5]).all()
    for f in range(0, n, 1024):
        k = min(1024, n - f)
        part = env.snapshot(f, k)
        r = part.blob.cpu().numpy()
        o = r[256:256 + 8 * (k + 1)].view(np.int64)
        assert np.array_equal(np.diff(o), sizes[f:f + k]), f
        assert np.array_equal(r[o[0]:o[k]], raw[off[f]:off[f + k]]), f                 # the sections, byte for byte
    fresh = CDAVecEnv(cfg, n_markets=n, device="cuda:0", with_info=False)
    fresh.reset(seed=1)
    fresh.restore(snap)
    for m in range(n):
        assert bytes(fresh.get_state(m)) == bytes(env.get_state(m)), m
        (b1, a1), (b2, a2) = fresh.get_book(m), env.get_book(m)
        assert np.array_equal(b1, b2) and np.array_equal(a1, a2), m
    assert torch.equal(fresh.snapshot().blob, snap.blob)
    rng = np.random.default_rng(n)
    acts = [_actions(rng, n, 4, env.device) for _ in range(10)]
    _same_runs(_run(env, acts), _run(fresh, acts))
    assert torch.equal(fresh.snapshot().blob, env.snapshot().blob)
    env.close(); fresh.close()
