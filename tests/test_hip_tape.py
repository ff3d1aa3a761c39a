"""GPU: the trade tape (include/cda.h cda_tape_*; CDAVecEnv.enable_tape / drain_tape / tape_last; CDAEnv.tape) against the REFERENCE's OrderBook.tape, through the
fixtures tests/golden/tape_<trace>.npz (tests/golden/make_tape_goldens.py replays the stored inputs of trace_<trace>.npz through the reference and stores its tape).
Integers only: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import golden_util as G

pytestmark = pytest.mark.gpu

FIXTURES = ["aggr_s23", "A8_s3", "tick5_s301", "A16_aggr_s71", "reset_s51", "bankrupt_s61", "permshuf_s93", "perm8_s92", "bigbook8_waves_s203"]


def _fixture(name):
    with np.load(os.path.join(G.GOLD, f"tape_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def _tape_env(config, n, capacity, **kw):
    from hip_env import HipEnv
    env = HipEnv(config, n_markets=n, **kw)
    env.env.enable_tape(capacity)
    return env


class _Counting:
    """a HipEnv whose step() also notes every market's n_episode (golden_util.run_group drives it and checks everything else it always checks)"""

    def __init__(self, env):
        self._e, self.n_episode = env, []

    def __getattr__(self, k):
        return getattr(self._e, k)

    def step(self, *a):
        out = self._e.step(*a)
        self.n_episode.append(self._e.env.tape_counts()["n_episode"].cpu().numpy().copy())
        return out


def _replay(name, capacity=4096, state_every=16, metrics=False):
    rec, fx = G.load(name), _fixture(name)
    env = _Counting(_tape_env(rec["config"], 1, capacity))
    if metrics:                                                                       # the tape-writing instances then tally (the market's ST_EP_ON bit)
        env.env.enable_episode_metrics(True)
    G.run_group(env, [rec], state_every=state_every)
    return env, rec, fx


@pytest.mark.parametrize("name", FIXTURES)
def test_every_fixture_replays_to_the_reference_tape(name):
    assert_fixture_replays_to_the_reference_tape(name)


def assert_fixture_replays_to_the_reference_tape(name, metrics=False):
    """(tests/test_hip_step_variants.py replays the fixtures once more with the episode metrics on)"""
    env, rec, fx = _replay(name, state_every=64 if name.startswith("bigbook") else 16, metrics=metrics)
    got_len = np.array([c[0] for c in env.n_episode], np.int32)
    assert np.array_equal(got_len, fx["tape_len"]), (name, np.flatnonzero(got_len != fx["tape_len"])[:8])
    records, offsets, dropped = env.env.drain_tape()
    rows = records.cpu().numpy()
    assert offsets.cpu().tolist() == [0, len(fx["rows"])] and dropped.cpu().tolist() == [0]
    assert rows.shape == fx["rows"].shape
    for j, f in enumerate(("time", "price", "quantity", "counter_id", "counter_order_id", "counter_left", "init_id", "sides_step")):
        bad = np.flatnonzero(rows[:, j] != fx["rows"][:, j])
        assert bad.size == 0, (name, f, bad[:8], rows[bad[:4]], fx["rows"][bad[:4]])
    counts = {k: v.cpu().numpy() for k, v in env.env.tape_counts().items()}
    assert counts["n_total"][0] == len(fx["rows"]) and counts["episode"][0] == 1 + len(rec["resets"]) and counts["partial"][0] == 0      # (the first reset counts too)
    env.close()


def _actions(rng, n, a):
    return (rng.integers(0, 9, (n, a)).astype(np.int32), rng.uniform(-1, 1, (n, a)).astype(np.float32),
            rng.uniform(0, 1, (n, a)).astype(np.float32), rng.integers(0, 10, (n, a)).astype(np.int32),
            rng.integers(0, 3, (n, a)).astype(np.int32))


@pytest.mark.parametrize("n,a,steps", [(1024, 4, 256), (256, 8, 128), (64, 16, 64)])
def test_the_tape_observes_and_never_steers(n, a, steps):
    from hip_env import HipEnv
    cfg = {"num_of_agents": a, "init_cash": 1000000, "max_step": steps, "is_render": False}
    off, on = HipEnv(cfg, n), _tape_env(cfg, n, 256)
    seeds = np.arange(500, 500 + n, dtype=np.uint64)
    assert np.array_equal(off.reset(seeds).view(np.uint32), on.reset(seeds).view(np.uint32))
    rng = np.random.default_rng(77)
    for t in range(steps):
        acts = _actions(rng, n, a)
        r0, r1 = off.step(*acts), on.step(*acts)
        assert np.array_equal(r0[0].view(np.uint32), r1[0].view(np.uint32)), f"obs, step {t}"
        assert np.array_equal(r0[1].view(np.uint64), r1[1].view(np.uint64)), f"reward, step {t}"
        assert np.array_equal(r0[2], r1[2]) and np.array_equal(r0[3], r1[3]), f"flags, step {t}"
        for k in r0[4]:
            assert np.array_equal(np.ascontiguousarray(r0[4][k]).view(np.uint8), np.ascontiguousarray(r1[4][k]).view(np.uint8)), f"info.{k}, step {t}"
    for i in list(range(0, n, max(1, n // 48))) + [n - 1]:
        assert bytes(off.get_state(i)) == bytes(on.get_state(i)), f"state of market {i}"
    assert int(on.env.tape_counts()["n_total"].sum()) > n                              # ... and it did observe
    off.close(); on.close()


def test_ring_cursors_and_capacity():
    name = "aggr_s23"
    env, rec, fx = _replay(name, capacity=64)
    K = len(fx["rows"])
    assert K > 300
    last, cnt = env.env.tape_last(64)
    assert cnt.cpu().tolist() == [64] and np.array_equal(last[0].cpu().numpy(), fx["rows"][-64:])
    last, cnt = env.env.tape_last(7)
    assert cnt.cpu().tolist() == [7] and np.array_equal(last[0].cpu().numpy(), fx["rows"][-7:])
    records, offsets, dropped = env.env.drain_tape()                                   # the env's cursor is still 0
    assert dropped.cpu().tolist() == [K - 64] and np.array_equal(records.cpu().numpy(), fx["rows"][-64:])
    records, offsets, dropped = env.env.drain_tape()                                   # ... and now at n_total
    assert records.shape[0] == 0 and offsets.cpu().tolist() == [0, 0] and dropped.cpu().tolist() == [0]
    env.close()
    # drained every 7 steps through a ring that is large enough, the pieces are the tape
    r = G.load(name)
    env = _tape_env(r["config"], 1, 128)
    env.reset(seeds=np.array([int(r["seed"])], np.uint64))
    parts = []
    for t in range(r["cat"].shape[0]):
        env.step(r["cat"][t][None], r["mean"][t][None], r["sigma"][t][None], r["price"][t][None], r["off"][t][None], r["present"][t][None])
        if t % 7 == 6:
            rows, _, dropped = env.env.drain_tape()
            assert dropped.cpu().tolist() == [0]
            parts.append(rows.cpu().numpy())
    parts.append(env.env.drain_tape()[0].cpu().numpy())
    assert np.array_equal(np.concatenate(parts), fx["rows"])
    for bad in (0, 3, 100, -8):
        with pytest.raises(ValueError):
            env.env.enable_tape(bad)
    env.env.disable_tape()
    assert not env.env.tape_enabled
    with pytest.raises(RuntimeError, match="enable_tape"):
        env.env.drain_tape()
    env.close()


def _step_tape(env, acts_of, steps, via=None):
    for t in range(steps):
        (via or env.step)(*acts_of(t))
    rows, off, dropped = env.drain_tape()
    assert int(dropped.sum()) == 0
    return rows.cpu().numpy(), off.cpu().numpy()


@pytest.mark.parametrize("cap", [256, 512])
def test_one_launch_or_many_record_the_same_tape(cap):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a, steps = 96, 4, 48
    cfg = {"num_of_agents": a, "init_cash": 1000000, "max_step": steps, "is_render": False, "book_capacity": cap}
    ref = CDAVecEnv(cfg, n)
    ref.enable_tape(512)
    ref.reset(seed=900)
    acts_of = lambda t: ref.random_actions(t, action_seed=11)      # noqa: E731
    want, want_off = _step_tape(ref, acts_of, steps)
    assert len(want) > n
    # four groups on four streams
    grp = CDAVecEnv(cfg, n, groups=4)
    grp.enable_tape(512)
    grp.reset(seed=900)
    got, off = _step_tape(grp, acts_of, steps)
    assert np.array_equal(off, want_off) and np.array_equal(got, want)
    # a captured step graph, replayed
    cap_env = CDAVecEnv(cfg, n, with_info=False)
    cap_env.enable_tape(512)
    cap_env.reset(seed=900)
    dev = cap_env.device
    bufs = [torch.zeros((n, a), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.float32, torch.int32, torch.int32)]
    cap_env.step(*[torch.from_numpy(x).to(dev) for x in acts_of(0)])                  # (warm-up outside the capture; step 0 is then replayed from a fresh reset)
    cap_env.reset(seed=900)
    cap_env.enable_tape(512)
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    with torch.cuda.graph(g, stream=s):
        cap_env.step(*bufs)
    cap_env.reset(seed=900)                                                           # (the capture ran nothing: the counters are still empty)
    assert int(cap_env.tape_counts()["n_total"].sum()) == 0
    for t in range(steps):
        for b, x in zip(bufs, acts_of(t)):
            b.copy_(torch.from_numpy(x))
        g.replay()
    torch.cuda.synchronize()
    got, off = cap_env.drain_tape()[:2]
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(got.cpu().numpy(), want)
    # the whole episode in ONE launch of the random-agent kernel
    run = CDAVecEnv(cfg, n, with_info=False)
    run.enable_tape(512)
    run.reset(seed=900)
    run.run_random(steps, action_seed=11)
    got, off = run.drain_tape()[:2]
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(got.cpu().numpy(), want)
    for e in (ref, grp, cap_env, run):
        e.close()


def test_auto_reset_counts_episodes_and_keeps_the_finished_one_readable():
    """reset_s51 is 3 x 40 steps with explicit resets; its first reset keeps the RNG stream (seed=None) - exactly what the device-side auto reset does - so with
    auto_reset the first TWO episodes are the fixture's.  Its third was re-seeded by the trace, which an auto reset never does: over steps 80 .. 119 the counters
    are checked against the tape itself (n_total grows by what n_episode counts, nothing is dropped, the drained rows are the third episode's), not the fixture."""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    r, fx = G.load("reset_s51"), _fixture("reset_s51")
    ep_rows = [fx["rows"][fx["episode"] == k] for k in range(3)]
    two = len(ep_rows[0]) + len(ep_rows[1])
    for with_info in (False, True):                                                   # the in-kernel reset / the reset pass behind a step with info tensors
        env = CDAVecEnv(dict(r["config"], auto_reset=True), 1, with_info=with_info)
        env.enable_tape(256)
        env.reset(seed=np.array([int(r["seed"])], np.uint64))
        prev_total, third = 0, 0
        for t in range(120):
            env.step(r["cat"][t][None], r["mean"][t][None], r["sigma"][t][None], r["price"][t][None], r["off"][t][None], r["present"][t][None])
            c = {k: int(v[0]) for k, v in env.tape_counts().items()}
            ended = (t + 1) % 40 == 0                                                 # this step ended an episode: the market has been reset behind it
            assert c["episode"] == 1 + (t + 1) // 40 and c["partial"] == 0, (t, c)
            assert c["n_total"] >= prev_total, (t, c)
            if t < 80:
                assert c["n_episode"] == (0 if ended else int(fx["tape_len"][t])), (t, c)
                assert c["n_total"] == (len(ep_rows[0]) if t >= 40 else 0) + int(fx["tape_len"][t]), (t, c)
            else:                                                                     # the third episode: n_total carried across two resets
                third += c["n_total"] - prev_total
                assert c["n_total"] == two + third and c["n_episode"] == (0 if ended else third), (t, c)
            prev_total = c["n_total"]
            if t == 39:                                                               # the episode that just ended is still in the ring
                rows = env.drain_tape()[0].cpu().numpy()
                assert np.array_equal(rows, ep_rows[0])
            if t == 79:
                rows = env.drain_tape()[0].cpu().numpy()
                assert np.array_equal(rows, ep_rows[1])
        assert c["episode"] == 4 and c["n_episode"] == 0 and third > 0
        rows, off, dropped = env.drain_tape()                                         # the cursor went across two finished episodes
        rows = rows.cpu().numpy()
        assert dropped.cpu().tolist() == [0] and off.cpu().tolist() == [0, third] and len(rows) == third
        assert ((rows[:, 7] >> 2) < 40).all() and (np.diff(rows[:, 7] >> 2) >= 0).all() and (np.diff(rows[:, 0]) >= 0).all()      # one episode: steps and LOB time restart at 0 and only grow
        last, cnt = env.tape_last(8)                                                  # the current (fourth) episode is empty
        assert cnt.cpu().tolist() == [0] and int(last.abs().sum()) == 0
        env.close()


def test_place_order_records_its_fills():
    """The one-order hook (cda_place_order) on a tape-enabled env: the decoded orders of the first steps of a fixture's trace, placed one by one in the trace's
    execution order, fill exactly as the reference filled them - every field of the record but the step index (the hook takes no env step: t stays 0)."""
    name, steps = "aggr_s23", 48
    r, fx = G.load(name), _fixture(name)
    env = _tape_env(r["config"], 1, 1024)
    env.reset(seeds=np.array([int(r["seed"])], np.uint64))
    for t in range(steps):
        for tr in r["exec_order"][t][: int(r["n_acts"][t])]:
            tr = int(tr)
            typ, side, size, price = (int(r[k][t, tr]) for k in ("dec_type", "dec_side", "dec_size", "dec_price"))
            assert typ in (0, 1, 2, 3) and side in (0, 1)
            env.place_order(0, tr, typ, side, size, price if typ != 0 else 1)
        env.mark_to_mkt(0)
        assert int(env.env.tape_counts()["n_episode"][0]) == int(fx["tape_len"][t]), t
    K = int(fx["tape_len"][steps - 1])
    assert K > 40
    rows = env.env.drain_tape()[0].cpu().numpy()
    want = fx["rows"][:K].copy()
    want[:, 7] &= 3
    assert np.array_equal(rows, want)
    env.close()


def test_restore_marks_the_tail_partial_until_the_next_reset():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a = 8, 4
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 256, "is_render": False}, n)
    env.enable_tape(1024)
    env.reset(seed=31)
    counts = lambda: {k: v.cpu().numpy().copy() for k, v in env.tape_counts().items()}      # noqa: E731
    for t in range(24):
        env.step(*env.random_actions(t, action_seed=5))
    snap = env.snapshot(2, 4)                                                         # markets 2 .. 5
    for t in range(24, 40):
        env.step(*env.random_actions(t, action_seed=5))
    c1 = counts()
    assert (c1["n_total"] > 0).all() and (c1["partial"] == 0).all() and np.array_equal(c1["n_total"], c1["n_episode"])
    env.restore(snap, first=2)
    c2 = counts()
    sel = np.zeros(n, bool); sel[2:6] = True
    assert np.array_equal(c2["n_total"], c1["n_total"]) and np.array_equal(c2["episode"], c1["episode"])      # the ring and its position are not touched
    assert (c2["n_episode"][sel] == 0).all() and (c2["partial"][sel] == 1).all()
    assert np.array_equal(c2["n_episode"][~sel], c1["n_episode"][~sel]) and (c2["partial"][~sel] == 0).all()
    for t in range(24, 36):                                                           # the restored markets replay steps 24 ..: only that tail is counted
        env.step(*env.random_actions(t, action_seed=5))
    c3 = counts()
    assert np.array_equal(c3["n_episode"][sel], (c3["n_total"] - c1["n_total"])[sel]) and (c3["n_episode"][sel] > 0).any() and (c3["partial"][sel] == 1).all()
    last, cnt = env.tape_last(1024, 2, 4)
    assert np.array_equal(cnt.cpu().numpy(), c3["n_episode"][sel])
    rows, off, _ = env.drain_tape()
    rows, off = rows.cpu().numpy(), off.cpu().numpy()
    for j, m in enumerate(range(2, 6)):                                               # ... and they are the newest rows of the market's drained tape
        k = int(c3["n_episode"][m])
        assert np.array_equal(last[j, :k].cpu().numpy(), rows[off[m + 1] - k:off[m + 1]])
    mask = np.zeros(n, np.uint8); mask[3] = 1
    env.reset(mask=mask)                                                              # the next reset clears the bit - of the market that was reset
    c4 = counts()
    assert c4["partial"].tolist() == [0, 0, 1, 0, 1, 1, 0, 0] and c4["n_episode"][3] == 0 and c4["episode"][3] == c3["episode"][3] + 1
    assert np.array_equal(c4["n_total"], c3["n_total"])
    env.close()


@pytest.mark.parametrize("cap", [256, 512])
def test_run_random_hands_over_to_the_general_build_mid_episode_and_keeps_the_tape(cap):
    """Books prefilled to the point where the tile-only kernel is about to give a market up (resting orders + agents > tile).  The random agents cancel more
    of the prefilled orders than they add in most markets, but in some the book grows over the limit a few dozen steps in (measured: about one market in twelve,
    around step 20 - 40, with 40 - 80 fills on its tape by then): there k_tape_run's hot part closes the tape and the general build re-opens it inside the same
    launch (and the stepped env's k_tstep calls slow_tstep from then on).  One launch and per-step launches must give the same tape."""
    from decimal import Decimal
    from gym_continuousdoubleauction_amd import CDAVecEnv, _capi as K
    n, a, steps = 96, 8, 64
    per_side = (cap - a) // 2                                                         # 2 x per_side + a = cap: one more resting order and the market is cold
    cfg = {"num_of_agents": a, "init_cash": 10 ** 9, "max_step": 4000, "is_render": False, "initial_price_min": 5000, "initial_price_max": 6000, "book_capacity": cap}

    def prefilled():
        env = CDAVecEnv(cfg, n, with_info=False)
        env.enable_tape(4096)
        env.reset(seed=40)
        for i in range(n):
            s = env.get_state(i)
            lp = s.last_price
            s.n_bids = s.n_asks = per_side
            hold = [0] * a
            for k in range(per_side):                                                 # far from the touch on both sides, with the matching escrow
                b, q = s.bids[k], s.asks[k]
                b.price, b.qty, b.owner, b.order_id, b.timestamp = max(1, lp - 40 - k // 4), 1 + k % 3, k % a, 2 * k + 1, 2 * k + 1
                q.price, q.qty, q.owner, q.order_id, q.timestamp = lp + 40 + k // 4, 1 + k % 3, (k + 3) % a, 2 * k + 2, 2 * k + 2
                hold[k % a] += b.price * b.qty
                hold[(k + 3) % a] += q.price * q.qty
            s.lob_time = s.next_order_id = 2 * per_side
            for j in range(a):
                s.acc[j].cash_on_hold = K.decimal_to_dec(Decimal(hold[j]) * Decimal("1.0"))
                s.acc[j].cash = K.decimal_to_dec(Decimal(10 ** 9 - hold[j]) * Decimal("1.0"))
            env.set_state(i, s)
        assert (env.check_invariants().cpu().numpy() == 0).all()
        return env

    ref = prefilled()
    crossed_at = np.full(n, -1)
    fills_at_crossing = np.zeros(n, np.int64)
    for t in range(steps):
        ref.step(*ref.random_actions(t, action_seed=77))
        orders = np.array([ref.get_state(i).n_bids + ref.get_state(i).n_asks for i in range(n)]) if t < 56 else None
        if orders is not None:
            now = (crossed_at < 0) & (orders + a > cap)
            crossed_at[now] = t
            fills_at_crossing[now] = ref.tape_counts()["n_total"].cpu().numpy()[now]
    want, want_off, dropped = ref.drain_tape()
    total = np.diff(want_off.cpu().numpy())
    assert int(dropped.sum()) == 0
    # the hand-over happened in the MIDDLE of the episode - fills before it and fills after it - in several markets
    mid = (crossed_at > 0) & (fills_at_crossing > 0) & (fills_at_crossing < total)
    assert mid.sum() >= 3, (crossed_at, fills_at_crossing, total)
    run = prefilled()
    run.run_random(steps, action_seed=77)
    got, got_off, dropped = run.drain_tape()
    assert int(dropped.sum()) == 0 and torch.equal(got_off, want_off) and torch.equal(got, want)
    for k in ("n_total", "n_episode", "episode", "partial"):
        assert torch.equal(run.tape_counts()[k], ref.tape_counts()[k]), k
    for i in (0, n // 2, n - 1):
        assert bytes(run.get_state(i)) == bytes(ref.get_state(i))
    ref.close(); run.close()


def test_rollout_chains_record_through_the_step_kernel_and_refuse_a_toggled_tape():
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd._lib import lib
    N, A, T = 64, 4, 32
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    assert lib().cda_policy_step_supported(env._h) == 1
    env.enable_tape(1024)
    assert lib().cda_policy_step_supported(env._h) == 0
    env.reset(seed=700)
    roll = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=21), T, groups=2, seed=3)
    buf = roll.run()
    torch.cuda.synchronize()
    b = {k: v.cpu().numpy() for k, v in buf.items() if k in ("category", "size_mean", "size_sigma", "price", "price_offset")}
    got, off = env.drain_tape()[:2]
    other = CDAVecEnv(cfg, n_markets=N, with_info=False)
    other.enable_tape(1024)
    other.reset(seed=700)
    for t in range(T):
        other.step(b["category"][t], b["size_mean"][t], b["size_sigma"][t], b["price"][t], b["price_offset"][t])
    want, want_off = other.drain_tape()[:2]
    assert len(want) > 0 and torch.equal(off, want_off) and torch.equal(got, want)
    env.disable_tape()
    with pytest.raises(RuntimeError, match="trade tape"):
        roll.run()
    env.close(); other.close()


def test_the_facade_tape_is_the_reference_tape():
    from decimal import Decimal
    from gym_continuousdoubleauction_amd import CDAEnv
    from gym_continuousdoubleauction_amd.tape import to_reference_records
    name = "tick5_s301"
    r, fx = G.load(name), _fixture(name)
    env = CDAEnv(r["config"])
    with pytest.raises(RuntimeError, match="enable_tape"):
        env.tape
    env.enable_tape(1024)
    env.reset(seed=int(r["seed"]))
    A = r["cat"].shape[1]
    for t in range(r["cat"].shape[0]):
        order = sorted((a for a in range(A) if r["present"][t, a]), key=lambda a: (int(r["present"][t, a]), a))
        env.step({f"agent_{a}": {"category": np.int64(r["cat"][t, a]), "size_mean": np.array([r["mean"][t, a]], np.float32), "size_sigma": np.array([r["sigma"][t, a]], np.float32),
                                 "price": np.int64(r["price"][t, a]), "price_offset": np.int64(r["off"][t, a])} for a in order})
    tape = env.tape
    assert tape == to_reference_records(fx["rows"])
    for i, s in zip(fx["repr_idx"], fx["repr"]):                                        # ... and the reference's own records, as it printed them
        assert tape[int(i)] == eval(str(s), {"Decimal": Decimal, "np": np, "__builtins__": {}}), (i, s)
    env.close()


def test_evaluate_saves_the_tape_with_market_episode_and_module_ids(tmp_path):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    from gym_continuousdoubleauction_amd.tape import load_tape
    N, A, E = 64, 4, 3
    env = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 32, "is_render": False, "auto_reset": True}, n_markets=N, with_info=False)
    pol = mlp.FusedPolicy("cuda:0", seed=5)
    path = str(tmp_path / "tape.npz")
    keep = {}
    res = evaluate(env, pol, opponents=["random"], trained_slots=2, episodes=E, seed=3, tape=path, keep=keep)
    plain = evaluate(env, pol, opponents=["random"], trained_slots=2, episodes=E, seed=3)
    assert res["summary"] == plain["summary"] and not env.tape_enabled                 # the tape changed nothing, and the env's setting is back
    z = load_tape(path)
    rows, market, episode = z["records"], z["market"], z["episode"]
    assert len(rows) > N and int(z["dropped"].sum()) == 0
    assert set(np.unique(episode)) <= set(range(E)) and market.min() >= 0 and market.max() < N
    assert list(z["module_names"]) == list(res["modules"]) and np.array_equal(z["modules"], keep["modules"])
    assert np.array_equal(z["init_module"], keep["modules"][market, rows[:, 6]]) and np.array_equal(z["counter_module"], keep["modules"][market, rows[:, 3]])
    # per (market, episode) the records are in step order and the step index stays inside the episode
    t = rows[:, 7] >> 2
    assert t.min() >= 0 and t.max() < 32
    for m in (0, N // 2, N - 1):
        for e in range(E):
            sel = (market == m) & (episode == e)
            assert (np.diff(t[sel]) >= 0).all(), (m, e)
    # the same actions replayed by plain steps on a tape-enabled env: the same records, episode by episode
    other = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 32, "is_render": False, "auto_reset": True}, n_markets=N, with_info=False)
    other.enable_tape(4096)
    other.reset(seed=(np.uint64(3) * np.uint64(N) + np.arange(N, dtype=np.uint64)))
    acts = {k: v.numpy() for k, v in keep["actions"].items()}
    got_rows, got_ep, got_m = [], [], []
    for step in range(E * 32):
        other.step(acts["category"][step], acts["size_mean"][step], acts["size_sigma"][step], acts["price"][step], acts["price_offset"][step])
        r, off, _ = other.drain_tape()
        got_rows.append(r.cpu().numpy()); got_ep.append(np.full(len(r), step // 32, np.int32)); got_m.append(np.repeat(np.arange(N, dtype=np.int32), np.diff(off.cpu().numpy())))
    got_rows, got_ep, got_m = np.concatenate(got_rows), np.concatenate(got_ep), np.concatenate(got_m)
    key_a = np.lexsort((np.arange(len(rows)), episode, market))
    key_b = np.lexsort((np.arange(len(got_rows)), got_ep, got_m))
    assert np.array_equal(rows[key_a], got_rows[key_b]) and np.array_equal(episode[key_a], got_ep[key_b]) and np.array_equal(market[key_a], got_m[key_b])
    env.close(); other.close()


def test_evaluate_labels_episodes_of_markets_that_are_out_of_step(tmp_path):
    """Rollout chunks no longer than an episode (max_step 256 -> chunks of 128 steps), and markets whose own horizon is shorter (per-market max_step 100: one reset
    inside every chunk, at a different in-episode step each time; 48: several per chunk): the episode id of every saved record equals the one a per-step drained
    replay of the same actions gives - there the episode of a record is the market's episode counter when the step ran."""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    from gym_continuousdoubleauction_amd.tape import load_tape
    N, A, S = 48, 4, 256
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": S, "is_render": False, "auto_reset": True}
    rows_cfg = [{"max_step": (S, 100, 48)[i % 3]} for i in range(N)]
    env = CDAVecEnv(cfg, n_markets=N, with_info=False, market_configs=rows_cfg)
    pol = mlp.FusedPolicy("cuda:0", seed=5)
    path = str(tmp_path / "tape.npz")
    keep = {}
    res = evaluate(env, pol, opponents=["random"], trained_slots=2, episodes=1, seed=9, tape=path, keep=keep)
    assert res["config"]["horizon"] <= S // 2 and not env.tape_enabled
    z = load_tape(path)
    rows, market, episode = z["records"], z["market"], z["episode"]
    assert episode.min() == 0 and episode[market % 3 == 0].max() == 0 and episode[market % 3 == 1].max() == 2 and episode[market % 3 == 2].max() == 5
    other = CDAVecEnv(cfg, n_markets=N, with_info=False, market_configs=rows_cfg)
    other.enable_tape(4096)
    other.reset(seed=(np.uint64(9) * np.uint64(N) + np.arange(N, dtype=np.uint64)))
    acts = {k: v.numpy() for k, v in keep["actions"].items()}
    got_rows, got_ep, got_m = [], [], []
    for step in range(S):
        ep_now = other.tape_counts()["episode"].cpu().numpy() - 1
        other.step(acts["category"][step], acts["size_mean"][step], acts["size_sigma"][step], acts["price"][step], acts["price_offset"][step])
        r, off, _ = other.drain_tape()
        m = np.repeat(np.arange(N, dtype=np.int32), np.diff(off.cpu().numpy()))
        got_rows.append(r.cpu().numpy()); got_m.append(m); got_ep.append(ep_now[m].astype(np.int32))
    got_rows, got_ep, got_m = np.concatenate(got_rows), np.concatenate(got_ep), np.concatenate(got_m)
    key_a = np.lexsort((np.arange(len(rows)), market))
    key_b = np.lexsort((np.arange(len(got_rows)), got_m))
    assert np.array_equal(rows[key_a], got_rows[key_b]) and np.array_equal(market[key_a], got_m[key_b])
    bad = np.flatnonzero(episode[key_a] != got_ep[key_b])
    assert bad.size == 0, (bad[:8], market[key_a][bad[:8]], episode[key_a][bad[:8]], got_ep[key_b][bad[:8]])
    # a tape that is already running is the caller's: evaluate does not wipe it
    env.enable_tape(64)
    with pytest.raises(ValueError, match="trade tape is off"):
        evaluate(env, pol, opponents=["random"], trained_slots=2, episodes=1, seed=9, tape=path)
    assert env.tape_capacity == 64
    env.close(); other.close()
