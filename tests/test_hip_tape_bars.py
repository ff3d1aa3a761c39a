"""GPU: the tape's device reductions (CDAVecEnv.tape_bars / tape_flows, include/cda.h cda_tape_bars / cda_tape_flows) and the remembered previous episode
(tape_counts()["n_previous"], tape_last(episode="previous")).  Expected values never come from the code under test: the few-line numpy statements below are
applied to the REFERENCE's tape rows (tests/golden/tape_*.npz) or to records read back with drain_tape, which tests/test_hip_tape.py pins to those fixtures.
Integers only: every comparison is exact."""
import numpy as np
import pytest
import torch

import golden_util as G
from test_hip_tape import FIXTURES, _actions, _fixture, _replay

pytestmark = pytest.mark.gpu

BAR_FIELDS = ("open", "high", "low", "close", "n_trades", "n_self", "volume", "buy_volume", "notional")


def np_bars(rows, bar_steps, n_bars):
    """-> (int64 [n_bars, 9] in the order of BAR_FIELDS, rows left out because their bar index is >= n_bars)"""
    rows = np.asarray(rows, np.int64).reshape(-1, 8)
    bar = (rows[:, 7] >> 2) // bar_steps
    out = np.zeros((n_bars, 9), np.int64)
    for b in range(n_bars):
        x = rows[bar == b]
        if len(x):
            p, q = x[:, 1], x[:, 2]
            out[b] = [p[0], p.max(), p.min(), p[-1], len(x), (x[:, 3] == x[:, 6]).sum(), q.sum(), q[(x[:, 7] & 2) == 0].sum(), (p * q).sum()]
    return out, int((bar >= n_bars).sum())


def np_flows(rows, agents):
    out = np.zeros((agents, agents, 3), np.int64)
    for _, price, qty, counter, _, _, init, _ in np.asarray(rows, np.int64).reshape(-1, 8).tolist():
        out[init, counter] += (qty, price * qty, 1)
    return out


def dev_bars(bars):
    """the device's int32 [n, n_bars, 12] as int64 [n, n_bars, 9] (the three 64-bit sums from their word pairs)"""
    w = bars.cpu().numpy()
    assert w.dtype == np.int32 and w.shape[-1] == 12
    wide = np.ascontiguousarray(w[..., 6:]).view(np.int64)
    return np.concatenate([w[..., :6].astype(np.int64), wide], axis=-1)


def check_market(env, m, which, rows, agents, bar_steps, n_bars, lost=0, partial=0):
    bars, info = env.tape_bars(bar_steps, n_bars, episode=which, first_market=m, n_markets=1)
    want, beyond = np_bars(rows, bar_steps, n_bars)
    got = dev_bars(bars)[0]
    bad = np.argwhere(got != want)
    assert bad.size == 0, (which, m, bar_steps, n_bars, bad[:6], got[bad[:3, 0]], want[bad[:3, 0]])
    assert info.cpu().tolist() == [[len(rows) - beyond, lost, beyond, partial]], (which, m, bar_steps, info.cpu().tolist())
    flows, info = env.tape_flows(episode=which, first_market=m, n_markets=1)
    assert flows.dtype == torch.int64 and tuple(flows.shape) == (1, agents, agents, 3)
    assert np.array_equal(flows[0].cpu().numpy(), np_flows(rows, agents)), (which, m)
    assert info.cpu().tolist() == [[len(rows), lost, 0, partial]]


@pytest.mark.parametrize("name", FIXTURES)
def test_bars_and_flows_of_every_fixture_equal_numpy_over_the_reference_tape(name):
    from gym_continuousdoubleauction_amd.tape import as_bars, bars_from_records
    env, rec, fx = _replay(name, state_every=64 if name.startswith("bigbook") else 16)
    agents, max_step = int(rec["config"]["num_of_agents"]), int(rec["config"]["max_step"])
    rows = fx["rows"][fx["episode"] == fx["episode"].max()]
    assert len(rows) > 0
    for bar_steps in (1, 7, 64, max_step):
        check_market(env.env, 0, "current", rows, agents, bar_steps, -(-max_step // bar_steps))
    # the default bar count, the structured view and the host statement of tape.py agree with it
    bars, info = env.env.tape_bars(7)
    assert tuple(bars.shape) == (1, -(-max_step // 7), 12)
    host, _ = bars_from_records(rows, 7, bars.shape[1])
    assert np.array_equal(as_bars(bars)[0], host)
    # fewer bars than the episode has steps: the rest is counted in info, not folded into the last bar
    check_market(env.env, 0, "current", rows, agents, 3, 5)
    env.close()


def test_the_previous_episode_is_remembered_across_a_reset():
    env, rec, fx = _replay("reset_s51")
    ep = [fx["rows"][fx["episode"] == k] for k in range(3)]
    assert [len(e) for e in ep] == [31, 41, 25]
    counts = {k: v.cpu().tolist() for k, v in env.env.tape_counts().items()}
    assert counts["n_previous"] == [41] and counts["n_episode"] == [25] and counts["n_total"] == [97]
    for bar_steps in (1, 7, 40):
        check_market(env.env, 0, "previous", ep[1], 4, bar_steps, -(-40 // bar_steps))
        check_market(env.env, 0, "current", ep[2], 4, bar_steps, -(-40 // bar_steps))
    last, cnt = env.env.tape_last(64, episode="previous")
    assert cnt.cpu().tolist() == [41] and np.array_equal(last[0, :41].cpu().numpy(), ep[1]) and int(last[0, 41:].abs().sum()) == 0
    last, cnt = env.env.tape_last(5, episode="previous")
    assert cnt.cpu().tolist() == [5] and np.array_equal(last[0].cpu().numpy(), ep[1][-5:])
    last, cnt = env.env.tape_last(64)                                                  # the default is what it was: the current episode
    assert cnt.cpu().tolist() == [25] and np.array_equal(last[0, :25].cpu().numpy(), ep[2])
    with pytest.raises(ValueError):
        env.env.tape_last(4, episode="next")
    env.close()


def _labelled_rows(env, totals, episodes):
    """every market's whole tape (a cursor of its own at 0: the env's is not moved) and, per record, the episode it belongs to: the records a step wrote belong to
    the episode the market was in BEFORE that step (a step that ends an episode still writes into it).  totals / episodes: tape_counts() after every step,
    [steps + 1, N] with the values before the first step in row 0."""
    rows, off, dropped = env.drain_tape(cursor=torch.zeros(env.n_markets, dtype=torch.int64, device=env.device))
    assert int(dropped.sum()) == 0
    rows, off = rows.cpu().numpy(), off.cpu().numpy()
    totals, episodes = np.asarray(totals), np.asarray(episodes)
    out = []
    for m in range(env.n_markets):
        r = rows[off[m]:off[m + 1]]
        label = np.repeat(episodes[:-1, m], np.diff(totals[:, m]))
        assert len(label) == len(r) == totals[-1, m]
        out.append((r, label))
    return out


@pytest.mark.parametrize("n,a,groups", [(1024, 4, None), (256, 8, None), (64, 16, None), (256, 4, 4)])
def test_both_remembered_episodes_of_an_auto_resetting_batch(n, a, groups):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    max_step, steps, bar_steps = 48, 256, 8
    cfg = {"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n, with_info=False, **({"groups": groups} if groups else {}))      # without info tensors the step kernel resets the market itself
    env.enable_tape(4096)
    env.reset(seed=np.arange(700, 700 + n, dtype=np.uint64))
    c = env.tape_counts()
    totals, episodes = [c["n_total"].cpu().numpy().copy()], [c["episode"].cpu().numpy().copy()]
    rng = np.random.default_rng(78)
    checked = 0
    for t in range(steps):
        env.step(*_actions(rng, n, a))
        c = {k: v.cpu().numpy().copy() for k, v in env.tape_counts().items()}
        totals.append(c["n_total"]); episodes.append(c["episode"])
        # behind the step that ended an episode (the current one is empty), in the middle of an episode, and at the end
        if t + 1 in (2 * max_step, 2 * max_step + 4, steps):
            assert (c["episode"] == 1 + (t + 1) // max_step).all()
            per_market = _labelled_rows(env, totals, episodes)
            n_bars = max_step // bar_steps
            bars = {w: dev_bars(env.tape_bars(bar_steps, episode=w)[0]) for w in ("current", "previous")}
            binfo = {w: env.tape_bars(bar_steps, episode=w)[1].cpu().numpy() for w in ("current", "previous")}
            flows = {w: env.tape_flows(episode=w)[0].cpu().numpy() for w in ("current", "previous")}
            finfo = {w: env.tape_flows(episode=w)[1].cpu().numpy() for w in ("current", "previous")}
            assert bars["current"].shape == (n, n_bars, 9) and flows["current"].shape == (n, a, a, 3)
            for m, (r, label) in enumerate(per_market):
                for w, ep in (("current", c["episode"][m]), ("previous", c["episode"][m] - 1)):
                    x = r[label == ep]
                    want, beyond = np_bars(x, bar_steps, n_bars)
                    assert beyond == 0
                    assert np.array_equal(bars[w][m], want), (t, m, w, np.argwhere(bars[w][m] != want)[:4])
                    assert np.array_equal(flows[w][m], np_flows(x, a)), (t, m, w)
                    assert binfo[w][m].tolist() == [len(x), 0, 0, 0] and finfo[w][m].tolist() == [len(x), 0, 0, 0], (t, m, w)
                assert c["n_previous"][m] == (label == c["episode"][m] - 1).sum() and c["n_episode"][m] == (label == c["episode"][m]).sum()
            if t + 1 == 2 * max_step:
                assert (c["n_episode"] == 0).all() and not bars["current"].any() and not flows["current"].any()
            assert (c["n_previous"] > 0).sum() > n // 8
            checked += 1
    assert checked == 3
    # a sub-range reads the same rows
    sub, _ = env.tape_bars(bar_steps, episode="previous", first_market=n // 2 + 1, n_markets=5)
    assert np.array_equal(dev_bars(sub), bars["previous"][n // 2 + 1:n // 2 + 6])
    sub, _ = env.tape_flows(episode="current", first_market=n - 3, n_markets=3)
    assert np.array_equal(sub.cpu().numpy(), flows["current"][n - 3:])
    env.close()


def test_the_reset_pass_behind_a_step_with_info_tensors_remembers_the_episode_too():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a, max_step = 96, 4, 24
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}, n, with_info=True)
    env.enable_tape(1024)
    env.reset(seed=np.arange(40, 40 + n, dtype=np.uint64))
    c = env.tape_counts()
    totals, episodes = [c["n_total"].cpu().numpy().copy()], [c["episode"].cpu().numpy().copy()]
    rng = np.random.default_rng(3)
    for t in range(2 * max_step + 5):
        env.step(*_actions(rng, n, a))
        c = {k: v.cpu().numpy().copy() for k, v in env.tape_counts().items()}
        totals.append(c["n_total"]); episodes.append(c["episode"])
    per_market = _labelled_rows(env, totals, episodes)
    bars = {w: dev_bars(env.tape_bars(5, episode=w)[0]) for w in ("current", "previous")}
    flows = {w: env.tape_flows(episode=w)[0].cpu().numpy() for w in ("current", "previous")}
    assert (c["episode"] == 3).all() and (c["n_previous"] > 0).any()
    for m, (r, label) in enumerate(per_market):
        assert c["n_previous"][m] == (label == 2).sum()
        for w, ep in (("current", 3), ("previous", 2)):
            assert np.array_equal(bars[w][m], np_bars(r[label == ep], 5, 5)[0]), (m, w)
            assert np.array_equal(flows[w][m], np_flows(r[label == ep], a)), (m, w)
    env.close()


def test_a_ring_smaller_than_the_episode_reports_what_it_lost():
    env, rec, fx = _replay("aggr_s23", capacity=64)
    rows = fx["rows"]
    assert len(rows) == 353
    for bar_steps in (1, 16, 256):
        check_market(env.env, 0, "current", rows[-64:], 4, bar_steps, -(-256 // bar_steps), lost=289)
    env.close()


def test_after_a_restore_only_the_tail_is_read_and_nothing_is_remembered():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a = 8, 4
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 256, "is_render": False}, n)
    env.enable_tape(1024)
    env.reset(seed=31)
    for t in range(24):
        env.step(*env.random_actions(t, action_seed=4))
    env.reset(seed=32)                                                                # a finished episode to remember
    for t in range(24):
        env.step(*env.random_actions(t, action_seed=5))
    snap = env.snapshot(2, 4)                                                         # markets 2 .. 5
    for t in range(24, 40):
        env.step(*env.random_actions(t, action_seed=5))
    c1 = {k: v.cpu().numpy().copy() for k, v in env.tape_counts().items()}
    assert (c1["n_previous"] > 0).any() and (c1["n_previous"] + c1["n_episode"] == c1["n_total"]).all()
    env.restore(snap, first=2)
    sel = np.zeros(n, bool); sel[2:6] = True
    c2 = {k: v.cpu().numpy().copy() for k, v in env.tape_counts().items()}
    assert (c2["n_previous"][sel] == 0).all() and np.array_equal(c2["n_previous"][~sel], c1["n_previous"][~sel])
    for t in range(24, 36):
        env.step(*env.random_actions(t, action_seed=5))
    c3 = {k: v.cpu().numpy().copy() for k, v in env.tape_counts().items()}
    rows, off, _ = env.drain_tape()
    rows, off = rows.cpu().numpy(), off.cpu().numpy()
    assert (c3["n_episode"][sel] > 0).any()
    for m in range(n):
        r = rows[off[m]:off[m + 1]]
        k = int(c3["n_episode"][m])
        tail = r[len(r) - k:]
        check_market(env, m, "current", tail, a, 8, 32, partial=int(sel[m]))          # a restored market: only what followed the restore, flagged partial
        if sel[m]:
            assert (tail[:, 7] >> 2 >= 24).all()
            check_market(env, m, "previous", r[:0], a, 8, 32)                         # nothing is remembered
        else:
            p = int(c1["n_previous"][m])
            check_market(env, m, "previous", r[:p], a, 8, 32)
    env.close()


def test_reading_is_not_steering():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a, steps = 128, 4, 96
    cfg = {"num_of_agents": a, "init_cash": 1000000, "max_step": 40, "is_render": False, "auto_reset": True}
    plain, read = CDAVecEnv(cfg, n, with_info=False), CDAVecEnv(cfg, n, with_info=False)
    sample = list(range(0, n, 9)) + [n - 1]
    for e in (plain, read):
        e.enable_tape(1024)
        e.reset(seed=77)
    for t in range(steps):
        acts = plain.random_actions(t, action_seed=6)
        plain.step(*acts)
        read.step(*acts)
        if t % 13 == 5:
            before = [bytes(read.get_state(i)) for i in sample]
            cb = {k: v.clone() for k, v in read.tape_counts().items()}
            for w in ("current", "previous"):
                read.tape_bars(4, episode=w); read.tape_bars(1, 3, episode=w); read.tape_flows(episode=w); read.tape_last(9, episode=w)
            assert before == [bytes(read.get_state(i)) for i in sample]
            assert all(torch.equal(v, cb[k]) for k, v in read.tape_counts().items())
    for i in sample:
        assert bytes(plain.get_state(i)) == bytes(read.get_state(i)), i
    for k, v in plain.tape_counts().items():
        assert torch.equal(v, read.tape_counts()[k]), k
    assert torch.equal(plain.drain_tape()[0], read.drain_tape()[0])
    plain.close(); read.close()


def test_tape_off_and_bad_arguments_are_refused():
    from gym_continuousdoubleauction_amd import CDAVecEnv, CDAEnv, _capi as K
    from gym_continuousdoubleauction_amd._lib import lib
    n, a = 16, 4
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 32, "is_render": False}, n)
    env.reset(seed=1)
    bars = torch.full((n, 4, 12), -5, dtype=torch.int32, device=env.device)
    flows = torch.full((n, a, a, 3), -5, dtype=torch.int64, device=env.device)
    with pytest.raises(RuntimeError, match="enable_tape"):
        env.tape_bars(4)
    with pytest.raises(RuntimeError, match="enable_tape"):
        env.tape_flows()
    assert lib().cda_tape_bars(env._h, 0, n, 0, 4, 4, bars.data_ptr(), None, None) == K.ERR_UNSUPPORTED
    assert lib().cda_tape_flows(env._h, 0, n, 0, flows.data_ptr(), None, None) == K.ERR_UNSUPPORTED
    env.enable_tape(256)
    for t in range(8):
        env.step(*env.random_actions(t, action_seed=2))
    for kw in ({"bar_steps": 0}, {"bar_steps": -3}, {"bar_steps": 4, "n_bars": 0}, {"bar_steps": 4, "first_market": n}, {"bar_steps": 4, "first_market": -1},
               {"bar_steps": 4, "first_market": 8, "n_markets": 9}, {"bar_steps": 4, "n_markets": 0}, {"bar_steps": 4, "episode": "last"}):
        with pytest.raises(ValueError):
            env.tape_bars(**kw)
    for kw in ({"first_market": n}, {"first_market": 8, "n_markets": 9}, {"n_markets": 0}, {"episode": 1}):
        with pytest.raises(ValueError):
            env.tape_flows(**kw)
    # the library refuses them itself, without a launch: the buffers keep their fill
    for first, cnt, which, bar_steps, n_bars in ((0, n, 0, 0, 4), (0, n, 0, 4, 0), (0, n + 1, 0, 4, 4), (-1, 4, 0, 4, 4), (4, 0, 0, 4, 4), (0, n, 2, 4, 4), (0, n, -1, 4, 4)):
        assert lib().cda_tape_bars(env._h, first, cnt, which, bar_steps, n_bars, bars.data_ptr(), None, None) == K.ERR_INVALID
    assert lib().cda_tape_bars(env._h, 0, n, 0, 4, 4, bars.data_ptr() + 4, None, None) == K.ERR_INVALID      # (not 16-byte aligned)
    for first, cnt, which in ((0, n + 1, 0), (-1, 4, 0), (0, n, 2)):
        assert lib().cda_tape_flows(env._h, first, cnt, which, flows.data_ptr(), None, None) == K.ERR_INVALID
    torch.cuda.synchronize()
    assert int((bars != -5).sum()) == 0 and int((flows != -5).sum()) == 0
    got, _ = env.tape_bars(4, 4)                                                      # ... and the same shapes, asked properly, are filled
    assert int((got[:, :, 4] > 0).sum()) > 0
    env.close()
    # the one-market facade
    rec, fx = G.load("tick5_s301"), _fixture("tick5_s301")
    one = CDAEnv(rec["config"])
    with pytest.raises(RuntimeError, match="enable_tape"):
        one.tape_bars(4)
    one.enable_tape(64)
    one.reset(seed=int(rec["seed"]))
    b = one.tape_bars(4)
    assert b.shape == (-(-int(rec["config"]["max_step"]) // 4),) and b.dtype.names == BAR_FIELDS and int(b["n_trades"].sum()) == 0
    one.close()


def test_flows_by_module_on_a_league_mapping():
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd.league import LeagueSlotMapper
    from gym_continuousdoubleauction_amd.tape import flows_by_module
    n, a, k = 192, 8, 2
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 64, "is_render": False}, n, with_info=False)
    env.enable_tape(1024)
    env.reset(seed=5)
    for t in range(48):
        env.step(*env.random_actions(t, action_seed=8))
    bank = mlp.PolicyBank("cuda:0", n, a, k, max_frozen=4, seed=5, random_seed=9)
    mapper = LeagueSlotMapper(a, k, a - k, 1.0, 3.0)
    net_of = {mapper.add_champion(): bank.snapshot(0) for _ in range(3)}
    slot_pool = torch.full((n, a), -1, dtype=torch.int32, device="cuda:0")
    mapper.assign_device(bank, episode_ids=[f"e0-m{i}" for i in range(n)], net_of=net_of, slot_pool=slot_pool)
    module_of = torch.where(slot_pool < 0, torch.arange(a, device="cuda:0", dtype=torch.int32).expand(n, a), slot_pool + k)
    n_mod = len(mapper.available_modules)
    flows, _ = env.tape_flows()
    got = flows_by_module(flows, module_of, n_mod)
    assert got.device == flows.device and got.dtype == torch.int64 and tuple(got.shape) == (n_mod, n_mod, 3)
    f, mod = flows.cpu().numpy(), module_of.cpu().numpy()
    want = np.zeros((n_mod, n_mod, 3), np.int64)
    for i in range(n):
        for x in range(a):
            for y in range(a):
                want[mod[i, x], mod[i, y]] += f[i, x, y]
    assert np.array_equal(got.cpu().numpy(), want) and int(want[:, :, 2].sum()) == int(env.tape_counts()["n_total"].sum()) > n
    assert len(np.unique(mod)) > a                                                    # (champions were drawn: more modules than slots)
    with pytest.raises(ValueError):
        flows_by_module(flows, module_of, int(mod.max()))
    env.close()
