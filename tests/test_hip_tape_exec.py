"""GPU: the tape's execution report (CDAVecEnv.tape_exec / CDAEnv.tape_exec, include/cda.h cda_tape_exec; evaluate(exec_horizons=...)).  The expected tables are
tape.exec_from_records - which tests/test_tape_exec_host.py pins to a naive loop and to hand-written answers - of the REFERENCE's tape rows
(tests/golden/tape_*.npz) or of records read back with drain_tape, which tests/test_hip_tape.py pins to those fixtures.  Integers only: every comparison is exact."""
import numpy as np
import pytest
import torch

import golden_util as G
from test_hip_tape import FIXTURES, _actions, _fixture, _replay
from test_hip_tape_bars import _labelled_rows
from test_tape_exec_host import HORIZONS

pytestmark = pytest.mark.gpu


def check_market(env, m, which, rows, agents, horizons=HORIZONS, lost=0, partial=0):
    from gym_continuousdoubleauction_amd.tape import exec_from_records
    stats, marks, info = env.tape_exec(horizons, episode=which, first_market=m, n_markets=1)
    assert stats.dtype == torch.int64 and marks.dtype == torch.int64 and info.dtype == torch.int32
    assert tuple(stats.shape) == (1, agents, 16) and tuple(marks.shape) == (1, agents, len(horizons), 2, 4)
    want_s, want_m = exec_from_records(rows, agents, horizons)
    got_s, got_m = stats[0].cpu().numpy(), marks[0].cpu().numpy()
    assert np.array_equal(got_s, want_s), (which, m, np.argwhere(got_s != want_s)[:6], got_s[got_s != want_s][:6], want_s[got_s != want_s][:6])
    assert np.array_equal(got_m, want_m), (which, m, np.argwhere(got_m != want_m)[:6], got_m[got_m != want_m][:6], want_m[got_m != want_m][:6])
    assert info.cpu().tolist() == [[len(rows), lost, 0, partial]], (which, m, info.cpu().tolist())
    return got_s, got_m


@pytest.mark.parametrize("name", FIXTURES)
def test_the_report_of_every_fixture_equals_the_restatement_over_the_reference_tape(name):
    env, rec, fx = _replay(name, state_every=64 if name.startswith("bigbook") else 16)
    agents = int(rec["config"]["num_of_agents"])
    last = int(fx["episode"].max())
    rows = fx["rows"][fx["episode"] == last]
    assert len(rows) > 0
    check_market(env.env, 0, "current", rows, agents)
    check_market(env.env, 0, "current", rows, agents, horizons=(3,))
    check_market(env.env, 0, "current", rows, agents, horizons=(7, 0, 2, 64, 1, 1000000, 11, 5))      # eight, unsorted, one beyond any episode
    if last > 0:
        check_market(env.env, 0, "previous", fx["rows"][fx["episode"] == last - 1], agents)
    else:
        check_market(env.env, 0, "previous", rows[:0], agents)
    env.close()


@pytest.mark.parametrize("n,a,steps", [(1024, 4, 200), (512, 8, 200), (64, 16, 200)])
def test_random_play_with_auto_reset_both_remembered_episodes(n, a, steps):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd.tape import STAT, exec_from_records
    max_step, hz = 64, (1, 5, 20)
    cfg = {"num_of_agents": a, "init_cash": 1000000, "max_step": max_step, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n, with_info=False)
    env.enable_tape(4096)
    env.reset(seed=np.arange(900, 900 + n, dtype=np.uint64))
    c = env.tape_counts()
    totals, episodes = [c["n_total"].cpu().numpy().copy()], [c["episode"].cpu().numpy().copy()]
    rng = np.random.default_rng(79)
    checked = 0
    for t in range(steps):
        env.step(*_actions(rng, n, a))
        c = {k: v.cpu().numpy().copy() for k, v in env.tape_counts().items()}
        totals.append(c["n_total"]); episodes.append(c["episode"])
        # right behind the step that ended an episode (the current one is empty), and in the middle of an episode
        if t + 1 in (2 * max_step, steps):
            per_market = _labelled_rows(env, totals, episodes)
            got = {w: [x.cpu().numpy() for x in env.tape_exec(hz, episode=w)] for w in ("current", "previous")}
            flows = {w: env.tape_flows(episode=w)[0].cpu().numpy() for w in ("current", "previous")}
            for m, (r, label) in enumerate(per_market):
                for w, ep in (("current", c["episode"][m]), ("previous", c["episode"][m] - 1)):
                    x = r[label == ep]
                    want_s, want_m = exec_from_records(x, a, hz)
                    stats, marks, info = (g[m] for g in got[w])
                    assert np.array_equal(stats, want_s), (t, m, w, np.argwhere(stats != want_s)[:6])
                    assert np.array_equal(marks, want_m), (t, m, w, np.argwhere(marks != want_m)[:6])
                    assert info.tolist() == [len(x), 0, 0, 0], (t, m, w)
            for w in ("current", "previous"):
                stats, marks, info = got[w]
                # maker + taker quantity is twice what changed hands between different agents; a complete episode's net purchases are its final position
                off = flows[w][..., 0].sum(axis=(1, 2)) - np.trace(flows[w][..., 0], axis1=1, axis2=2)
                assert np.array_equal((stats[:, :, STAT["maker_qty"]] + stats[:, :, STAT["taker_qty"]]).sum(axis=1), 2 * off)
                assert (info[:, 1] == 0).all() and (info[:, 3] == 0).all()
                assert np.array_equal(stats[:, :, STAT["buy_qty"]] - stats[:, :, STAT["sell_qty"]], stats[:, :, STAT["final_pos"]])
            if t + 1 == 2 * max_step:
                assert (c["n_episode"] == 0).all() and not got["current"][0][:, :, :14].any() and not got["current"][1].any()
            assert int(got["previous"][1][:, :, 0, :, 2].sum()) > n                   # mark-outs were scored, not only counted as open
            checked += 1
    assert checked == 2
    # a sub-range of markets reads the same rows
    sub = env.tape_exec(hz, episode="previous", first_market=n // 2 + 1, n_markets=5)
    assert all(np.array_equal(x.cpu().numpy(), g[n // 2 + 1:n // 2 + 6]) for x, g in zip(sub, got["previous"]))
    sub = env.tape_exec(hz, first_market=n - 3, n_markets=3)
    assert all(np.array_equal(x.cpu().numpy(), g[n - 3:]) for x, g in zip(sub, got["current"]))
    env.close()


def test_per_market_max_step():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a, steps = 96, 4, 150
    cfg = {"num_of_agents": a, "init_cash": 1000000, "max_step": 128, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=n, with_info=False, market_configs=[{"max_step": (128, 50, 24)[i % 3]} for i in range(n)])
    env.enable_tape(2048)
    env.reset(seed=np.arange(70, 70 + n, dtype=np.uint64))
    c = env.tape_counts()
    totals, episodes = [c["n_total"].cpu().numpy().copy()], [c["episode"].cpu().numpy().copy()]
    rng = np.random.default_rng(80)
    for t in range(steps):
        env.step(*_actions(rng, n, a))
        c = {k: v.cpu().numpy().copy() for k, v in env.tape_counts().items()}
        totals.append(c["n_total"]); episodes.append(c["episode"])
    assert np.array_equal(c["episode"], 1 + steps // np.array([(128, 50, 24)[i % 3] for i in range(n)]))
    for m, (r, label) in enumerate(_labelled_rows(env, totals, episodes)):
        for w, ep in (("current", c["episode"][m]), ("previous", c["episode"][m] - 1)):
            check_market(env, m, w, r[label == ep], a, horizons=(1, 5, 20))
    env.close()


def test_a_ring_smaller_than_the_episode_reports_what_it_lost():
    env, rec, fx = _replay("aggr_s23", capacity=64)
    rows = fx["rows"]
    assert len(rows) == 353
    got_s, _ = check_market(env.env, 0, "current", rows[-64:], 4, lost=289)               # positions relative to the first held record
    from gym_continuousdoubleauction_amd.tape import STAT, exec_from_records
    assert not np.array_equal(got_s[:, STAT["final_pos"]], exec_from_records(rows, 4, HORIZONS)[0][:, STAT["final_pos"]])
    env.close()


def test_after_a_restore_only_the_tail_is_read():
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
    env.restore(snap, first=2)
    sel = np.zeros(n, bool); sel[2:6] = True
    for t in range(24, 36):
        env.step(*env.random_actions(t, action_seed=5))
    c3 = {k: v.cpu().numpy().copy() for k, v in env.tape_counts().items()}
    rows, off, _ = env.drain_tape()
    rows, off = rows.cpu().numpy(), off.cpu().numpy()
    assert (c3["n_episode"][sel] > 0).any()
    for m in range(n):
        r = rows[off[m]:off[m + 1]]
        tail = r[len(r) - int(c3["n_episode"][m]):]
        check_market(env, m, "current", tail, a, partial=int(sel[m]))
        check_market(env, m, "previous", r[:0] if sel[m] else r[:int(c1["n_previous"][m])], a)
    env.close()


def test_tape_off_and_bad_arguments_are_refused():
    import ctypes
    from gym_continuousdoubleauction_amd import CDAVecEnv, CDAEnv, _capi as K
    from gym_continuousdoubleauction_amd._lib import lib
    from gym_continuousdoubleauction_amd.tape import STAT_FIELDS, exec_from_records
    n, a = 16, 4
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 32, "is_render": False}, n)
    env.reset(seed=1)
    stats = torch.full((n, a, 16), -5, dtype=torch.int64, device=env.device)
    marks = torch.full((n, a, 8, 2, 4), -5, dtype=torch.int64, device=env.device)
    hz = (ctypes.c_int32 * 9)(1, 5, 20, 0, 0, 0, 0, 0, 0)
    call = lambda first, cnt, which, h, nh, s=0, k=0: lib().cda_tape_exec(env._h, first, cnt, which, h, nh, stats.data_ptr() + s, marks.data_ptr() + k, None, None)      # noqa: E731
    with pytest.raises(RuntimeError, match="enable_tape"):
        env.tape_exec()
    assert call(0, n, 0, hz, 3) == K.ERR_UNSUPPORTED
    env.enable_tape(256)
    for t in range(8):
        env.step(*env.random_actions(t, action_seed=2))
    for kw in ({"horizons": ()}, {"horizons": tuple(range(9))}, {"horizons": (1, -1)}, {"first_market": n}, {"first_market": -1}, {"first_market": 8, "n_markets": 9},
               {"n_markets": 0}, {"episode": "last"}):
        with pytest.raises(ValueError):
            env.tape_exec(**kw)
    # the library refuses them itself, without a launch: the buffers keep their fill
    for first, cnt, which, nh in ((0, n + 1, 0, 3), (-1, 4, 0, 3), (4, 0, 0, 3), (0, n, 2, 3), (0, n, -1, 3), (0, n, 0, 0), (0, n, 0, 9), (0, n, 0, -1)):
        assert call(first, cnt, which, hz, nh) == K.ERR_INVALID, (first, cnt, which, nh)
    assert call(0, n, 0, (ctypes.c_int32 * 3)(1, -2, 3), 3) == K.ERR_INVALID
    assert call(0, n, 0, hz, 3, s=4) == K.ERR_INVALID and call(0, n, 0, hz, 3, k=4) == K.ERR_INVALID      # (not 8-byte aligned)
    assert call(0, n, 0, None, 3) == K.ERR_INVALID
    torch.cuda.synchronize()
    assert int((stats != -5).sum()) == 0 and int((marks != -5).sum()) == 0
    # ... and asked properly - the horizons in device memory this time - the tables are filled and equal the method's
    dev_hz = torch.tensor([1, 5, 20], dtype=torch.int32, device=env.device)
    m3 = torch.empty((n, a, 3, 2, 4), dtype=torch.int64, device=env.device)
    torch.cuda.synchronize()
    assert lib().cda_tape_exec(env._h, 0, n, 0, dev_hz.data_ptr(), 3, stats.data_ptr(), m3.data_ptr(), None, None) == K.OK
    torch.cuda.synchronize()
    want = env.tape_exec((1, 5, 20))
    assert torch.equal(stats, want[0]) and torch.equal(m3, want[1]) and int(stats[:, :, 5].sum()) > 0
    env.close()
    # the one-market facade
    rec, fx = G.load("tick5_s301"), _fixture("tick5_s301")
    one = CDAEnv(rec["config"])
    with pytest.raises(RuntimeError, match="enable_tape"):
        one.tape_exec()
    one.enable_tape(64)
    one.reset(seed=int(rec["seed"]))
    r = one.tape_exec((2, 9))
    agents = int(rec["config"]["num_of_agents"])
    assert set(r) == set(STAT_FIELDS) | {"markouts", "horizons", "info"} and r["horizons"].tolist() == [2, 9] and r["info"].tolist() == [0, 0, 0, 0]
    empty = exec_from_records(np.zeros((0, 8), np.int32), agents, (2, 9))
    assert all(np.array_equal(r[f], empty[0][:, i]) for i, f in enumerate(STAT_FIELDS)) and np.array_equal(r["markouts"], empty[1])
    one.close()


def test_reading_is_not_steering():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    n, a = 128, 4
    cfg = {"num_of_agents": a, "init_cash": 1000000, "max_step": 40, "is_render": False, "auto_reset": True}
    plain, read = CDAVecEnv(cfg, n, with_info=False), CDAVecEnv(cfg, n, with_info=False)
    sample = list(range(0, n, 9)) + [n - 1]
    for e in (plain, read):
        e.enable_tape(1024)
        e.reset(seed=77)
    for t in range(96):
        acts = plain.random_actions(t, action_seed=6)
        plain.step(*acts)
        read.step(*acts)
        if t % 13 == 5:
            for w in ("current", "previous"):
                x = read.tape_exec(episode=w)
                y = read.tape_exec(episode=w)
                assert all(torch.equal(p, q) for p, q in zip(x, y))                   # and twice the same: nothing depends on scheduling
    for i in sample:
        assert bytes(plain.get_state(i)) == bytes(read.get_state(i)), i
    for k, v in plain.tape_counts().items():
        assert torch.equal(v, read.tape_counts()[k]), k
    assert torch.equal(plain.drain_tape()[0], read.drain_tape()[0])
    plain.close(); read.close()


def test_evaluate_adds_an_execution_block_that_equals_the_host_fold(tmp_path):
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    from gym_continuousdoubleauction_amd.tape import STAT, STAT_ADDITIVE, exec_from_records, exec_summary, load_tape
    N, A, S, hz = 48, 4, 256, (1, 5)
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": S, "is_render": False, "auto_reset": True}
    own = [(S, 100, 48)[i % 3] for i in range(N)]
    env = CDAVecEnv(cfg, n_markets=N, with_info=False, market_configs=[{"max_step": s} for s in own])
    pol = mlp.FusedPolicy("cuda:0", seed=5)
    plain = evaluate(env, pol, opponents=["random", "random"], trained_slots=2, episodes=1, seed=9)
    path = str(tmp_path / "tape.npz")
    keep = {}
    res = evaluate(env, pol, opponents=["random", "random"], trained_slots=2, episodes=1, seed=9, tape=path, keep=keep, exec_horizons=hz)
    # without the option: the keys of the parent, and the same figures with it
    assert set(plain) == {"mode", "episodes", "nav_conservation_violations", "modules", "config", "agent_steps_per_s", "summary"}
    assert set(res) == set(plain) | {"execution"} and res["summary"] == plain["summary"]
    for name, block in plain["modules"].items():
        assert set(block) == {"agent_episodes", "episode_return_mean", "episode_return_std", "episode_nav_mean", "trades", "rejections", "maker_fill_ratio_mean",
                              "reward_term_sums", "slots"}
        assert set(res["modules"][name]) == set(block) | {"execution"} and all(res["modules"][name][k] == v for k, v in block.items())
    # the host fold: every market's last finished episode from the saved tape, through the restatement, summed per module
    z = load_tape(path)
    rows, market, episode, modules = z["records"], z["market"], z["episode"], z["modules"]
    names = [str(x) for x in z["module_names"]]
    assert names == ["policy", "opponent_0", "opponent_1"] == list(res["modules"])
    want_s = np.zeros((3, 16), np.int64); want_s[:, 14:] = -1
    want_m = np.zeros((3, 2, 2, 4), np.int64)
    steps = np.zeros(3, np.int64)
    n_rows = 0
    for m in range(N):
        r = rows[(market == m) & (episode == S // own[m] - 1)]
        n_rows += len(r)
        s, mk = exec_from_records(r, A, hz)
        assert np.array_equal(keep["execution_tables"]["stats"][m], s) and np.array_equal(keep["execution_tables"]["markouts"][m], mk), m
        for x in range(A):
            i = modules[m, x]
            for f in STAT_ADDITIVE:
                want_s[i, STAT[f]] += s[x, STAT[f]]
            want_s[i, STAT["max_long"]] = max(want_s[i, STAT["max_long"]], s[x, STAT["max_long"]])
            want_s[i, STAT["max_short"]] = min(want_s[i, STAT["max_short"]], s[x, STAT["max_short"]])
            want_s[i, STAT["last_step"]] = max(want_s[i, STAT["last_step"]], s[x, STAT["last_step"]])
            if s[x, STAT["first_step"]] >= 0:
                want_s[i, STAT["first_step"]] = s[x, STAT["first_step"]] if want_s[i, STAT["first_step"]] < 0 else min(want_s[i, STAT["first_step"]], s[x, STAT["first_step"]])
            want_m[i] += mk[x]
            steps[i] += s[:, STAT["last_step"]].max() + 1
    about = res["execution"]
    assert about["horizons"] == [1, 5] and about["episode"] == "previous" and about["markets"] == N and about["records"] == n_rows > N
    assert about["records_lost"] == 0 and about["partial_markets"] == 0
    for i, name in enumerate(names):
        block = res["modules"][name]["execution"]
        assert block["stats"] == want_s[i].tolist() and block["markout_rows"] == want_m[i].tolist() and block["position_steps"] == int(steps[i]), name
        ratios = exec_summary(want_s[i], want_m[i], horizons=hz, steps=int(steps[i]))
        assert all(block[k] == v for k, v in ratios.items()), name
        assert block["markouts"]["k1"]["maker"]["fills"] + block["markouts"]["k1"]["maker"]["open_fills"] == int(want_s[i, STAT["maker_fills"]])
    assert res["modules"]["policy"]["execution"]["turnover"] > 0
    with pytest.raises(ValueError, match="tape"):
        evaluate(env, pol, opponents=["random"], episodes=1, seed=9, exec_horizons=hz)
    with pytest.raises(ValueError):
        evaluate(env, pol, opponents=["random"], episodes=1, seed=9, tape=path, exec_horizons=(-1,))
    assert not env.tape_enabled
    env.close()
