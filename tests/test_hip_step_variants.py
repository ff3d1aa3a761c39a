"""GPU: episode metrics and the trade tape on EVERY step-kernel instance (tests/step_variants.py states the matrix; tests/test_step_variants_host.py that its rows
hit what they claim).  Which instance steps a market is decided by the tile (cap256 / cap512), info tensors, the metrics, the tape and whether the market is cold
(csrc/cda_kernels.inc market_is_cold -> the out-of-line general build).  The instances tally in two ways: k_step<INFO, 1>, k_policy_step<1>, k_run_random<1> by a
compile-time switch; the general build (slow_step, slow_run_random) and every tape-writing instance (k_tstep<INFO>, slow_tstep, k_tape_run) from the market's ST_EP_ON
bit at run time - and an episode that ends on a cold market is handed back (`over == 2`) to the caller's episode_end_after_step.  Every row runs with the metrics on
against the CPU oracle's replay of the same actions: the collected tables, the step outputs, the ledger, the coldness, and - tape on - the tape of a metrics-off twin.

What the rows exercise, counted on the oracle (python -m pytest -s tests/test_step_variants_host.py prints every row's figures): 114 .. 125 episodes per row
(>= 2 N); in the 15 prefilled rows 37 .. 41 of the 38 / 41 markets end their first episode cold, 17 .. 41 of them with a fill in that step; the three prefilled
run_random rows hand 6 .. 9 markets that started hot to the general build in the middle of a launch; the six small-cash rows end 2 episodes `terminated` (the two
markets that start with a full done set), the two shallow 16-agent ones 3 more with a bankrupt account; no shallow row is ever cold; NAV is conserved in every episode."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_variants as V      # noqa: E402

pytestmark = pytest.mark.gpu

TAPE_CAPACITY = 4096


def _env(row, metrics):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    stepped = row["path"] in ("step", "step_info", "run_random")
    env = CDAVecEnv(V.config_of(row), n_markets=row["N"], with_info=row["path"] == "step_info", groups=row["groups"] if stepped else 1)
    assert env.book_capacity == row["tile"]
    if row["tape"]:
        env.enable_tape(TAPE_CAPACITY)
    env.reset(seed=row["seed"])
    V.prefill(env, row)
    if metrics:
        env.enable_episode_metrics(True)
    return env


def _step(env, acts):
    """one cda_step; groups > 1: the launches of the group chains (cda_step_groups), joined before the outputs are read"""
    out = env.step(*acts, pipelined=env.groups > 1)
    env.join()
    return out


def _orders(env):
    return env.book_counts()[:, :, 0].sum(1).cpu().numpy().astype(np.int64)


def _collect(env):
    return [t.cpu().numpy() for t in env.collect_episode_metrics()]


def _tape(env):
    rec, off, dropped = env.drain_tape()
    return {"records": rec.cpu().numpy(), "offsets": off.cpu().numpy(), "dropped": dropped.cpu().numpy(), **{k: v.cpu().numpy() for k, v in env.tape_counts().items()}}


def _same_tape(got, want, what):
    assert len(want["records"]) > 0 and int(want["dropped"].sum()) == 0, what
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, "tape", k)


def _assert_tables(row, dev, em, what):
    """the collected tables against the oracle's: integer and decimal-derived columns bit for bit, the f64 sums within the helper's bound - at 16 agents (600 and more
    (market, agent) rows per sum) the bound of the order of addition"""
    from episode_metrics_util import abs_sums, assert_tables_equal, assert_tables_within_order_bound
    if row["agents"] == 16:
        sums = abs_sums(em)
        assert_tables_within_order_bound(dev[0], dev[1], *em.table(), sums, what=what)
    else:
        assert_tables_equal(dev[0], dev[1], *em.table(), what=what)


def _same_bits(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = np.argwhere(g.view(np.uint8).reshape(g.shape + (-1,)) != w.view(np.uint8).reshape(w.shape + (-1,)))
    assert bad.size == 0, (what, bad[:4])


def _finish(row, env, run, what):
    """the ledger, the flags, the invariants and the second collection at the end of a row"""
    for i in V.ledger_markets(row):
        assert bytes(env.get_state(i)) == bytes(run.ora.get_state(i)), (what, "state of market", i)
    assert (env.flags() == 0).all() and (run.ora.flags() == 0).all() and (env.check_invariants() == 0).all(), what
    again = _collect(env)
    assert not again[0].any() and not again[1].any(), what


def _run_stepped(row):
    """step / step_info: the host's action stream, one cda_step per step"""
    what, acts, cut = V.name_of(row), V.actions_of(row), row["max_step"]
    env, run = _env(row, True), V.OracleRun(row)
    twin = _env(row, False) if row["tape"] else None
    outs, mid = [], None
    for t, a in enumerate(acts):
        if t == cut - 1:
            orders = _orders(env)                                          # before the step that ends the first episodes
        obs, rew, term, trunc, _ = _step(env, a)
        outs.append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), term.cpu().numpy().copy(), trunc.cpu().numpy().copy()))
        if twin is not None:
            _step(twin, a)
        if t == cut - 1:
            mid = _collect(env)
    end = _collect(env)
    run.play(acts[:cut])
    _assert_tables(row, mid, run.em, what + ": first collection")
    run.play(acts[cut:])
    _assert_tables(row, end, run.em, what + ": second collection")
    assert np.array_equal(orders, run.steps[cut - 1]["orders"]), (what, "resting orders before the first episode's last step")
    for t, (o, r, te, tr) in enumerate(outs):
        s = run.steps[t]
        _same_bits(o, s["obs"], (what, "obs", t)); _same_bits(r, s["reward"], (what, "reward", t))
        assert np.array_equal(te, s["terminated"]) and np.array_equal(tr, s["truncated"]), (what, "flags", t)
    if twin is not None:
        _same_tape(_tape(env), _tape(twin), what)
        twin.close()
    _finish(row, env, run, what)
    V.check_claims(row, V.claims(row, run.steps), run.em.violating)
    env.close(); run.close()


def _run_random(row):
    """three launches of cda_run_random (every market to its own episode end), each collected and followed by the reset of all markets"""
    what = V.name_of(row)
    env, run = _env(row, True), V.OracleRun(row)
    twin = _env(row, False) if row["tape"] else None
    n = row["max_step"] + 3                                                # (more steps than an episode has: every market stops at its own end)
    for launch in range(3):
        want = run.play_random(launch)
        obs, ret, term, trunc, steps = env.run_random(n, action_seed=V.action_seed(row, launch))
        _same_bits(obs.cpu().numpy(), want["obs"], (what, "obs", launch)); _same_bits(ret.cpu().numpy(), want["return"], (what, "return", launch))
        assert np.array_equal(term.cpu().numpy(), want["terminated"]) and np.array_equal(trunc.cpu().numpy(), want["truncated"]), (what, "flags", launch)
        assert np.array_equal(steps.cpu().numpy(), want["steps"]), (what, "steps", launch)
        assert np.array_equal(_orders(env), want["orders"]), (what, "resting orders behind launch", launch)
        for i, state in want["states"].items():
            assert bytes(env.get_state(i)) == state, (what, "state of market", i, "launch", launch)
        assert (env.flags() == 0).all() and (want["flags"] == 0).all() and (env.check_invariants() == 0).all(), (what, launch)
        if launch != 1:                                                    # launch 0: the (cold) first episodes alone; launches 1 and 2 together
            _assert_tables(row, _collect(env), run.em, f"{what}: collection behind launch {launch}")
        env.reset()                                                        # the launch has credited its episodes: the reset must not do it again
        if twin is not None:
            twin.run_random(n, action_seed=V.action_seed(row, launch))
            twin.reset()
    if twin is not None:
        _same_tape(_tape(env), _tape(twin), what)
        twin.close()
    _finish(row, env, run, what)
    V.check_claims(row, V.claims(row, run.steps), run.em.violating)
    env.close(); run.close()


def _run_rollout(row):
    """mlp.RolloutChains, four runs of max_step - 1 steps: the policy inside the step kernel (tile 256, up to 8 agents, tape off), else the policy launch and k_step /
    k_tstep.  The oracle replays the actions the policy took."""
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd._lib import lib
    what, H = V.name_of(row), V.horizon(row)
    env, run = _env(row, True), V.OracleRun(row)
    in_kernel = row["path"] == "rollout" and row["tile"] == 256 and row["agents"] <= 8
    assert lib().cda_policy_step_supported(env._h) == int(in_kernel), what
    roll = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=3), H, groups=row["groups"], seed=17)
    acts, outs, tables = [], [], {}
    for r in range(4):
        if r == 1:
            orders = _orders(env)                                          # max_step - 1 steps in: before the step that ends the first episodes
        buf = roll.run()
        torch.cuda.synchronize()
        b = {k: v.cpu().numpy().copy() for k, v in buf.items() if k in V.ACTION_KEYS + ("obs", "reward", "terminated", "truncated")}
        for t in range(H):
            acts.append(tuple(b[k][t] for k in V.ACTION_KEYS))
            outs.append((b["obs"][t + 1], b["reward"][t], b["terminated"][t].astype(bool), b["truncated"][t].astype(bool)))
        if r in (1, 3):                                                    # behind run 1 only first episodes have ended
            tables[r] = _collect(env)
    run.play(acts[:2 * H])
    _assert_tables(row, tables[1], run.em, what + ": first collection")
    run.play(acts[2 * H:])
    _assert_tables(row, tables[3], run.em, what + ": second collection")
    assert np.array_equal(orders, run.steps[H]["orders"]), (what, "resting orders before the first episode's last step")
    for t, (o, rw, te, tr) in enumerate(outs):
        s = run.steps[t]
        _same_bits(o, s["obs"], (what, "obs", t)); _same_bits(rw, s["reward"], (what, "reward", t))
        assert np.array_equal(te, s["terminated"]) and np.array_equal(tr, s["truncated"]), (what, "flags", t)
    if row["tape"]:                                                        # the twin: plain steps of the same actions, tape on, metrics off
        twin = _env(row, False)
        for a in acts:
            twin.step(*a)
        _same_tape(_tape(env), _tape(twin), what)
        twin.close()
    _finish(row, env, run, what)
    V.check_claims(row, V.claims(row, run.steps), run.em.violating)
    env.close(); run.close()


@pytest.mark.parametrize("row", V.ROWS, ids=V.NAMES)
def test_metrics_outputs_ledger_and_tape_equal_the_oracle_on_every_instance(row):
    """One row of the matrix, metrics on, 3 max_step + 2 steps.  Two collections - behind the step (launch, run) with which the prefilled first episodes have ended
    cold, and at the end - equal the oracle replay's tables (assert_tables_equal; 16 agents: assert_tables_within_order_bound), a further collection is all zeros;
    observation, reward, terminated and truncated of every step equal the oracle's bit for bit; get_state of every fourth market and of the last equals the
    oracle's; book_counts() before the first episodes' last step equals the oracle's resting-order counts (cold / spilled rows: > tile - agents in three quarters
    of the markets and more, asserted with the row's other claims on what was really played); tape rows: drained records, offsets, dropped and every tape_counts()
    array equal those of a twin env that plays the same seeds and actions with the tape on and the metrics off; flags() and check_invariants() are 0."""
    {"step": _run_stepped, "step_info": _run_stepped, "run_random": _run_random, "rollout": _run_rollout, "rollout_tape": _run_rollout}[row["path"]](row)


@pytest.mark.parametrize("name", ["aggr_s23", "A8_s3", "tick5_s301", "A16_aggr_s71", "reset_s51", "bankrupt_s61", "permshuf_s93", "perm8_s92", "bigbook8_waves_s203"])
def test_every_fixture_replays_to_the_reference_tape_with_the_metrics_on(name):
    """the nine tapes cut from the reference (tests/test_hip_tape.py FIXTURES), replayed with enable_episode_metrics(True): the same tape_len per step and the same rows
    as tests/golden/tape_<name>.npz.  bigbook8_waves_s203 puts slow_tstep under the tallies against the real reference."""
    import test_hip_tape as TT
    assert name in TT.FIXTURES and len(TT.FIXTURES) == 9
    TT.assert_fixture_replays_to_the_reference_tape(name, metrics=True)
