"""GPU: the action sampler of the policy kernels (sample_action / sample_head / u01 / rollout_key of csrc/cda_mlp_dev.inc, inlined into every
cda_mlp_policy_step* instance, k_policy_step and the league epilogue; k_policy_sample of csrc/cda_ppo.hip) against tests/sampler_ref.py, the float64 host
restatement of the documented law (include/cda_mlp.h "Sampling law"), SAMPLE BY SAMPLE, and against the law itself on constructed distributions.

Bounds, and where they come from:

* Categorical heads: exact equality with the class of u_exact wherever u_exact lies more than EPS = 1e-5 from every boundary of the float64 CDF; inside the
  band ("undecided") the device's class must lie between the classes of u - EPS and u + EPS.  EPS is derived, not measured: a head has at most 10 terms
  __expf(l_j - max), each within ~2.5e-7 absolute; ten float32 additions ~6e-7; u * s one rounding: ~3e-6 in all, times 3.  At most UNDECIDED_CAP = 2e-3 of a
  case's samples may be undecided (the law alone: 2 EPS x 19 boundaries ~ 4e-4).
* Gaussian heads: n_dev = (a_cont - mu) exp(-log_std) against the float64 Box-Muller value of the kernels' two float32 uniforms.  The bound is the accuracy
  of __logf / __cosf / __sinf on gfx950: measured (MEASURED_GAUSS below), asserted at 4 x that, never above 1e-4 (every structural error - wrong uniform,
  swapped sin / cos, wrong half-word, wrong key - moves n by O(1)).
* size_mean / size_sigma: float64 tanh / sigmoid of the device's a_cont, 1e-6.  logp: the float64 log-probability of the device's action, 2e-4.

Measured on an MI355X (every test prints its figures before it asserts):
  largest |n_dev - n_ref|: 1.84e-6 (the 4.2 M samples of each law test; 1.1e-6 .. 1.6e-6 in every other case)  ->  MEASURED_GAUSS = 1.9e-6, asserted 7.6e-6
  undecided shares (cap 2e-3): policy_step's seven cases 1.2e-4 .. 4.8e-4; rollout steps (4120 samples each, both paths, both rollouts) 0 .. 7.3e-4;
  league slots per net 1.5e-4 .. 6.8e-4; act_fused 3.3e-4 / 6.7e-4; law tests (4.2 M) 3.0e-4 .. 3.9e-4; the edge launches (65536) 3.2e-4 .. 4.9e-4;
  no decided sample disagreed anywhere.  size_mean / size_sigma within 2.1e-7, logp within 2.7e-6.
With u01's clamp removed (the parent's library) exactly the u == 1 edge tests fail: the twelve categorical ones (3 heads x 4 paths: the last class, logit -100,
is drawn and the recorded logp is -105.9 .. -106.6) and policy_step's radius case (r = 0 where the law's clamped uniform gives 3.45e-4).

The keys (include/cda_mlp.h): cda_mlp_policy_step and the league step take (seed, *counter, draw) as given; a RolloutChains rollout uses its per-chain rollout
counter - 1 for the first rollout, bumped by one at the end of each - and draw = the step index t inside the rollout; cda_policy_sample (ActorCritic.act_fused)
uses (seed, its device counter - 0 at first, bumped by every call) and no draw term."""
import functools
import math

import numpy as np
import pytest
import torch

import mlp_variants as V
import sampler_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
#: the largest |n_dev - n_ref| seen on an MI355X over every case of this file, rounded up (module docstring): tests/mlp_variants.py holds the figure and _compare
MEASURED_GAUSS, GAUSS_BOUND, ACTION_KEYS = V.MEASURED_GAUSS, V.GAUSS_BOUND, V.ACTION_KEYS          # (1.9e-6, asserted at 4 x that = 7.6e-6)


def _theta(n_hist=4, seed=3, scale=2.0, sd=False, vfs=False):
    from gym_continuousdoubleauction_amd import mlp
    th = mlp.init_theta(42 * n_hist, generator=torch.Generator().manual_seed(seed), state_dependent_log_std=sd, vf_share_layers=vfs)
    th[:mlp.layout(n_hist).OFF_LS] *= scale
    return th


def _policy(n_hist=4, seed=3, scale=2.0, sd=False, act="tanh", vfs=False):
    from gym_continuousdoubleauction_amd import mlp
    return mlp.FusedPolicy(DEV, theta=_theta(n_hist, seed, scale, sd, vfs), state_dependent_log_std=sd, activation=act, vf_share_layers=vfs)


def _constant_theta(logits22, means=(0.25, -0.5), log_std=(-0.5, -0.7), seed=3):
    """a parameter vector whose output layer has zero weights and the wanted outputs in its bias: every row's 24 outputs are exactly those, whatever the observation"""
    from gym_continuousdoubleauction_amd import mlp
    th = _theta(4, seed, 1.0)
    th[mlp.OFF_WO:mlp.OFF_BO] = 0
    th[mlp.OFF_BO:mlp.OFF_LS] = 0
    th[mlp.OFF_BO:mlp.OFF_BO + 22] = torch.from_numpy(np.asarray(logits22, np.float32))
    th[mlp.OFF_BO + 22:mlp.OFF_BO + 24] = torch.tensor(means)
    th[mlp.OFF_LS:] = torch.tensor(log_std)
    return th


def _row_of(th):
    """the 32 outputs and the log-stds of a constant network (float32)"""
    from gym_continuousdoubleauction_amd import mlp
    return th[mlp.OFF_BO:mlp.OFF_LS].numpy().copy(), th[mlp.OFF_LS:].numpy().copy()


def _obs(n, width=168, seed=5):
    x = torch.randn(n, width, generator=torch.Generator().manual_seed(seed)) * 1.5
    x[:, ::7] = 0.0
    return x


_log_std, _flat, _compare = V.log_std_rows, V.flat, V.compare          # (shared with tests/test_hip_mlp_variants.py: every compiled object's sampling launch)


# ---- section 3: per-sample agreement -------------------------------------------------------------------------------------------------------------------------
# every axis value of the issue appears: n_hist 1 / 4 / 8, tanh / relu, vf_share_layers off / on, the state-dependent log-std head off / on, A 1 / 4 / 5 / 16, N not
# a multiple of the 32-row tile, a sub-range, draw 0 / 1 / 7 / 2^31 - 1, counter 0 / 5 / 2^40, seed 0 / 2^64 - 1
STEP_CASES = [
    # n_hist, act,   vfs,   sd,    A,  N,    first, n,    draw,          counter, seed
    (4, "tanh", False, False, 4, 2053, 0, None, 0, 0, 0),
    (1, "relu", False, False, 1, 8197, 0, None, 1, 5, 2 ** 64 - 1),
    (8, "tanh", True, False, 5, 1701, 0, None, 7, 2 ** 40, 0),
    (4, "relu", True, True, 16, 517, 0, None, 2 ** 31 - 1, 5, 2 ** 64 - 1),
    (4, "tanh", False, True, 4, 2300, 37, 2101, 7, 2 ** 40, 12345),
    (8, "relu", False, False, 4, 2053, 0, None, 1, 0, 2 ** 64 - 1),
    (1, "tanh", True, True, 5, 1701, 0, None, 0, 5, 0),
]


@pytest.mark.parametrize("n_hist,act,vfs,sd,A,N,first,n,draw,counter,seed", STEP_CASES)
def test_policy_step_draws_the_restated_sample(n_hist, act, vfs, sd, A, N, first, n, draw, counter, seed):
    p = _policy(n_hist, seed=11 + n_hist, sd=sd, act=act, vfs=vfs)
    obs = _obs(N, 42 * n_hist, seed=31).to(DEV)
    ctr = torch.full((1,), counter, dtype=torch.int64, device=DEV)
    from gym_continuousdoubleauction_amd import mlp
    outs = mlp._act_outputs(N, A, DEV)
    for v in outs.values():
        v.fill_(5)
    p.policy_step(obs, A, seed=seed, counter=ctr, draw=draw, first_market=first, n_markets=n, outs=outs)
    torch.cuda.synchronize()
    out = p.forward(obs).cpu().numpy()
    rows = np.arange(first, N if n is None else first + n)
    i = (rows[:, None] * A + np.arange(A)[None, :]).reshape(-1)
    take = lambda a: np.repeat(a[rows], A, axis=0)                               # noqa: E731
    _compare(f"policy_step h{n_hist} {act} vfs{int(vfs)} sd{int(sd)} A{A} N{N} draw{draw} ctr{counter}", _flat(outs, rows), R.rollout_key(seed, counter, draw), i,
             take(out), take(_log_std(p, out)))
    assert np.array_equal(outs["value"].cpu().numpy()[rows], out[rows, 24])
    rest = np.setdiff1d(np.arange(N), rows)
    for k in ACTION_KEYS:                                                        # a sub-range leaves the rest alone
        assert (outs[k].cpu().numpy()[rest] == 5).all(), k


@pytest.mark.parametrize("one_launch", ["2", "0"])
def test_rollout_chains_draw_the_restated_samples_at_every_step(one_launch, monkeypatch):
    """both paths of a rollout (CDA_POLICY_STEP=2: k_policy_step, the policy inside the env's step kernel; 0: policy kernel + step kernel), 2 chains, graphs on.
    Key: (seed, the chain's rollout counter: 1 for the first rollout, 2 for the second, draw = the step index t)."""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd._lib import lib
    monkeypatch.setenv("CDA_POLICY_STEP", one_launch)
    N, A, T, seed = 1030, 4, 5, 99
    cfg = {"num_of_agents": A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=N, with_info=False)
    assert lib().cda_policy_step_supported(env._h) == 1
    p = _policy(4, seed=29)
    env.reset(seed=500)
    roll = mlp.RolloutChains(env, p, T, groups=2, seed=seed, use_graphs=True)
    i = np.arange(N * A)
    for rnd in range(2):
        buf = roll.run()
        torch.cuda.synchronize()
        assert roll.graphs is not None and int(roll.counter.item()) == 1 + rnd
        for t in range(T):
            out = p.forward(buf["obs"][t]).cpu().numpy()
            dev = _flat({k: buf[k][t] for k in ACTION_KEYS})
            _compare(f"rollout one_launch={one_launch} rollout {rnd} step {t}", dev, R.rollout_key(seed, 1 + rnd, t), i, np.repeat(out, A, axis=0),
                     np.repeat(_log_std(p, out), A, axis=0))
    env.close()


def _bank(N, A, k, frozen, seed=3, scale=2.0):
    from gym_continuousdoubleauction_amd import mlp
    bank = mlp.PolicyBank(DEV, N, A, k, max_frozen=max(frozen, 1), seed=seed, random_seed=4242)
    for q in range(k):
        bank.policies[q].theta.copy_(_theta(4, seed + 100 * q, scale)); bank.policies[q].pack()
    for f in range(frozen):
        row = bank.snapshot(0)
        th = _theta(4, seed + 1000 + f, scale)
        th[mlp.OFF_LS:] = torch.tensor([-0.3 - 0.1 * f, -0.7])
        bank.theta[row].copy_(th)
        bank.wb[row].copy_(mlp.FusedPolicy(DEV, theta=th).wb)
    torch.cuda.synchronize()
    return bank


def test_league_step_draws_the_restated_sample_per_slot():
    """network slots: the restatement with that slot's net's outputs, the shared key and the global sample index; random-module slots: include/cda_random_agents.h
    restated in numpy with the key the epilogue documents (random_seed + counter * 0x9e3779b97f4a7c15, market, draw, slot)"""
    from gym_continuousdoubleauction_amd import mlp
    N, A, k, F = 6100, 8, 2, 2
    seed, counter, draw = 77, 5, 3
    bank = _bank(N, A, k, F)
    sn = torch.randint(-1, k + F, (N, A), generator=torch.Generator().manual_seed(9), dtype=torch.int32)
    sn[:, 0], sn[:, 1] = 0, 1
    bank.set_slots(sn)
    obs = _obs(N, seed=31).to(DEV)
    ctr = torch.full((1,), counter, dtype=torch.int64, device=DEV)
    o = bank.act(obs, seed, ctr, draw, greedy=False)
    torch.cuda.synchronize()
    snc = sn.numpy()
    key = R.rollout_key(seed, counter, draw)
    flat = _flat(o)
    for net in range(k + F):
        pol = mlp.FusedPolicy(DEV, theta=bank.theta[net].cpu())
        out = pol.forward(obs).cpu().numpy()
        i = np.nonzero((snc == net).reshape(-1))[0]
        assert i.size > 6000
        _compare(f"league net {net}", {kk: v[i] for kk, v in flat.items()}, key, i, out[i // A], _log_std(pol, out)[i // A])
    m, a = np.nonzero(snc < 0)
    want = R.random_module((bank.random_seed + counter * R.K_RANDOM) & R.M64, m, draw, a)
    for name, w in zip(("category", "size_mean", "size_sigma", "price", "price_offset"), want):
        assert np.array_equal(o[name].cpu().numpy()[m, a], w), name
    assert (o["logp"].cpu().numpy()[m, a] == 0).all() and (o["a_cont"].cpu().numpy()[m, a] == 0).all()


def _actor_critic(bias24=None, seed=2):
    from gym_continuousdoubleauction_amd import ppo
    torch.manual_seed(seed)
    m = ppo.ActorCritic(168).to(DEV)
    with torch.no_grad():
        if bias24 is None:
            m.out.weight.mul_(3.0)
        else:
            m.out.weight.zero_(); m.out.bias.zero_()
            m.out.bias[:24] = torch.from_numpy(np.asarray(bias24, np.float32)).to(DEV)
    return m


def test_act_fused_draws_the_restated_sample():
    """cda_policy_sample (k_policy_sample: the older copy of the sampler): key = (seed, its own device counter, no draw term) - the first call draws with counter 0,
    the next with 1; one row per market serving its A agents (sample index = row * A + agent), and one row per sample"""
    from gym_continuousdoubleauction_amd import ppo
    n, a, seed = 3001, 4, 2 ** 64 - 1
    m = _actor_critic()
    obs = _obs(n, seed=8).to(DEV)
    st = ppo.new_sampler_state(seed, DEV)
    ls = m.log_std.detach().cpu().numpy()
    with torch.no_grad():
        out = m.trunk_packed(obs).float().cpu().numpy()
        for call in range(2):
            acts, logp, val, env_acts = m.act_fused(obs, n, a, st, shared=True)
            torch.cuda.synchronize()
            dev = {"category": acts[0].cpu().numpy(), "price": acts[1].cpu().numpy(), "price_offset": acts[2].cpu().numpy(), "a_cont": acts[3].cpu().numpy(),
                   "logp": logp.cpu().numpy(), "size_mean": env_acts[1].cpu().numpy().reshape(-1), "size_sigma": env_acts[2].cpu().numpy().reshape(-1)}
            assert np.array_equal(env_acts[0].cpu().numpy().reshape(-1), dev["category"]) and np.array_equal(env_acts[3].cpu().numpy().reshape(-1), dev["price"])
            assert np.array_equal(env_acts[4].cpu().numpy().reshape(-1), dev["price_offset"])
            _compare(f"act_fused shared call {call}", dev, R.rollout_key(seed, call, 0), np.arange(n * a), np.repeat(out, a, axis=0), ls)
        acts, logp, val, env_acts = m.act_fused(obs, n, 1, ppo.new_sampler_state(5, DEV), shared=False)
        torch.cuda.synchronize()
        dev = {"category": acts[0].cpu().numpy(), "price": acts[1].cpu().numpy(), "price_offset": acts[2].cpu().numpy(), "a_cont": acts[3].cpu().numpy(),
               "logp": logp.cpu().numpy(), "size_mean": env_acts[1].cpu().numpy().reshape(-1), "size_sigma": env_acts[2].cpu().numpy().reshape(-1)}
        _compare("act_fused per-sample rows", dev, R.rollout_key(5, 0, 0), np.arange(n), out, ls)


TIE = np.array([1, 3, 3, 0, 3, -1, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 2, 2], np.float32)       # exact ties: the lowest index wins (1 | 0 | 1)


def test_greedy_actions_are_the_mode_with_ties_to_the_lowest_index():
    """FusedPolicy.act (MODE_GREEDY) and the league's greedy step (MODE_LEAGUE_GREEDY): argmax of each head of the device's own outputs, the Gaussian means; and on a
    network whose outputs hold exact ties"""
    from gym_continuousdoubleauction_amd import mlp
    N, A = 1031, 4
    obs = _obs(N, seed=12).to(DEV)
    for tag, p in (("random", _policy(4, seed=41, sd=True)), ("ties", mlp.FusedPolicy(DEV, theta=_constant_theta(TIE)))):
        o = p.act(obs, A)
        torch.cuda.synchronize()
        out = p.forward(obs).cpu().numpy()
        ref = R.mode(out, _log_std(p, out))
        for head, _, _ in R.HEADS:
            assert np.array_equal(o[head].cpu().numpy(), np.repeat(ref[head][:, None], A, axis=1)), (tag, head)
        assert np.array_equal(o["a_cont"].cpu().numpy(), np.repeat(out[:, None, 22:24], A, axis=1))
        assert np.abs(o["logp"].cpu().numpy() - ref["logp"][:, None]).max() <= 2e-4
        assert np.abs(o["size_mean"].cpu().numpy() - ref["size_mean"][:, None]).max() <= 1e-6 and np.abs(o["size_sigma"].cpu().numpy() - ref["size_sigma"][:, None]).max() <= 1e-6
        if tag == "ties":
            assert (o["category"] == 1).all() and (o["price"] == 0).all() and (o["price_offset"] == 1).all()
    bank = mlp.PolicyBank(DEV, N, A, 2, max_frozen=1, random_seed=7)
    bank.policies[0].theta.copy_(_constant_theta(TIE)); bank.policies[0].pack()
    bank.policies[1].theta.copy_(_theta(4, 55, 2.0)); bank.policies[1].pack()
    sn = torch.randint(0, 2, (N, A), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    bank.set_slots(sn)
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    o = bank.act(obs, 1, ctr, 0, greedy=True)
    torch.cuda.synchronize()
    snc = sn.numpy()
    out1 = bank.policies[1].forward(obs).cpu().numpy()
    ref1 = R.mode(out1, _log_std(bank.policies[1], out1))
    for head, want0 in (("category", 1), ("price", 0), ("price_offset", 1)):
        got = o[head].cpu().numpy()
        assert (got[snc == 0] == want0).all(), head
        assert np.array_equal(got[snc == 1], np.repeat(ref1[head][:, None], A, axis=1)[snc == 1]), head


# ---- section 4: the law on constructed distributions (every threshold is first met by the restatement's own samples: tests/test_sampler_ref_host.py) --------------
def _law_step(th, counter=R.LAW_COUNTER, draw=R.LAW_DRAW, keys=ACTION_KEYS):
    from gym_continuousdoubleauction_amd import mlp
    p = mlp.FusedPolicy(DEV, theta=th)
    obs = torch.randn(R.LAW_MARKETS, 168, generator=torch.Generator(DEV).manual_seed(1), device=DEV)
    row, ls = _row_of(th)
    assert np.array_equal(p.forward(obs[:4096]).cpu().numpy()[:, :24], np.repeat(row[None, :24], 4096, axis=0))          # the outputs ARE the bias, bit for bit
    ctr = torch.full((1,), counter, dtype=torch.int64, device=DEV)
    o = p.policy_step(obs, R.LAW_AGENTS, seed=R.LAW_SEED, counter=ctr, draw=draw)
    torch.cuda.synchronize()
    return _flat({k: o[k] for k in keys}), row, ls


@pytest.mark.parametrize("name", sorted(R.law_distributions()))
def test_the_sampler_follows_the_law_on_constructed_distributions(name):
    """4 M samples of one launch from constant logits: goodness of fit of each head, classes of probability zero never drawn, the joint 9 x 10 x 3 table against the
    product law, offset against the sign and the terciles of n0, 64 equiprobable bins / tails / correlations of the normals - and every sample against the restatement"""
    logits = R.law_distributions()[name]
    dev, row, ls = _law_step(_constant_theta(logits))
    x = dev["a_cont"].astype(np.float64)
    n = (x - row[22:24].astype(np.float64)) * np.exp(-ls.astype(np.float64))
    res = R.law_checks(logits, dev["category"].astype(np.int64), dev["price"].astype(np.int64), dev["price_offset"].astype(np.int64), n[:, 0], n[:, 1])
    print(f"[sampler] law {name}: " + " ".join(f"{k}={v:.3g}" for k, (v, _) in res.items()))
    bad = {k: v for k, (v, ok) in res.items() if not ok}
    assert not bad, (name, bad)
    _compare(f"law {name}", dev, R.rollout_key(R.LAW_SEED, R.LAW_COUNTER, R.LAW_DRAW), np.arange(R.LAW_N), row, ls)


def test_serial_structure_of_the_keys():
    """the same sample at draws t, t + 1; samples i, i + 1 of one draw; the same (i, draw) at counters c, c + 1: independent categories (9 x 9 tables, p > 1e-6);
    equal keys give equal bits"""
    th = _constant_theta(R.law_distributions()["linspace"])
    keys = ("category", "a_cont", "logp")
    base, _, _ = _law_step(th, keys=keys)
    again, _, _ = _law_step(th, keys=keys)
    assert all(np.array_equal(base[k].view(np.uint32), again[k].view(np.uint32)) for k in keys)
    c = base["category"].astype(np.int64)
    nxt_draw = _law_step(th, draw=R.LAW_DRAW + 1, keys=keys)[0]["category"].astype(np.int64)
    nxt_ctr = _law_step(th, counter=R.LAW_COUNTER + 1, keys=keys)[0]["category"].astype(np.int64)
    ps = {"draw": R.serial_p(c, nxt_draw), "counter": R.serial_p(c, nxt_ctr), "neighbour": R.serial_p(c[:-1], c[1:])}
    print(f"[sampler] serial: {ps}")
    assert all(v > R.P_MIN for v in ps.values()), ps
    assert not np.array_equal(c, nxt_draw) and not np.array_equal(c, nxt_ctr)


# ---- section 5: the u == 1 edge --------------------------------------------------------------------------------------------------------------------------------
EDGE_N, EDGE_A = 16384, 4
R_TOP = math.sqrt(-2.0 * math.log(R.U_MAX))           # the Box-Muller radius of the top draw: 3.45e-4 (0 if the uniform were 1.0)


@functools.lru_cache(maxsize=None)
def _edge(name):
    """(seed, i): sample i < EDGE_N * EDGE_A draws k = 2^24 - 1 for uniform `name` at (seed, counter 0, draw 0) - found and asserted with the restatement alone"""
    hit = R.find_top_draw(name, EDGE_N * EDGE_A)
    assert hit is not None
    seed, i = hit
    assert int(R.draws24(R.rollout_key(seed, 0, 0), np.array([i]))[name][0]) == R.TOP and float(R.u_f32(R.TOP)) == 1.0 and i < EDGE_N * EDGE_A
    return seed, i


def _edge_logits(name):
    """the head under test gives its LAST class logit -100 (probability 0); the other heads are uniform"""
    l = np.zeros(24, np.float32)
    for head, lo, hi in R.HEADS:
        if head == name:
            l[hi - 1] = R.DEAD
    l[22:24] = (0.25, -0.5)
    return l


def _edge_assert(tag, name, cat, price, off, a_cont, logp, ls=(-0.5, -0.7)):
    last = {"category": (cat, R.N_CAT - 1), "price": (price, R.N_PRICE - 1), "price_offset": (off, R.N_OFF - 1)}
    print(f"[sampler] edge {tag} {name}: action ({int(cat)}, {int(price)}, {int(off)}) a_cont ({float(a_cont[0])!r}, {float(a_cont[1])!r}) logp {float(logp)!r}")
    if name in last:
        got, dead = last[name]
        assert int(got) != dead, (tag, name, "the sampler drew a class of probability zero")
    else:
        # the radius' top draw: |n| = sqrt(-2 ln(1 - 2^-24)) = 3.45e-4 (a_cont = mu to within that; exactly mu where the uniform is 1.0); the angle's: any finite sample
        n = (np.asarray(a_cont, np.float64) - np.array([0.25, -0.5])) * np.exp(-np.asarray(ls, np.float64))
        assert np.isfinite(n).all()
        if name == "radius":
            assert np.abs(n).max() <= R_TOP + GAUSS_BOUND, (tag, n)
    assert math.isfinite(float(logp)) and float(logp) > -20.0, (tag, name, float(logp))


@pytest.mark.parametrize("name", list(R.UNIFORMS))
def test_the_top_draw_takes_no_class_of_probability_zero_policy_step(name):
    from gym_continuousdoubleauction_amd import mlp
    seed, i = _edge(name)
    th = _constant_theta(_edge_logits(name)[:22])
    p = mlp.FusedPolicy(DEV, theta=th)
    o = p.policy_step(_obs(EDGE_N, seed=3).to(DEV), EDGE_A, seed=seed, counter=torch.zeros(1, dtype=torch.int64, device=DEV), draw=0)
    torch.cuda.synchronize()
    d = _flat(o)
    _edge_assert("policy_step", name, d["category"][i], d["price"][i], d["price_offset"][i], d["a_cont"][i], d["logp"][i])
    row, ls = _row_of(th)
    _compare(f"edge policy_step {name}", d, R.rollout_key(seed, 0, 0), np.arange(EDGE_N * EDGE_A), row, ls)


@pytest.mark.parametrize("name", list(R.UNIFORMS))
def test_the_top_draw_takes_no_class_of_probability_zero_one_launch_rollout(name, monkeypatch):
    """k_policy_step: a one-step rollout whose chain counter is set to 0 (key = seed, 0, draw 0)"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd._lib import lib
    monkeypatch.setenv("CDA_POLICY_STEP", "2")
    seed, i = _edge(name)
    cfg = {"num_of_agents": EDGE_A, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}
    env = CDAVecEnv(cfg, n_markets=EDGE_N, with_info=False)
    assert lib().cda_policy_step_supported(env._h) == 1
    env.reset(seed=500)
    p = mlp.FusedPolicy(DEV, theta=_constant_theta(_edge_logits(name)[:22]))
    roll = mlp.RolloutChains(env, p, 1, groups=1, seed=seed, use_graphs=False)
    roll._counters.zero_()
    buf = roll.run()
    torch.cuda.synchronize()
    assert int(roll.counter.item()) == 0
    d = _flat({k: buf[k][0] for k in ACTION_KEYS})
    _edge_assert("k_policy_step", name, d["category"][i], d["price"][i], d["price_offset"][i], d["a_cont"][i], d["logp"][i])
    env.close()


@pytest.mark.parametrize("name", list(R.UNIFORMS))
def test_the_top_draw_takes_no_class_of_probability_zero_league_step(name):
    from gym_continuousdoubleauction_amd import mlp
    seed, i = _edge(name)
    bank = mlp.PolicyBank(DEV, EDGE_N, EDGE_A, 1, max_frozen=1)
    bank.policies[0].theta.copy_(_constant_theta(_edge_logits(name)[:22])); bank.policies[0].pack()
    bank.set_slots(torch.zeros((EDGE_N, EDGE_A), dtype=torch.int32))
    o = bank.act(_obs(EDGE_N, seed=3).to(DEV), seed, torch.zeros(1, dtype=torch.int64, device=DEV), 0, greedy=False)
    torch.cuda.synchronize()
    d = _flat(o)
    _edge_assert("league_step", name, d["category"][i], d["price"][i], d["price_offset"][i], d["a_cont"][i], d["logp"][i])


@pytest.mark.parametrize("name", list(R.UNIFORMS))
def test_the_top_draw_takes_no_class_of_probability_zero_act_fused(name):
    from gym_continuousdoubleauction_amd import ppo
    seed, i = _edge(name)
    m = _actor_critic(_edge_logits(name))
    with torch.no_grad():
        m.log_std.copy_(torch.tensor([-0.5, -0.7]))
        acts, logp, _, _ = m.act_fused(_obs(EDGE_N, seed=3).to(DEV), EDGE_N, EDGE_A, ppo.new_sampler_state(seed, DEV), shared=True)
    torch.cuda.synchronize()
    _edge_assert("act_fused", name, acts[0][i].item(), acts[1][i].item(), acts[2][i].item(), acts[3][i].cpu().numpy(), logp[i].item())
