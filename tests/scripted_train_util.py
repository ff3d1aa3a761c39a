"""Test helpers for training against scripted opponents (tests/test_hip_scripted_train.py): the fused update's gradient when a shared policy owns the LEADING k
slots of every row (update_check_util's stages, its bands), the host statement of the league's assignment with scripted pool entries, and the replay of whole
training runs through the CPU oracle with the scripted slots held to the specification."""
import math

import numpy as np
import torch

import update_check_util as U

KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset")


def check_gradient_slots(A, k, kl_coef, vf_clip, R=512, seed=6, chunks=4):
    """update_check_util.check_gradient for FusedUpdate(policy, R, rows, k) with rec_stride = 8 * A: the samples are slots 0 .. k - 1 of every row, the records of
    the slots behind them are NaN (a scripted slot's record is no policy sample).  The same stages and bands: (a) the loss gradient on the kernel's own outputs,
    (b) the weight gradient from the kernel's own images, (c) the backward pass alone and the whole gradient against float32 autograd, (d) loss statistics, norm,
    Adam; and everything the step wrote is finite."""
    from gym_continuousdoubleauction_amd import mlp
    prob = U.make_problem(A, None, kl_coef, R=R, seed=seed)
    prob["rec"][:, k:] = float("nan")
    prob["rec_ref"] = prob["rec"][:, :k].contiguous()            # what the references read: the trained slots' records
    prob["agents"] = k
    upd = U.make_update(prob, R, chunks=chunks, vf_clip=vf_clip)
    d = upd.dev
    assert bool(torch.isnan(d["rec"][:, k:]).all()) and upd.A == k
    upd.set_extra(rec_stride=8 * A, kl_coef=kl_coef, vf_clip=vf_clip, dist_old=d["dist"], log_std_old=d["ls"])
    chunks_, tiles = U.step(prob, upd, 0, R)
    for name, t in (("outputs", upd.out[:R]), ("d_out", upd.d_out[:R]), ("grad", upd.grad), ("out6", upd.out6), ("norm2", upd.norm2[2])):
        assert bool(torch.isfinite(t).all()), name
    _, off, n, terms = U.stage_loss_gradient(prob, upd, 0, R, vf_clip)
    assert n == R * k
    U.stage_weight_gradient(prob, upd, 0, R)
    cos, worst = U.stage_whole_gradient(prob, upd, 0, R, vf_clip)
    # check_gradient's own closing checks: the reported loss, value loss and KL against the float32 statement, and the clamp active on a real share
    p = prob["p"]
    pm = upd.perm.cpu()
    sel = prob["rec_ref"][pm]
    acts = (sel[..., 0].contiguous().view(torch.int32).long().reshape(-1), sel[..., 1].contiguous().view(torch.int32).long().reshape(-1),
            sel[..., 2].contiguous().view(torch.int32).long().reshape(-1), sel[..., 3:5].reshape(-1, 2))
    m = mlp.actor_critic_from_theta(p.theta).float()
    loss, pg, vl, kl = U._torch_objective(m, prob["x"][pm], acts, sel[..., 5].reshape(-1), sel[..., 6].reshape(-1), sel[..., 7].reshape(-1), prob["dist_old"][pm],
                                          prob["ls_old"], 0.3, 1.0, 0.01, kl_coef, vf_clip, k)
    out6 = upd.out6.cpu()
    assert abs(float(out6[3]) - float(loss.detach())) <= 2e-2 * abs(float(loss.detach())) + 1e-3
    assert abs(float(out6[1]) - float(vl.detach())) <= 2e-2 * float(vl.detach()) + 1e-4
    if kl_coef:
        assert float(kl.detach()) > 1e-4 and abs(float(out6[6]) - float(kl.detach())) <= 3e-2 * float(kl.detach()) + 1e-5
    else:
        assert float(out6[6]) == 0.0
    if vf_clip:
        frac = float(((m.evaluate(prob["x"][pm], acts, agents_per_row=k)[2] - sel[..., 7].reshape(-1)).pow(2) > vf_clip).float().mean())
        assert 0.2 < frac < 0.95, frac
    ratios = U.stage_rest(prob, upd, chunks_, tiles, terms)
    assert bool(torch.isfinite(p.theta).all())
    return cos, worst, ratios


def host_assignment(mapper, episode_ids, net_of):
    """(slot_net, slot_script, slot_pool) i32 [N, A] by the host rule: LeagueSlotMapper.assign (numpy), a champion's bank row from net_of, LEAGUE_RANDOM elsewhere,
    1 + the profile index where a scripted module was drawn"""
    a = mapper.assign(episode_ids)
    k, names = mapper.num_trainable, mapper.available_modules
    slot_net, slot_script, slot_pool = (np.zeros(a.shape, np.int32) for _ in range(3))
    for (i, s), idx in np.ndenumerate(a):
        if s < k:
            slot_net[i, s], slot_pool[i, s] = s, -1
            continue
        name = names[idx]
        slot_pool[i, s] = idx - k
        slot_net[i, s] = net_of.get(name, -1)
        slot_script[i, s] = 1 + mapper.scripted[name][0] if name in mapper.scripted else 0
    return slot_net, slot_script, slot_pool


def classes_drawn(mapper, episode_ids):
    """the pool classes (policy / scripted / champion) the host rule draws for these ids"""
    a = mapper.assign(episode_ids)[:, mapper.num_trainable:]
    return {mapper.available_modules[i].split("_")[0] for i in np.unique(a)}


def snapshot_rollout(roll, slots=None):
    """a host copy of what a replay needs of the rollout that just ran: the buffers, the rollout counter its draws were keyed with, the scripted slot table"""
    torch.cuda.synchronize()
    b = {key: roll.buf[key].cpu().numpy().copy() for key in KEYS + ("obs", "reward", "terminated", "truncated", "logp", "a_cont")}
    env = roll.env
    table = env.scripted_slot_tensor().cpu().numpy().copy() if slots is None else np.asarray(slots)
    return {"b": b, "counter": int(roll.counter.item()), "slots": table}


def replay_run(cfg, n, seed, rollouts, profiles, script_seed, base=0, check_scripts=(), tick=1):
    """every rollout of a run, in order, through the CPU oracle from the run's reset: observations, rewards and episode ends bit for bit (the oracle resets where
    the env reset itself).  check_scripts: indices of the rollouts in which, at every step, the scripted slots' recorded actions must be scripted.py's specification
    on the ORACLE's books and accounts (and carry logp = a_cont = 0).  Returns the set of categories the checked scripted slots played."""
    import oracle_lib as O
    from gym_continuousdoubleauction_amd import scripted as S
    from test_scripted_host import views_of_books
    a = cfg["num_of_agents"]
    ora = O.OracleEnv({key: v for key, v in cfg.items() if key != "auto_reset"}, n_markets=n)
    o = ora.reset(seeds=(seed + np.arange(n)).astype(np.uint64))
    m, j = np.meshgrid(np.arange(n), np.arange(a), indexing="ij")
    acted = set()
    for r, ro in enumerate(rollouts):
        b, slots = ro["b"], ro["slots"]
        T = b["category"].shape[0]
        assert np.array_equal(b["obs"][0].view(np.uint32), o.view(np.uint32)), ("first observation of rollout", r)
        scripted, pix = slots != 0, np.maximum(slots - 1, 0)
        depth = np.array([p.depth_levels for p in profiles])[pix]
        for t in range(T):
            if r in check_scripts:
                states = [ora.get_state(i) for i in range(n)]
                views = views_of_books([ora.get_book(i) for i in range(n)], a, [[int(s.acc[x].net_position) for x in range(a)] for s in states],
                                       [int(s.t_step) for s in states], tick, depth)
                want = S.actions_from_views(profiles, pix, views, script_seed, ro["counter"], base + m, t, j)
                for key, w in zip(KEYS, want):
                    assert np.array_equal(b[key][t][scripted].view(np.uint32), w[scripted].view(np.uint32)), (r, t, key)
                acted |= set(want[0][scripted].tolist())
                assert (b["logp"][t][scripted] == 0).all() and (b["a_cont"][t][scripted] == 0).all()
            oo, orw, ot, otr, _ = ora.step(*(b[key][t] for key in KEYS))
            assert np.array_equal(b["reward"][t].view(np.uint64), orw.view(np.uint64)), (r, t)
            assert np.array_equal(b["terminated"][t], ot) and np.array_equal(b["truncated"][t], otr), (r, t)
            done = (ot | otr).astype(bool)
            if done.any():
                oo = ora.reset(mask=done.astype(np.uint8)).copy()
            assert np.array_equal(b["obs"][t + 1].view(np.uint32), oo.view(np.uint32)), (r, t)
            o = oo
    ora.close()
    return acted


def finite(stats):
    return all(math.isfinite(v) for v in stats.values() if isinstance(v, float))
