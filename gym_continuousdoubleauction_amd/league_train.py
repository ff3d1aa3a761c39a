"""League self-play on the batched env (SURVEY §8(f)-1 + 3 together): the trainable slots learn with PPO against a pool of
fixed random opponents and frozen champion snapshots, assigned per episode by the reference's mapping rule.

Two loops:
  * `train_league_fused` - the reference's training topology (train/train.py:466-503: `num_trained_agents` SEPARATELY trained policies, policy_p plays slot p; every
    other slot drawn per episode from uniform random modules and champions, callbk/league_based_self_play_callback.py:1286-1344; promotion by the reference's
    rule, :780-880) on the hand-written network kernels (include/cda_mlp.h `cda_league`): one policy launch per step for every module of every market, rollouts
    replayed from HIP graphs, each policy's update reading its own slot's records in place.  This is the one `bench.py` and `profiles/r05/bench_league.json` measure.
  * `train_league` - the same idea on the float32 torch network (ppo.ActorCritic), one shared learning policy, step by step from the host: the statement the
    fused loop's tests compare against, 30-50 x slower.  What it keeps of the reference:
      - slots below `num_trainable` are played by the learning policy, every other slot by a module drawn from the pool
        (`LeagueSlotMapper`, weights original_opponent_weight / champion_weight, keyed by the episode id);
      - only the trainable slots' transitions feed the PPO update;
      - a champion is a frozen copy of the learning policy, added to the pool when the iteration's mean return of the trainable slots beats the
        best so far by `promote_margin` (a plain statement of the idea; the reference's trigger is `League.maybe_promote` below);
      - one iteration = one whole episode of every market (`horizon == max_step`).

    python -m gym_continuousdoubleauction_amd.league_train --fused --markets 2048 --agents 8 --episode 64 --iters 10
    python -m gym_continuousdoubleauction_amd.league_train --markets 1024 --agents 4 --iters 6
"""
import argparse
import contextlib
import copy
import json
import os
import shutil
import time

import numpy as np
import torch

from . import ppo
from .league import LeagueSlotMapper, RandomModule


class _FrozenPolicy:
    """A champion snapshot: acts like the policy it was copied from, without gradients."""

    def __init__(self, model):
        self.model = copy.deepcopy(model).eval()
        for p in self.model.parameters():
            p.requires_grad_(False)

    @torch.no_grad()
    def __call__(self, obs):
        actions, _, _ = self.model.act(obs)
        return tuple(x.reshape(-1) for x in ppo.to_env_actions(actions, obs.shape[0], 1))


def train_league(env, iters=4, num_trainable=1, lr=5e-5, epochs=4, reward_scale=1e-3, seed=0, original_opponent_weight=1.0,
                 champion_weight=3.0, promote_margin=0.0, max_champions=8, recorder=None, log=print):
    """env: CDAVecEnv-shaped, its max_step is the episode length.  Returns (model, mapper, history).
    recorder: an `episode_record.BatchedEpisodeRecorder` (env built with_info=True): the episodes of its markets are written
    in the reference's Parquet schema, `module_id` = the module that played each slot."""
    torch.manual_seed(seed)
    dev = env.obs.device
    N, A, T = env.n_markets, env.num_agents, int(env.max_step)
    k = int(num_trainable)
    model = ppo.ActorCritic(env.obs_dim).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr, fused=dev.type == "cuda")
    mapper = LeagueSlotMapper(A, k, A - k, original_opponent_weight, champion_weight)
    modules = {name: RandomModule(dev, seed=1000 + i) for i, name in enumerate(mapper.available_modules[k:])}
    best, history = None, []
    for it in range(iters):
        t0 = time.perf_counter()
        env.reset(seed=seed + it * N)                                   # a fresh episode for every market
        assignment = mapper.assign([f"iter{it}-market{i}" for i in range(N)])
        groups = {name: (torch.as_tensor(mk, device=dev), torch.as_tensor(sl, device=dev))
                  for name, (mk, sl) in mapper.group_by_module(assignment).items() if name in modules}
        if recorder is not None:
            recorder.iteration = it
            names = mapper.names(assignment)
            recorder.begin_episodes([f"iter{it}-market{int(i)}" for i in recorder.markets], module_ids=[list(names[int(i)]) for i in recorder.markets])
        buf_obs, buf_act, buf_logp, buf_val, buf_rew = [], [], [], [], []
        acts = [torch.zeros((N, A), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.float32, torch.int32, torch.int32)]
        for _ in range(T):
            obs = env.obs
            pobs = obs.repeat_interleave(k, dim=0)                       # the k trainable slots of each market
            with torch.no_grad():
                a_tr, logp, val = model.act(pobs)
            for dst, src in zip(acts, ppo.to_env_actions(a_tr, N, k)):
                dst[:, :k] = src
            for name, (mk, sl) in groups.items():                        # one batched forward per opponent module
                for dst, src in zip(acts, modules[name](obs.index_select(0, mk))):
                    dst[mk, sl] = src.to(dst.dtype)
            o_next, r, _, _, info = env.step(*acts)
            if recorder is not None:
                recorder.record_step(o_next, r, info, acts)
            buf_obs.append(pobs); buf_act.append(a_tr); buf_logp.append(logp); buf_val.append(val)
            buf_rew.append((r[:, :k].float() * reward_scale).reshape(-1))
        if recorder is not None:
            recorder.finish(complete=True)
        rew, val = torch.stack(buf_rew), torch.stack(buf_val)
        done = torch.zeros_like(rew)
        done[-1] = 1.0                                                   # the episode ends with the rollout
        adv, ret = ppo.gae(rew, val, torch.zeros_like(val[0]), done)
        flat = lambda xs: torch.cat(xs, 0)                               # noqa: E731
        a_all = tuple(flat([b[i] for b in buf_act]) for i in range(4))
        stats = ppo.ppo_update(model, opt, flat(buf_obs), a_all, flat(buf_logp), adv.reshape(-1), ret.reshape(-1), epochs=epochs,
                               minibatch=min(65536, N * k * T))
        episode_return = float(rew.sum(0).mean()) / reward_scale
        promoted = None
        if (best is None or episode_return > best + promote_margin) and sum(n.startswith("champion_") for n in mapper.available_modules) < max_champions:
            best = episode_return if best is None else max(best, episode_return)
            promoted = mapper.add_champion()
            modules[promoted] = _FrozenPolicy(model)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        stats.update(iter=it, episode_return=episode_return, promoted=promoted, pool=list(mapper.pool()),
                     agent_steps_per_s=N * A * T / (time.perf_counter() - t0))
        history.append(stats)
        log(json.dumps(stats))
    return model, mapper, history


class League:
    """The league's host state next to the device banks: who is in the pool, which bank row holds which champion, when the last one was promoted - the reference's
    trigger (train/callbk/league_based_self_play_callback.py:780-880): a trainable policy becomes a champion when its mean episode return of the iteration exceeds
    mean + std_dev_multiplier x std of all modules' returns, at most every `min_iterations_between_champions` iterations, the oldest champion leaving once
    `max_champions` are held (config/train_config.json:60-64)."""

    def __init__(self, mapper, bank, std_dev_multiplier=0.1, max_champions=8, min_iterations_between_champions=2):
        self.mapper, self.bank = mapper, bank
        self.std_dev_multiplier, self.max_champions, self.min_gap = float(std_dev_multiplier), int(max_champions), int(min_iterations_between_champions)
        self.net_of = {}                                       # champion id -> bank row
        self.history = []                                      # [{"id", "iteration", "return", "source"}]

    def module_returns(self, per_slot, slot_pool, allreduce=None):
        """{module id: mean return of the episodes it completed this iteration}: per_slot f64 [N, A, 2] (mlp.EpisodeReturns), slot_pool i32 [N, A] (the draw per slot,
        -1 = the slot's own trainable policy).  A handful of tiny device reductions + one small copy to the host."""
        k, names = self.mapper.num_trainable, self.mapper.available_modules
        N, A = slot_pool.shape
        idx = torch.where(slot_pool < 0, torch.arange(A, device=slot_pool.device, dtype=torch.int32).expand(N, A), slot_pool + k).long().reshape(-1)
        # (masked sums - not index_add_: a dozen bins under 16 k double-precision atomics took 1.6 ms per call, a fifth of an iteration; not a one-hot matrix product
        # either: a float64 GEMM with two columns is 1.9 ms in the library)
        mask = idx[None, :] == torch.arange(len(names), device=idx.device)[:, None]                    # [modules, N * A]
        flat = per_slot.reshape(-1, 2)
        zero = torch.zeros((), dtype=torch.float64, device=flat.device)
        sums = torch.stack([torch.where(mask, flat[:, 0][None, :], zero).sum(1), torch.where(mask, flat[:, 1][None, :], zero).sum(1)], dim=1)
        if allreduce is not None:                              # data parallel: the modules' returns over ALL shards (every rank then takes the same decision)
            allreduce(sums)
        host = sums.cpu().numpy()
        return {names[i]: host[i, 0] / host[i, 1] for i in range(len(names)) if host[i, 1] > 0}

    def maybe_promote(self, returns, iteration):
        """the reference's end-of-iteration decision; returns the new champion's id or None"""
        k = self.mapper.num_trainable
        valid = [v for v in returns.values() if np.isfinite(v)]
        if not valid:
            return None
        threshold = float(np.mean(valid)) + self.std_dev_multiplier * float(np.std(valid))
        best, best_ret = None, -float("inf")
        for p in range(k):
            r = returns.get(self.mapper.available_modules[p])
            if r is not None and r > best_ret:
                best, best_ret = p, r
        if best is None or not best_ret > threshold:
            return None
        if self.history and iteration - self.history[-1]["iteration"] < self.min_gap:
            return None
        slot = None
        if len(self.net_of) >= self.max_champions:            # rolling window: the oldest champion leaves and its bank row is reused
            oldest = next(c["id"] for c in self.history if c["id"] in self.net_of)
            slot = self.net_of.pop(oldest) - k
            self.mapper.remove(oldest)
        cid = self.mapper.add_champion()
        self.net_of[cid] = self.bank.snapshot(best, frozen_slot=slot)
        self.history.append({"id": cid, "iteration": iteration, "return": best_ret, "source": self.mapper.available_modules[best]})
        return cid


def train_league_fused(env, iters=4, horizon=None, num_trainable=2, lr=5e-5, epochs=4, seed=0, original_opponent_weight=1.0, champion_weight=3.0,
                       std_dev_multiplier=0.1, max_champions=8, min_iterations_between_champions=2, chains=4, minibatch=262144, objective=None, use_graph=True,
                       recorder=None, info_markets=0, run_id="league", log=print, keep=None, allreduce=None, world=1, first_market=0, episode_metrics=True,
                       strict_nav_check=True, state_dependent_log_std=False, hidden=(256, 256),
                       checkpoint_dir=None, chkpt_freq=0, chkpt_keep=3, restore=None, iters_is_delta=False, activation="tanh", vf_share_layers=False,
                       scripted_opponents=None, scripted_weight=1.0, random_opponents=None):
    """League self-play on the fused kernels (include/cda_mlp.h `cda_league`): the reference's training topology - `num_trainable` SEPARATELY trained policies
    (policy_p plays slot p), every other slot drawn per episode from the pool of uniform random modules and frozen champions by the reference's mapping rule
    (computed on the device, league.LeagueSlotMapper.assign_device) - at the speed of the fused loop: ONE policy launch per step serves every module of every
    market, the rollout never leaves its HIP graphs, each trainable policy's update reads its own slot's sample records in place (record stride, no compaction).
    env: CDAVecEnv with auto_reset; an episode = env.max_step steps = max_step / horizon iterations (horizon must divide it): all markets change opponents
    together at the episode boundary.  Returns (bank, league, history).
    episode_metrics (default on): every episode end is checked and tallied on the device (ppo.train_fused), here PER MODULE - keyed by the draw of the mapping fn, so
    a champion's or a random module's figures are its own whatever slot it played (the reference's `module_episode_returns_mean` keying, callbk:780-800);
    history[i]["episode_metrics"] = {"episodes", "nav_conservation_violations", ..., "modules": {module id: {...}}}; a violation raises (strict_nav_check).
    allreduce / world / first_market: the data-parallel learner of ppo.train_fused for the league - every rank rolls out and back-propagates its own shard of
    markets (global indices [first_market, first_market + N): env seeds, sampling keys and EPISODE IDS follow them, so the opponents a market meets do not depend
    on the GPU count), the ranks sum each policy's gradient (one all-reduce of 0.9 MB per policy and minibatch step) and advantage sums, and the per-module returns
    behind the promotion rule - so every rank promotes the same champions in lockstep - and merge their episode-metric tables by the device's rule
    (episode_metrics.allreduce_tables: MIN / MAX / SUM by column; the callable must take op=), so every rank logs and checks the global figures.
    checkpoint_dir / chkpt_freq / chkpt_keep / restore / iters_is_delta (all off by default): a resumable run, as in ppo.train_fused (checkpoint.py).  A league
    checkpoint is taken only at an EPISODE BOUNDARY ((it + 1) % per_episode == 0, where no opponent window is open): chkpt_freq must be a multiple of
    max_step / horizon (ValueError otherwise), and the final save is skipped when the run does not end on a boundary.  It holds the env snapshot, every
    trainable net (theta + Adam), every bank row as save_league's policy files (league/ in the checkpoint) plus the bank's packed weights, the League and mapper
    state (champions and their rows, promotion history, champion id counter, pool), the rollout counters, the updates' shuffle state, the KL coefficients and
    the running episode returns: the mapping, episode ids and promotions continue exactly.  Single-process runs only; no recorder.
    activation: `fcnet_activation` of the whole bank (mlp.PolicyBank: trainable policies and their champion snapshots share it); vf_share_layers likewise (RLlib's
    shared trunk for every net of the bank).
    scripted_opponents / scripted_weight / random_opponents: scripted modules (scripted.parse_profile's forms: rule-based agents on the device) in the per-episode
    opponent pool, as modules scripted_<i>_<law> behind the fixed opponents, weighted scripted_weight (1.0 = the reference rule's "otherwise"); random_opponents =
    the number of uniform random modules in the pool (default A - num_trainable; 0: a pool of scripted modules and champions only).  The profiles are attached to the
    env once, with an all-zero slot table, before the rollout graphs are captured; at every episode boundary the assignment launch (cda_league_assign_scripted)
    rewrites the env's resident slot table beside bank.slot_net - no re-attach, no re-capture - and they are detached on exit, also on an exception (scripted.attached).  Module returns,
    per-module episode metrics, the recorder and league.json name them; promotion considers trainable policies only.  A checkpoint's args hold their canonical
    fields and the weight.  Single-process runs only (ValueError with world > 1); an env that has scripts attached already is refused."""
    if getattr(env, "label_tap", None) is not None:                  # (an action the label tap mixed in is no policy sample)
        raise ValueError("train_league_fused does not take an env with a label tap attached: an action the tap mixed in is not a sample of a policy (clear_label_tap() first)")
    if getattr(env, "scripted", False):                              # (a scripted slot's sample record is no policy sample: it must not reach a loss)
        raise ValueError("train_league_fused does not take an env with scripted opponents attached: pass them as scripted_opponents=[...] (the league attaches its pool's "
                         "profiles itself) after clear_scripted()")
    from .ppo import _refuse_stateful
    _refuse_stateful(env, scripted_opponents, "train_league_fused(scripted_opponents=...)")
    attach, profiles = contextlib.nullcontext(), []
    if scripted_opponents is not None:
        from . import scripted as SC
        profiles = [SC.parse_profile(o) for o in scripted_opponents]
        if not profiles:
            raise ValueError("scripted_opponents: None or a non-empty list of scripted opponents")
        if len(profiles) > SC.MAX_PROFILES:
            raise ValueError(f"at most {SC.MAX_PROFILES} scripted opponents, got {len(profiles)}")
        if int(world) > 1 or allreduce is not None:
            raise ValueError("scripted opponents in the league's pool: single-process runs only - data-parallel runs (world > 1) with scripts are out of scope")
        if not 1 <= int(num_trainable) <= env.num_agents - 1:
            raise ValueError(f"num_trainable must lie in 1 .. num_agents - 1 = {env.num_agents - 1} for a pool to be drawn from")
        # all-zero table: nobody is scripted until the first assignment writes the draws; the script epoch (and the graphs captured on it) then hold for the whole run
        attach = SC.attached(env, np.zeros((env.n_markets, env.num_agents), np.int32), profiles, seed=seed, market_index_base=int(first_market))
    with attach:
        return _train_league_fused(env, profiles, ppo.merged_objective(objective), iters=iters, horizon=horizon, num_trainable=num_trainable, lr=lr, epochs=epochs, seed=seed,
                                   original_opponent_weight=original_opponent_weight, champion_weight=champion_weight, std_dev_multiplier=std_dev_multiplier, max_champions=max_champions,
                                   min_iterations_between_champions=min_iterations_between_champions, chains=chains, minibatch=minibatch, use_graph=use_graph, recorder=recorder,
                                   info_markets=info_markets, run_id=run_id, log=log, keep=keep, allreduce=allreduce, world=world, first_market=first_market, episode_metrics=episode_metrics,
                                   strict_nav_check=strict_nav_check, state_dependent_log_std=state_dependent_log_std, hidden=hidden, activation=activation, vf_share_layers=vf_share_layers,
                                   scripted_weight=scripted_weight, random_opponents=random_opponents, ck=dict(checkpoint_dir=checkpoint_dir, chkpt_freq=chkpt_freq, chkpt_keep=chkpt_keep, restore=restore, iters_is_delta=iters_is_delta))


def _train_league_fused(env, profiles, obj, *, iters, horizon, num_trainable, lr, epochs, seed, original_opponent_weight, champion_weight, std_dev_multiplier, max_champions,
                        min_iterations_between_champions, chains, minibatch, use_graph, recorder, info_markets, run_id, log, keep, allreduce, world, first_market,
                        episode_metrics, strict_nav_check, state_dependent_log_std, hidden, activation, vf_share_layers, scripted_weight, random_opponents, ck):
    """train_league_fused's loop.  profiles: the pool's scripted modules, attached to the env ([]: none); obj: the merged objective; ck: checkpoint.Run's keywords"""
    from . import checkpoint as CK, episode_metrics as EM
    from .mlp import EpisodeReturns, FusedUpdate, PolicyBank, RolloutChains
    dev = env.obs.device
    N, A, k = env.n_markets, env.num_agents, int(num_trainable)
    T = int(horizon or env.max_step)
    if int(env.max_step) % T:
        raise ValueError("the horizon must divide the episode length (max_step)")
    per_episode = int(env.max_step) // T
    run = CK.Run("league", iters=iters, world=world, allreduce=allreduce, recorder=recorder, run_id=run_id, **ck)
    if run.resumable and run.chkpt_freq % per_episode:
        raise ValueError(f"league checkpoints are taken at episode boundaries only: chkpt_freq ({run.chkpt_freq}) must be a multiple of max_step / horizon = {per_episode}")
    bank = PolicyBank(dev, N, A, k, max_frozen=max_champions, seed=seed, random_seed=seed + 12345 + 104729 * int(first_market), n_hist=env.n_hist, state_dependent_log_std=state_dependent_log_std, hidden=hidden,
                      activation=activation, vf_share_layers=vf_share_layers)
    n_random = A - k if random_opponents is None else int(random_opponents)
    if n_random < 0:
        raise ValueError("random_opponents must be >= 0")
    mapper = LeagueSlotMapper(A, k, n_random, original_opponent_weight, champion_weight, scripted_weight=scripted_weight)
    for prof in profiles:
        mapper.add_scripted(prof)
    league = League(mapper, bank, std_dev_multiplier, max_champions, min_iterations_between_champions)
    slot_script = env.scripted_slot_tensor() if profiles else None
    if run.resumable:
        args = dict(CK.run_args(bank.policies[0], env, T, chains, obj, epochs, lr, minibatch, seed, episode_metrics), max_step=int(env.max_step), trainable=int(k),
                    max_champions=int(max_champions), std_dev_multiplier=float(std_dev_multiplier), min_iterations_between_champions=int(min_iterations_between_champions),
                    original_opponent_weight=float(original_opponent_weight), champion_weight=float(champion_weight), run_id=str(run_id))
        args = CK.with_order_schedule(CK.with_scripted(args, profiles, scripted_weight=scripted_weight), env.order_schedule_digest())
        run.open(args if random_opponents is None else dict(args, random_opponents=n_random))     # (the key only when the argument is given: checkpoints from before it existed resume)
    if allreduce is not None and world > 1 and episode_metrics:          # (before anything runs: the tables' MIN / MAX columns need op= on the collective)
        EM.check_allreduce(allreduce)
    run.start_env(env, seed, first_market, episode_metrics)
    if run.state is not None:
        _load_league_state(os.path.join(run.path, "league"), run.state, bank, league)
    module_of, module_names = torch.zeros((N, A), dtype=torch.int32, device=dev), list(mapper.available_modules)
    use_kl = obj["kl_coef"] > 0.0
    roll = RolloutChains(env, bank, T, groups=chains, seed=seed + 7919 * int(first_market), use_graphs=use_graph, with_dist=use_kl,
                         capture_ends=bool(obj["bootstrap_truncation"]), info_markets=info_markets if recorder is not None else 0)
    if keep is not None:
        keep.update(rollout=roll)                           # (from the start: a `log` callback can read each iteration's buffers through it)
    R = T * N
    rows_mb = max(32, min(R, (max(1, minibatch) // 32) * 32))              # one sample per row: a minibatch of `minibatch` samples is that many rows
    dp = allreduce is not None and world > 1
    upds = [FusedUpdate(bank.policies[p], R, rows_mb, 1, allreduce=allreduce if dp else None, world=world if dp else 1) for p in range(k)]
    # the trainable policies' updates are independent of each other: on their own streams one's kernel tails fill with the other's launches (CDA_LEAGUE_UPDATE_STREAMS=0: one stream)
    update_streams = list(roll.streams[:k]) if (k > 1 and len(roll.streams) >= 2 and not dp and os.environ.get("CDA_LEAGUE_UPDATE_STREAMS", "1") != "0") else []
    # (data parallel: one stream - the ranks must issue their collectives in ONE order)
    returns = EpisodeReturns(N, A, dev, per_slot=True)
    # Opponents change for ALL markets at the `it % per_episode == 0` boundary (lock-step by construction: a market that terminates early - every agent done - auto-resets
    # and plays its next episode against the SAME draw until the boundary; its early end is credited to that draw).  EpisodeReturns.per_slot holds one rollout's completed
    # episodes, so over a window of several rollouts they are summed here.
    window_per_slot = torch.zeros_like(returns.per_slot) if per_episode > 1 else None
    slot_pool = torch.full((N, A), -1, dtype=torch.int32, device=dev)
    kl_coefs = [float(obj["kl_coef"])] * k
    episode_ids = lambda e: [f"{run_id}-episode{e}-market{int(first_market) + i}" for i in range(N)]     # noqa: E731  (global market index)
    next_crcs = mapper.episode_crcs(episode_ids(0))
    if recorder is not None:
        names = lambda: np.array(mapper.available_modules, dtype=object)             # noqa: E731
        recorder.episode_namer = lambda m, e: f"{run_id}-episode{e}-market{m}"
        recorder.init_cash = env.market_rows(0, N)["init_cash"].astype("int64") if getattr(env, "per_market", False) else int(env.config.get("init_cash", 1000000))
    history = []
    if run.state is not None:
        CK.load_rollout_record(roll, run.state["rollout"])
        for p in range(k):
            CK.load_update_record(upds[p], run.state["updates"][p])
        CK.load_returns_record(returns, run.state["returns"])
        kl_coefs = [float(x) for x in run.state["kl_coefs"]]
        next_crcs = mapper.episode_crcs(episode_ids(int(run.state["iteration"]) // per_episode))

    def save(n_done):
        tmp = os.path.join(run.checkpoint_dir, CK.checkpoint_name(n_done) + ".league")
        shutil.rmtree(tmp, ignore_errors=True)
        save_league(tmp, bank, league)                          # the bank rows as policy files
        state = {"nets": [CK.net_record(pol) for pol in bank.policies], "wb": bank.wb.detach().cpu().clone(), "n_frozen": int(bank.n_frozen),
                 "league": _league_record(league), "rollout": CK.rollout_record(roll), "updates": [CK.update_record(u) for u in upds],
                 "returns": CK.returns_record(returns), "kl_coefs": [float(x) for x in kl_coefs]}
        return run.save(n_done, state, env, extra_dirs={"league": tmp})
    for it in run.its:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if it % per_episode == 0:                                            # a new episode everywhere: new opponents (one launch; the crcs were computed while the GPU worked)
            mapper.assign_device(bank, crcs=next_crcs, net_of=league.net_of, slot_pool=slot_pool, slot_script=slot_script)
            if episode_metrics:                                              # who plays what during the coming episodes: index into the pool AS IT STANDS NOW
                torch.where(slot_pool < 0, torch.arange(A, device=dev, dtype=torch.int32).expand(N, A), slot_pool + k, out=module_of)
                module_names = list(mapper.available_modules)
            if recorder is not None:
                sp = slot_pool[N - roll.info_markets:].cpu().numpy() if roll.info_markets else None
                mods = names()
                recorder.module_namer = lambda m: [mods[a] if sp[m - (N - roll.info_markets), a] < 0 else mods[k + sp[m - (N - roll.info_markets), a]] for a in range(A)]
                if hasattr(recorder, "_ordinal"):
                    recorder._name_episodes()
        buf = roll.run()
        rec, stats, count = roll.gae(gamma=obj["gamma"], lam=obj["lam"], reward_scale=obj["reward_scale"])
        if dp:                                                               # the advantages are standardised over the GLOBAL batch of each policy
            allreduce(stats)
            count = count * world
        torch.cuda.synchronize(dev)
        t_roll = time.perf_counter()
        obs_rows = buf["obs"][:T].view(R, -1)
        outs = []
        cur = torch.cuda.current_stream(dev)
        if update_streams:
            fork = torch.cuda.Event(); fork.record(cur)
        for p in range(k):                                                   # policy p learns from slot p's records only: rec + 8 p floats, a row every 8 A
            upds[p].set_extra(rec_stride=8 * A, kl_coef=kl_coefs[p], vf_clip=obj["vf_clip"], dist_old=buf["dist"][p] if use_kl else None,
                              log_std_old=roll.log_std_old[p] if use_kl else None)
            st = update_streams[p % len(update_streams)] if update_streams else cur
            if update_streams:
                st.wait_event(fork)
            with torch.cuda.stream(st):                                      # (the policies' updates are independent chains of launches)
                outs.append(upds[p].run(obs_rows, epochs=epochs, clip=obj["clip"], vf_coef=obj["vf_coef"], ent_coef=obj["ent_coef"], lr=lr, max_norm=obj["max_norm"],
                                        records=(rec.data_ptr() + 32 * p, stats[p], count)))
            if update_streams:
                ev = torch.cuda.Event(); ev.record(st); cur.wait_event(ev)
        returns.update(buf, T)
        if window_per_slot is not None:                                      # an episode window of several rollouts: an early end in an EARLIER rollout of the window counts too
            window_per_slot.add_(returns.per_slot)
        em = env.collect_episode_metrics(module_of=module_of, n_modules=len(module_names)) if episode_metrics else None     # (before the pool changes)
        if (it + 1) % per_episode == 0:                                      # host work under the GPU's: the next episode's ids
            next_crcs = mapper.episode_crcs(episode_ids((it + 1) // per_episode))
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        stats_h = {"iter": it, "agent_steps": N * A * T, "agent_steps_per_s": N * A * T / (t1 - t0), "rollout_s": t_roll - t0, "update_s": t1 - t_roll}
        for p, o in enumerate(outs):
            stats_h[f"policy_{p}"] = {key: float(v) for key, v in o.items()}
            kl_coefs[p] = ppo.adapt_kl_coef(kl_coefs[p], stats_h[f"policy_{p}"]["kl"], obj["kl_target"])
        promoted = None
        if (it + 1) % per_episode == 0:                                      # episodes just ended: credit the modules, run the reference's promotion rule
            mr = league.module_returns(returns.per_slot if window_per_slot is None else window_per_slot, slot_pool, allreduce=allreduce if dp else None)
            if window_per_slot is not None:
                window_per_slot.zero_()
            promoted = league.maybe_promote(mr, it)
            stats_h["module_returns"] = {m: float(v) for m, v in mr.items()}
        stats_h.update(promoted=promoted, pool=list(mapper.pool()), mean_reward_trainable=float(buf["reward"][:, :, :k].mean()))
        roll.check_capture_overflow()                                       # (outside the timed region; warns)
        if recorder is not None and roll.info is not None:
            recorder.record_rollout(roll, iteration=it)
        EM.log_iteration(it, stats_h, em, module_names, history, log, strict=strict_nav_check, allreduce=allreduce if dp else None)     # (the whole summary, per module)
        run.after_iteration(it, save, may_save=lambda n_done: n_done % per_episode == 0)     # (episode boundaries only: chkpt_freq is a multiple of per_episode)
    if keep is not None:
        keep.update(buffers=roll.buf, rollout=roll, updates=upds, slot_pool=slot_pool, returns=returns)
        if slot_script is not None:
            keep.update(slot_script=slot_script.clone())                 # (the resident table goes with the detach)
    return bank, league, history


def _league_record(league):
    """League + mapper host state: champions and their bank rows, promotion history, champion id counter, the pool in its order"""
    m = league.mapper
    return {"net_of": {str(c): int(r) for c, r in league.net_of.items()}, "history": [dict(c, **{"return": float(c["return"]), "iteration": int(c["iteration"])})
                                                                                      for c in league.history],
            "available_modules": [str(x) for x in m.available_modules], "champion_id_counter": int(m.champion_id_counter)}


def _load_league_state(league_dir, state, bank, league):
    """a league checkpoint back into fresh bank / League objects: trainable nets (theta + Adam), champion rows from save_league's policy files, the bank's
    packed weights, the League and mapper state"""
    from . import checkpoint as CK
    from .mlp import read_policy
    for pol, rec in zip(bank.policies, state["nets"]):
        CK.load_net_record(pol, rec)
    with open(os.path.join(league_dir, "league.json")) as fh:
        lj = json.load(fh)
    for entry in lj["trainable"] + lj["champions"]:
        theta, act, vfs = read_policy(os.path.join(league_dir, entry["file"]), with_activation=True, with_vf_share_layers=True)
        row = int(entry["row"])
        if act != bank.activation:
            raise ValueError(f"{entry['file']}: a {act} network, the bank's are {bank.activation}")
        if vfs != bank.vf_share_layers:
            raise ValueError(f"{entry['file']}: vf_share_layers = {vfs}, the bank's networks have {bank.vf_share_layers}")
        if theta.numel() != bank.theta.shape[1]:
            raise ValueError(f"{entry['file']}: {theta.numel()} parameters, the bank rows hold {bank.theta.shape[1]}")
        bank.theta[row].copy_(theta)
    if tuple(state["wb"].shape) != tuple(bank.wb.shape):
        raise ValueError(f"checkpoint bank weights have shape {tuple(state['wb'].shape)}, this bank {tuple(bank.wb.shape)}")
    bank.wb.copy_(state["wb"])
    bank.n_frozen = int(state["n_frozen"])
    bank._refresh()
    lr = state["league"]
    league.net_of = {str(c): int(r) for c, r in lr["net_of"].items()}
    league.history = [dict(c) for c in lr["history"]]
    league.mapper.available_modules = list(lr["available_modules"])
    league.mapper.champion_id_counter = int(lr["champion_id_counter"])


def save_league(directory, bank, league):
    """write every trainable policy (policy_<p>.pt, bank row p) and every champion snapshot held in the bank (champion_<id>.pt) as policy files
    (mlp.save_policy's format) and a league.json naming them: module id, bank row, file, and for champions the promotion iteration / return / source.
    Returns the league.json dict."""
    from .mlp import policy_record
    act = getattr(bank, "activation", "tanh")                   # (the bank's one activation: every file carries it, tanh files no key)
    vfs = bool(getattr(bank, "vf_share_layers", False))         # (likewise the bank's one vf_share_layers: only shared-trunk files carry the key)
    os.makedirs(directory, exist_ok=True)
    promoted = {c["id"]: c for c in league.history}
    out = {"format": "cda-league", "version": 1, "trainable": [], "champions": []}
    scripted_mods = getattr(getattr(league, "mapper", None), "scripted", {})
    if scripted_mods:                                           # the rule-based modules of the pool: no file, their profile's canonical fields (scripted.profile_record)
        from .scripted import profile_record
        out["scripted"] = [{"module": str(mid), "index": int(i), "profile": profile_record(prof)} for mid, (i, prof) in sorted(scripted_mods.items(), key=lambda kv: kv[1][0])]
        out["scripted_weight"] = float(league.mapper.scripted_weight)
    for p in range(bank.n_trainable):
        fname = f"policy_{p}.pt"
        torch.save(policy_record(bank.theta[p], activation=act, vf_share_layers=vfs), os.path.join(directory, fname))
        out["trainable"].append({"module": f"policy_{p}", "row": p, "file": fname})
    for cid, row in sorted(league.net_of.items(), key=lambda kv: kv[1]):
        fname = "champion_" + "".join(ch if ch.isalnum() or ch in "-_" else "_" for ch in str(cid)) + ".pt"
        torch.save(policy_record(bank.theta[row], activation=act, vf_share_layers=vfs), os.path.join(directory, fname))
        c = promoted.get(cid, {})
        out["champions"].append({"module": str(cid), "row": int(row), "file": fname, "promoted_iteration": c.get("iteration"),
                                 "return": None if c.get("return") is None else float(c["return"]), "source": None if c.get("source") is None else str(c["source"])})
    with open(os.path.join(directory, "league.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    return out


def main(argv=None, parse_only=False):
    """parse_only: return the parsed arguments without touching a device (the flags' tests)"""
    p = argparse.ArgumentParser(description="League self-play (PPO vs random opponents and champion snapshots) on one MI355X.")
    p.add_argument("--markets", type=int, default=1024)
    p.add_argument("--agents", type=int, default=4)
    p.add_argument("--episode", type=int, default=64, help="episode length = max_step")
    p.add_argument("--iters", type=int, default=6)
    p.add_argument("--fused", action="store_true", help="the league on the hand-written network kernels (train_league_fused): the reference's topology at the fused loop's speed")
    p.add_argument("--trainable", type=int, default=None, help="separately trained policies (default: 2 with --fused, the reference's num_trained_agents; 1 otherwise)")
    p.add_argument("--horizon", type=int, default=None, help="--fused: rollout length (divides --episode; default = --episode)")
    p.add_argument("--save-dir", default=None, help="--fused: write the trainable policies, the champion snapshots and league.json here (save_league)")
    ppo.add_shared_flags(p, cap="--episode")                   # the network, the objective, resumable runs and --market-configs
    p.add_argument("--scripted-opponent", action="append", default=None, metavar="SPEC",
                   help="--fused: a scripted module ('pass', 'maker', 'taker', 'imbalance', 'NAME:key=value,...') in the per-episode opponent pool; repeat for several")
    p.add_argument("--scripted-weight", type=float, default=1.0, metavar="W", help="--fused: the pool weight of every scripted module (1.0 = the reference rule's \"otherwise\")")
    p.add_argument("--random-opponents", type=int, default=None, metavar="R", help="--fused: uniform random modules in the pool (default: agents - trainable; 0: scripted modules and champions only)")
    args = p.parse_args(argv)
    if not args.fused and (args.checkpoint_dir or args.restore):
        raise SystemExit("--checkpoint-dir / --restore need --fused")
    if not args.fused and (args.scripted_opponent or args.random_opponents is not None):
        raise SystemExit("--scripted-opponent / --random-opponents need --fused")
    if not args.fused and args.order_schedule:
        raise SystemExit("--order-schedule needs --fused")
    if parse_only:
        return args
    from .vec_env import CDAVecEnv
    from .market_params import load_market_configs, round_robin
    cfg = {"num_of_agents": args.agents, "init_cash": 1000000, "max_step": args.episode, "is_render": False}
    mcfg = round_robin(load_market_configs(args.market_configs), args.markets) if args.market_configs else None
    if not args.fused:
        env = CDAVecEnv(cfg, n_markets=args.markets, device="cuda:0", with_info=False, market_configs=mcfg)
        train_league(env, iters=args.iters, num_trainable=args.trainable or 1)
        env.close()
        return
    env = CDAVecEnv(dict(cfg, auto_reset=True), n_markets=args.markets, device="cuda:0", with_info=False, market_configs=mcfg)
    if args.order_schedule:
        env.load_order_schedule(args.order_schedule)
    k = args.trainable or 2
    bank, league, hist = train_league_fused(env, iters=args.iters, horizon=args.horizon, num_trainable=k, chains=args.chains,
                                         objective=ppo.RLLIB_DEFAULTS if args.objective == "rllib" else None, state_dependent_log_std=args.log_std_head, hidden=tuple(args.fcnet_hiddens),
                                         checkpoint_dir=args.checkpoint_dir, chkpt_freq=args.chkpt_freq, chkpt_keep=args.chkpt_keep, restore=args.restore,
                                         iters_is_delta=args.iters_is_delta, activation=args.fcnet_activation, vf_share_layers=args.vf_share_layers,
                                         scripted_opponents=args.scripted_opponent, scripted_weight=args.scripted_weight, random_opponents=args.random_opponents)
    summary = {"metric": "agent-steps/sec end to end (league rollout + one PPO update per trainable policy)",
               "config": {"workload": f"{args.markets} markets x {args.agents} agents, {k} separately trained policies (policy_p plays slot p) against modules drawn per episode "
                                      f"and slot from {args.agents - k} uniform random modules + up to 8 champion snapshots (the reference's mapping rule, on the device); episode "
                                      f"{args.episode} steps, horizon {args.horizon or args.episode}, {args.iters} iterations; hand-written bf16 MFMA network kernels, one policy launch per step "
                                      "for every module, 4 epochs per policy per iteration",
                          "markets": args.markets, "agents": args.agents, "trainable": k, "episode": args.episode, "horizon": args.horizon or args.episode, "chains": args.chains,
                          "objective": args.objective, "activation": args.fcnet_activation, "scripted_opponents": args.scripted_opponent, "order_schedule": args.order_schedule,
                          "scripted_weight": args.scripted_weight if args.scripted_opponent else None},
               "iterations": hist, "champions": league.history}
    if args.save_dir:
        save_league(args.save_dir, bank, league)
        summary["saved"] = args.save_dir
    ppo.finish_summary(summary, env, hist, args.out)


if __name__ == "__main__":
    main()
