"""Random-agent driver for the MI355X env (the role `CDA_rand.run_random` plays in the reference,
gym_continuousDoubleAuction/CDA_rand.py:40-85: reset with a seed, draw every agent's action from its action
space, step until the horizon or an `__all__` flag).

Two modes:
  * `run_random(...)`   one market through the dict-shaped `CDAEnv` facade (BASELINE config #1 plumbing);
  * `run_random_batched(...)`  N markets through `CDAVecEnv` with the same uniform action law sampled on the GPU.

    python -m gym_continuousdoubleauction_amd.cda_rand --agents 4 --steps 1000 --seed 123 [--markets 4096]
    python -m gym_continuousdoubleauction_amd.cda_rand --markets 4096 --steps 256 --market-configs sweep.json     (`sweep`: one launch, many configs)
"""
import argparse
import sys
import time

# config/cli_defaults.json:9-14 of the reference
DEFAULT_AGENTS, DEFAULT_STEPS, DEFAULT_CASH = 4, 1000, 1000000


def _env_config(num_agents, max_step, init_cash):
    return {"num_of_agents": DEFAULT_AGENTS if num_agents is None else num_agents,
            "max_step": DEFAULT_STEPS if max_step is None else max_step,
            "init_cash": DEFAULT_CASH if init_cash is None else init_cash, "is_render": False}


def run_random(num_agents=None, max_step=None, init_cash=None, is_render=None, seed=None, device="cuda:0"):
    """Single market, dict API.  Returns the number of steps taken (the reference's contract)."""
    from .env import CDAEnv
    cfg = _env_config(num_agents, max_step, init_cash)
    env = CDAEnv(cfg, device=device)
    try:
        env.reset(seed=seed)
        space = env.action_spaces[env.agents[0]]            # one shared Dict space for every agent
        if seed is not None:
            space.seed(seed)
        taken = 0
        while taken < cfg["max_step"]:
            _, _, terminateds, truncateds, _ = env.step({aid: space.sample() for aid in env.agents})
            taken += 1
            if terminateds["__all__"] or truncateds["__all__"]:
                break
        return taken
    finally:
        env.close()


def run_random_batched(n_markets, num_agents=None, max_step=None, init_cash=None, seed=0, device="cuda:0", fused=True):
    """N markets; actions ~ the RandomRLModule law (train/model/model_handler.py:38-53) drawn on the device.
    fused=True: the whole episode of every market in ONE launch (`cda_run_random`: state stays in LDS, no market waits for
    the slowest of the batch); fused=False: one launch per step with torch-generated actions.
    Returns (steps, agent_steps_per_second)."""
    import torch
    from .vec_env import CDAVecEnv
    cfg = _env_config(num_agents, max_step, init_cash)
    env = CDAVecEnv(cfg, n_markets=n_markets, device=device, with_info=False)
    n, a = env.n_markets, env.num_agents
    if fused:
        env.reset(seed=seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, term, trunc, taken = env.run_random(cfg["max_step"], action_seed=seed)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if not bool((term | trunc).all()):
            raise RuntimeError("every market must end its episode within max_step")
        total = int(taken.sum().item())
        env.close()
        return int(taken.max().item()), total * a / dt
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    env.reset(seed=seed)
    torch.cuda.synchronize()
    t0, steps = time.perf_counter(), 0
    for _ in range(cfg["max_step"]):
        _, _, term, trunc, _ = env.step(
            torch.randint(0, 9, (n, a), generator=gen, device=device, dtype=torch.int32),
            torch.rand((n, a), generator=gen, device=device) * 2.0 - 1.0,
            torch.rand((n, a), generator=gen, device=device),
            torch.randint(0, 10, (n, a), generator=gen, device=device, dtype=torch.int32),
            torch.randint(0, 3, (n, a), generator=gen, device=device, dtype=torch.int32))
        steps += 1
        if steps == cfg["max_step"] and not bool(trunc.all()):
            raise RuntimeError("every market must truncate exactly on max_step")
    torch.cuda.synchronize()
    rate = n * a * steps / (time.perf_counter() - t0)
    env.close()
    return steps, rate


def sweep(configs, markets_per_config, steps, seed=0, base=None, device="cuda:0", env_out=None):
    """The tuning use case in one launch: the override dicts `configs` (per-market keys, market_params.PER_MARKET_KEYS) laid out over ONE env of
    len(configs) * markets_per_config markets (market m runs configs[m % len(configs)]), reset with `seed`, one cda_run_random launch of `steps`
    steps.  `base`: the env config the overrides apply to (default: 4 agents, init_cash 1e6, max_step = steps; a config's max_step may not exceed
    the env's).  Returns one dict per config: the markets that ran it, per agent the mean and std (population) of the episode return, and the mean
    and std of the steps taken.  env_out: a list that receives the env (left open) instead of closing it."""
    import numpy as np
    import torch
    from .vec_env import CDAVecEnv
    from .market_params import round_robin
    k, per = len(configs), int(markets_per_config)
    if k < 1 or per < 1:
        raise ValueError("sweep needs at least one config and one market per config")
    cfg = {"num_of_agents": DEFAULT_AGENTS, "init_cash": DEFAULT_CASH, "max_step": int(steps), "is_render": False}
    cfg.update(base or {})
    env = CDAVecEnv(cfg, n_markets=k * per, device=device, with_info=False, market_configs=round_robin(list(configs), k * per))
    try:
        env.reset(seed=seed)
        _, ret, _, _, taken = env.run_random(int(steps), action_seed=seed)
        ret = ret.cpu().numpy().astype(np.float64)
        taken = taken.cpu().numpy().astype(np.float64)
        torch.cuda.synchronize(env.device)
    finally:
        if env_out is None:
            env.close()
        else:
            env_out.append(env)
    out = []
    for c in range(k):
        r, t = ret[c::k], taken[c::k]
        out.append({"config": dict(configs[c]), "markets": int(len(r)), "return_mean": r.mean(axis=0).tolist(), "return_std": r.std(axis=0).tolist(),
                    "steps_mean": float(t.mean()), "steps_std": float(t.std())})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Random-agent CDA simulation on one MI355X.")
    ap.add_argument("--agents", type=int, default=DEFAULT_AGENTS)
    ap.add_argument("--steps", type=int, default=DEFAULT_STEPS)
    ap.add_argument("--init-cash", type=int, default=DEFAULT_CASH)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--markets", type=int, default=1, help="> 1 runs the batched env")
    ap.add_argument("--per-step-launch", action="store_true", help="batched env: one launch per step instead of one per episode")
    ap.add_argument("--market-configs", default=None, metavar="FILE.json", help="a sweep: a JSON list of per-market override dicts, market m runs entry m %% len(list); "
                                                                              "prints one JSON line per entry (cda_rand.sweep over --markets markets)")
    args = ap.parse_args(argv)
    if args.market_configs:
        import json
        from .market_params import load_market_configs
        configs = load_market_configs(args.market_configs)
        for row in sweep(configs, max(1, args.markets // len(configs)), args.steps, seed=args.seed or 0,
                         base={"num_of_agents": args.agents, "init_cash": args.init_cash}):
            print(json.dumps(row))
        return 0
    if args.markets > 1:
        steps, rate = run_random_batched(args.markets, args.agents, args.steps, args.init_cash, seed=args.seed or 0,
                                         fused=not args.per_step_launch)
        print(f"{args.markets} markets x {args.agents} random agents: {steps} steps, {rate / 1e6:.1f} M agent-steps/s")
    else:
        steps = run_random(args.agents, args.steps, args.init_cash, seed=args.seed)
        print(f"completed {steps} steps with {args.agents} random agents.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
