#!/usr/bin/env python3
"""Build-container tool (needs /root/reference): beyond the committed goldens, pit the CPU oracle against the REAL reference
on many fresh random episodes - random agent counts, balances, size ranges, price ranges, history depths, coefficients, action
laws, agent subsets, dict key orders that change every step, books of thousands of orders - comparing every recorded field bit for bit (the same comparison tests/test_oracle_golden.py runs).
Nothing is written; the point is the count of episodes that agree.

    PYTHONPATH=tests/golden/shim:/root/reference:tests:. python tests/golden/crosscheck_oracle.py [n_episodes] [seed]

With --services the episodes are the cases of the services fuzz (tests/fuzz_cases.py service_case; tests/test_hip_services_fuzz.py trusts the oracle on them): the
case's config - its redrawn history depth and, in short-horizon cases, its max_step included - once per distinct per-market row, under the case's law, agent
subsets and dict order, for the case's number of steps (a short-horizon case: one whole episode).  n_episodes then counts cases (default: the fuzz's own
twelve), seed defaults to the fuzz's.

    PYTHONPATH=tests/golden/shim:/root/reference:tests:. python tests/golden/crosscheck_oracle.py --services [n_cases] [seed]

With --edges the episodes are the cases of the config-edge tests (tests/fuzz_cases.py edge_cases; tests/test_hip_config_edges.py trusts the oracle on them): per case
EDGE_EPISODES episodes, from the case's first reset seeds, under its config, law, agent subsets and dict order, for the case's number of steps (at most one
horizon: the reference has no in-episode reset).  n then counts cases (default: the tests' own 32), seed defaults to theirs.

    PYTHONPATH=tests/golden/shim:/root/reference:tests:. python tests/golden/crosscheck_oracle.py --edges [n_cases] [seed]
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "shim"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_goldens as MG  # noqa: E402
import golden_util as G  # noqa: E402
import oracle_lib as O  # noqa: E402


def random_case(rng, i):
    from fuzz_cases import random_config, random_order
    cfg, law, present_p = random_config(rng)
    T = int(rng.integers(40, 140)) if law != "trend" else int(rng.integers(200, 700))      # (the trend law needs time to outgrow a tile)
    return f"x{i}", cfg, int(rng.integers(0, 2 ** 63)), T, int(rng.integers(0, 2 ** 31)), law, present_p, random_order(rng)


def service_episodes(n, seed):
    """the (config x row) episodes of the first n service cases: random_case's tuples"""
    import fuzz_cases as F
    out = []
    for i, case in enumerate(F.service_cases(F.SERVICE_SEED if seed is None else seed, F.SERVICE_CASES if n is None else n)):
        base = {k: v for k, v in case["oracle_cfg"].items() if k not in ("book_capacity", "book_spill")}       # (the reference has no tile and no ring)
        rng = np.random.default_rng(case["seed"])
        for j, row in enumerate(case["rows"] or [{}]):
            cfg = dict(base, **row)
            T = min(F.SERVICE_STEPS + F.SERVICE_STEPS_AFTER, cfg["max_step"])
            out.append((f"s{i}r{j}", cfg, int(rng.integers(0, 2 ** 63)), T, int(rng.integers(0, 2 ** 31)), case["law"], case["present_p"], case["order"]))
    return out


EDGE_EPISODES = 4


def edge_episodes(n, seed):
    """EDGE_EPISODES episodes of each of the first n edge cases: random_case's tuples"""
    import fuzz_cases as F
    out = []
    for i, case in enumerate(F.edge_cases(F.EDGE_SEED if seed is None else seed, F.EDGE_CASES if n is None else n)):
        cfg = {k: v for k, v in case["oracle_cfg"].items() if k not in ("book_capacity", "book_spill")}       # (the reference has no tile and no ring)
        rng = np.random.default_rng(case["seed"])
        for j in range(EDGE_EPISODES):
            out.append((f"e{i}m{j}", cfg, int(case["seeds"][j]), min(case["steps"], cfg["max_step"]), int(rng.integers(0, 2 ** 31)), case["law"], case["present_p"],
                        case["order"]))
    return out


def main():
    modes = [a for a in sys.argv[1:] if a in ("--services", "--edges")]
    args = [a for a in sys.argv[1:] if a not in ("--services", "--edges")]
    edges = "--edges" in modes
    listed = bool(modes)                                  # --services or --edges: the episodes are listed up front, not drawn one by one
    n = int(args[0]) if args else (None if listed else 200)
    seed = int(args[1]) if len(args) > 1 else (None if listed else 2024)
    episodes = (edge_episodes(n, seed) if edges else service_episodes(n, seed)) if listed else None
    rng = np.random.default_rng(seed)
    steps = 0
    n = len(episodes) if listed else n
    for i in range(n):
        name, cfg, seed, T, aseed, law, present_p, order = episodes[i] if listed else random_case(rng, i)
        with contextlib.redirect_stdout(io.StringIO()):
            rec = MG.run_trace(name, cfg, seed, T, aseed, law=law, present_p=present_p, dict_order=order)
        rec = {k: (v if isinstance(v, np.ndarray) else np.asarray(v)) for k, v in rec.items()}
        rec["config"] = json.loads(str(rec["config"]))
        rec["name"] = name
        full_cfg = dict(rec["config"])
        env = O.OracleEnv(full_cfg, n_markets=1)
        try:
            steps += G.run_group(env, [rec], state_every=1, trace_getter=lambda: env.trace)
        except AssertionError as e:
            print(f"MISMATCH in episode {i}: config={cfg} seed={seed} law={law} present_p={present_p} order={order}\n  {e}")
            return 1
        finally:
            env.close()
        if (i + 1) % 50 == 0:
            print(f"{i + 1} episodes, {steps} steps: all fields identical")
    kind = ("edge-case" if edges else "service-case") if listed else "random"
    print(f"oracle == reference on {n} {kind} episodes ({steps} steps)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
