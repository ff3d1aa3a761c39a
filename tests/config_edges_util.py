"""What tests/test_config_edges_host.py (the oracle alone) and tests/test_hip_config_edges.py (device against oracle) share: how an edge case of
tests/fuzz_cases.py is played.  A case's episodes are stepped under its own action stream; a market whose episode ended (terminated or truncated) is reset
with seed=None semantics before the next step - at max_step 1 and with init_cash <= 0 that is every market after every step."""
import numpy as np

import fuzz_cases as F


def case_steps(case):
    """(t, the five action arrays, present) of every step of the case"""
    rng = F.edge_actions(case)
    n, a = case["n_markets"], case["cfg"]["num_of_agents"]
    for t in range(case["steps"]):
        acts, present = F.batch_actions(rng, n, a, case["law"], case["present_p"], case["order"])
        yield t, acts, present


def done_mask(term, trunc):
    return ((np.asarray(term) != 0) | (np.asarray(trunc) != 0)).astype(np.uint8)


def play_on_oracle(case):
    """The case on the oracle alone.  Returns (why, fills, terminated, steps): why = None if the case was in reach at every step, else fuzz_cases.in_reach's
    first reason; fills = trades counted over all agents, markets and steps; terminated = markets x steps that ended terminated; steps = markets x steps played."""
    import oracle_lib as O
    ora = O.OracleEnv(case["oracle_cfg"], case["n_markets"])
    ora.reset(case["seeds"])
    why, fills, terminated = None, 0, 0
    for t, acts, present in case_steps(case):
        _obs, _rew, term, trunc, info = ora.step(*acts, present)
        if why is None:
            why = F.in_reach(case, ora)
            why = why and f"step {t}: {why}"
        fills += int(info["num_trades_step"].sum())
        terminated += int((term != 0).sum())
        done = done_mask(term, trunc)
        if done.any():
            ora.reset(None, done)
    ora.close()
    return why, fills, terminated, case["n_markets"] * case["steps"]


def generator_message(case_index, case, why):
    return (f"edge case {case_index} {case['edges']} is out of the device's reach ({why}): tests/fuzz_cases.py edge_case drew a case the device and the reference "
            f"do not agree on by design - fix the generator (or the seed), the kernel is not at fault.  cfg = {case['cfg']}")
