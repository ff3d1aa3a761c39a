#!/usr/bin/env python3
"""What the label tap costs (CDAVecEnv.set_label_tap, csrc/cda_scripted_label.inc k_script_label).

mlp.RolloutChains (a shared policy, four chains, captured graphs, horizon 64) at 4096 markets x 4 agents and 2048 x 8, slot 0 the policy's, the slots behind it
scripted (maker, taker, imbalance), three configurations:
  (a) the PARENT tree (--head: its checkout, built), no tap - it has none;
  (b) this tree, no tap: cda_scripted_step_actions is cda_scripted_actions, the chains launch what (a) launches;
  (c) this tree, the tap attached (slot 0 labelled by the maker, mix 0.5): ONE k_script_label launch per step in k_script_actions' place.
The alternative (c) replaces is (b) plus a second, dependent launch per step through cda_label_actions; (b)'s runs time that launch as well - `horizon` of them
captured back to back into a graph of their own and replayed, the way a fourth launch would sit in a chain - and the alternative's per-step time is the sum.
The three alternate in one call, --runs times each, the order rotated every round; every run is a fresh child process that measures both shapes: three warm-up
rollouts (the first captures), then --reps timed ones; host-clock time around the replays, ending in a device synchronise, over reps x horizon steps.

    python tools/dagger_cost_probe.py --head _ab_head --out profiles/dagger/cost.txt [--runs 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTED = ["maker", "taker", "imbalance"]
SHAPES = [(4096, 4), (2048, 8)]


def child(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd import scripted as S
    from gym_continuousdoubleauction_amd._lib import check, lib
    T, out = args.horizon, {}
    for n, a in SHAPES:
        env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}, n_markets=n, device="cuda:0", with_info=False)
        env.reset(seed=1)
        env.set_scripted(S.opponent_slots(n, a, 1, len(SCRIPTED)), SCRIPTED, seed=1)
        label = np.zeros((n, a), np.int32)
        label[:, 0] = 1
        if args.tap:
            env.set_label_tap(label, ["maker"], rows=T, seed=1, mix=0.5)
        chains = mlp.RolloutChains(env, mlp.FusedPolicy("cuda:0", seed=1), T, groups=4, seed=5, trained_slots=1)
        for _ in range(3):
            chains.run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            chains.run()
        torch.cuda.synchronize()
        res = {"us_per_step": 1e6 * (time.perf_counter() - t0) / (args.reps * T), "graphs": chains.graphs is not None}
        if args.second_launch:                                   # the alternative's second launch: T dependent cda_label_actions launches, captured and replayed
            slot_t = torch.from_numpy(label).to("cuda:0")
            prof_t = torch.from_numpy(S.profiles_array([S.parse_profile("maker")]).view(np.uint8).reshape(1, 64).copy()).to("cuda:0")
            acts = env._action_buffers()
            ctr = torch.ones(1, dtype=torch.int64, device="cuda:0")
            keys = ("category", "size_mean", "size_sigma", "price", "price_offset")
            g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream("cuda:0")
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                st = torch.cuda.current_stream("cuda:0").cuda_stream
                for t in range(T):
                    check(lib().cda_label_actions(env._h, 0, n, slot_t.data_ptr(), prof_t.data_ptr(), 1, 1, 0, ctr.data_ptr(), t, *(acts[k].data_ptr() for k in keys), st),
                          "cda_label_actions")
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                g.replay()
            torch.cuda.synchronize()
            res["label_launch_us"] = 1e6 * (time.perf_counter() - t0) / (args.reps * T)
        res["flagged_or_invalid_markets"] = int((env.flags() != 0).sum()) + int((env.check_invariants() != 0).sum())
        out[f"{n}x{a}"] = res
        env.close()
    print(json.dumps(out))


def run_one(tree, tap, second, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--horizon", str(args.horizon), "--reps", str(args.reps)] + (["--tap"] if tap else []) + \
          (["--second-launch"] if second else [])
    r = subprocess.run(["timeout", "-k", "10", str(args.timeout)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} exited {r.returncode}:\n{r.stderr[-2000:]}")       # (a faulted child ends the probe: nothing more is started)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", default=None, help="a built checkout of the parent tree (configuration (a); skipped when absent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dagger", "cost.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40, help="timed rollouts per shape and run, after three warm-up rollouts")
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child run")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--tap", action="store_true")
    ap.add_argument("--second-launch", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    sides = ([("a", os.path.abspath(args.head), False, False)] if args.head else []) + [("b", ROOT, False, True), ("c", ROOT, True, False)]
    res = {s[0]: [] for s in sides}
    for i in range(args.runs):
        for name, tree, tap, second in sides[i % len(sides):] + sides[:i % len(sides)]:
            res[name].append(run_one(tree, tap, second, args))
            print(name, json.dumps(res[name][-1]), flush=True)
    what = {"a": "(a) parent commit, no tap", "b": "(b) this commit, no tap", "c": "(c) this commit, tap attached (one k_script_label launch per step)"}
    lines = [f"mlp.RolloutChains, one shared policy in slot 0, {', '.join(SCRIPTED)} behind it, 4 chains, captured graphs, horizon {args.horizon}; {args.runs} runs each, alternating in one",
             f"call, each a fresh process: 3 warm-up rollouts + {args.reps} timed per shape; host-clock time ending in a device synchronise, per step.",
             f"    python tools/dagger_cost_probe.py --head <built parent checkout> --runs {args.runs} --reps {args.reps}", ""]
    for n, a in SHAPES:
        key = f"{n}x{a}"
        lines.append(f"{n} markets x {a} agents")
        med = {}
        for name in res:
            r = [x[key]["us_per_step"] for x in res[name]]
            med[name] = statistics.median(r)
            lines.append(f"  {what[name]}: median {med[name]:.2f} us per step, spread {min(r):.2f} .. {max(r):.2f}; runs {', '.join(f'{v:.2f}' for v in r)}; graphs "
                         f"{all(x[key]['graphs'] for x in res[name])}; flagged or invalid markets {sum(x[key]['flagged_or_invalid_markets'] for x in res[name])}")
        if "a" in res:
            lo, hi = min(x[key]["us_per_step"] for x in res["a"]), max(x[key]["us_per_step"] for x in res["a"])
            lines.append(f"  (b) median inside the spread of (a): {'yes' if lo <= med['b'] <= hi else 'NO'} ({med['b'] / med['a'] - 1.0:+.2%} against (a)'s median)")
        second = [x[key]["label_launch_us"] for x in res["b"]]
        alt = statistics.median(x[key]["us_per_step"] + x[key]["label_launch_us"] for x in res["b"])
        lines.append(f"  a second, dependent cda_label_actions launch per step (captured, replayed): median {statistics.median(second):.2f} us, spread {min(second):.2f} .. {max(second):.2f}")
        lines.append(f"  the alternative, (b) + that launch: {alt:.2f} us per step; (c): {med['c']:.2f} us per step ({med['c'] / alt - 1.0:+.2%}); the tap's own cost over (b): "
                     f"{med['c'] - med['b']:+.2f} us per step - {'the fused kernel beats the two launches' if med['c'] < alt else 'the fused kernel does NOT beat the two launches'}")
        lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
