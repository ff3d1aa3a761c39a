"""Snapshot / restore timing (include/cda.h cda_snapshot_*): blob bytes against the raw arena, kernel time by device events after warm-up, and the
bytes moved per second against the MI355X's 8 TB/s peak (about 6.3 TB/s achievable by a copy).  Shapes: 4096 x 4 and 8192 x 8 markets at max_step 4096,
after a few hundred random steps; the pack pass warm (repeated back to back: the blob stays in the Infinity Cache) and cold (512 MiB written in
between).  Load a variant library built with -DCDA_SNAP_NT_STORES=1 (tools/build_variant.sh) through CDA_HIP_LIB to time nt blob stores against the plain ones.
Also one checkpoint save's cost next to one train_fused iteration.  Prints JSON lines; --out writes them to a file
(profiles/snapshot/)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gym_continuousdoubleauction_amd import CDAVecEnv  # noqa: E402
from gym_continuousdoubleauction_amd._lib import check, lib  # noqa: E402

PEAK = 8.0e12


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e-3


def shape(n, a, steps, reps):
    env = CDAVecEnv({"num_of_agents": a, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}, n_markets=n, with_info=False)
    env.reset(seed=1)
    env.enable_episode_metrics(True)
    env.run_random(steps, action_seed=2)
    torch.cuda.synchronize()
    snap = env.snapshot()
    L, h, st = lib(), env._h, None
    off = torch.empty(n + 1, dtype=torch.int64, device=env.device)
    blob = torch.empty(snap.nbytes, dtype=torch.uint8, device=env.device)
    count = lambda: check(L.cda_snapshot_offsets(h, 0, n, off.data_ptr(), st), "offsets")                     # noqa: E731
    pack = lambda: check(L.cda_snapshot_pack(h, 0, n, off.data_ptr(), blob.data_ptr(), blob.numel(), st), "pack")   # noqa: E731
    for _ in range(3):
        count(); pack()
    torch.cuda.synchronize()
    t_count, t_pack = timed(count, reps), timed(pack, reps)             # WARM: the same 30-80 MB back to back, resident in the 256 MiB Infinity Cache
    flush = torch.empty(1 << 29, dtype=torch.uint8, device=env.device)  # COLD: 512 MiB written between two packs evicts L2 and the Infinity Cache
    cold = []
    for _ in range(reps):
        flush.fill_(1)
        cold.append(timed(pack, 1))
    t_pack_cold = sorted(cold)[len(cold) // 2]
    del flush
    t0 = time.perf_counter()
    for _ in range(3):
        env.restore(snap)
    torch.cuda.synchronize()
    t_restore_call = (time.perf_counter() - t0) / 3
    arena = int(env.state_bytes_per_market()) * n + n + n * a * 32 * 8 + n * 64 + n * (64 + env.book_spill * 2 * 4 * 4)
    out = {"shape": f"{n}x{a}", "steps": steps, "blob_bytes": snap.nbytes, "arena_bytes": arena, "ratio": arena / snap.nbytes,
           "offsets_s": t_count, "pack_warm_s": t_pack, "pack_warm_bytes_per_s": 2 * snap.nbytes / t_pack,
           "pack_cold_s (median, caches evicted)": t_pack_cold, "pack_cold_bytes_per_s": 2 * snap.nbytes / t_pack_cold, "pack_cold_of_peak": 2 * snap.nbytes / t_pack_cold / PEAK,
           "restore_call_s (host call: header read, device check, restore)": t_restore_call,
           "store_flavour": "nt" if os.environ.get("CDA_HIP_LIB") else "plain", "library": os.path.basename(os.environ.get("CDA_HIP_LIB") or "libcda_hip.so"),
           "spilled_orders": "none (300 random steps keep every book inside its tile)"}
    env.close()
    return out


def checkpoint_cost():
    from gym_continuousdoubleauction_amd import ppo
    env = CDAVecEnv({"num_of_agents": 4, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}, n_markets=4096, with_info=False)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        _, hist = ppo.train_fused(env, iters=3, horizon=64, log=lambda *_: None)
        t_plain = time.perf_counter() - t0
        env2 = CDAVecEnv({"num_of_agents": 4, "init_cash": 1000000, "max_step": 4096, "is_render": False, "auto_reset": True}, n_markets=4096, with_info=False)
        t0 = time.perf_counter()
        ppo.train_fused(env2, iters=3, horizon=64, log=lambda *_: None, checkpoint_dir=d, chkpt_freq=1)
        t_ck = time.perf_counter() - t0
        it_s = sum(h["rollout_s"] + h["update_s"] for h in hist) / len(hist)
        t0 = time.perf_counter()
        snap = env2.snapshot()
        torch.cuda.synchronize()
        t_snap = time.perf_counter() - t0
    return {"checkpoint": "4096x4 horizon 64 (configs[4])", "iteration_s": it_s, "snapshot_call_s": t_snap,
            "save_cost_per_iteration_s (3 saves, whole run difference / 3)": (t_ck - t_plain) / 3, "blob_bytes": snap.nbytes}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=None)
    p.add_argument("--no-checkpoint", action="store_true", help="only the pack / restore shapes (e.g. for a variant library loaded with CDA_HIP_LIB)")
    args = p.parse_args()
    rows = [shape(4096, 4, args.steps, args.reps), shape(8192, 8, args.steps, args.reps)] + ([] if args.no_checkpoint else [checkpoint_cost()])
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
