"""CPU: checkpoint directories (checkpoint.py), snapshot and checkpoint files (snapshot.py) and the argument checks of the cda_snapshot_* entry points -
everything of a resumable run that needs no GPU."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from gym_continuousdoubleauction_amd import _capi as K, checkpoint as CK, snapshot as S  # noqa: E402


def _state(tag=0):
    return {"kind": "ppo", "run_id": "r", "args": {"markets": 4}, "tag": tag}


def test_iter_naming_staging_and_pruning(tmp_path):
    d = str(tmp_path / "ck")
    for n in (1, 2, 3, 4, 5):
        p = CK.save_checkpoint(d, n, _state(n), keep=3)
        assert os.path.basename(p) == f"iter_{n}" and not os.path.exists(p + ".tmp")
    assert [n for n, _ in CK.list_checkpoints(d)] == [3, 4, 5]
    rec, snap = CK.load_checkpoint(os.path.join(d, "iter_5"))
    assert rec["tag"] == 5 and rec["iteration"] == 5 and snap is None
    CK.save_checkpoint(d, 5, _state(55), keep=0)                 # an existing iter_<n> is replaced; keep 0 keeps all
    assert CK.load_checkpoint(os.path.join(d, "iter_5"))[0]["tag"] == 55


def test_newest_skips_staging_and_foreign_directories(tmp_path):
    d = str(tmp_path / "ck")
    CK.save_checkpoint(d, 2, _state(), keep=5)
    CK.save_checkpoint(d, 10, _state(), keep=5)
    os.makedirs(os.path.join(d, "iter_99.tmp"))                 # an interrupted save
    torch.save({}, os.path.join(d, "iter_99.tmp", CK.STATE_FILE))
    os.makedirs(os.path.join(d, "iter_50"))                      # no state file: not a checkpoint
    os.makedirs(os.path.join(d, "logs"))
    open(os.path.join(d, "iter_70"), "w").close()                # a file, not a directory
    assert CK.newest_checkpoint(d).endswith("iter_10")
    assert CK.resolve_restore(d, True).endswith("iter_10")
    assert CK.newest_checkpoint(str(tmp_path / "none")) is None
    with pytest.raises(FileNotFoundError):
        CK.resolve_restore(str(tmp_path / "none"), True)
    for bad in (os.path.join(d, "iter_50"), os.path.join(d, "logs"), os.path.join(d, "iter_99.tmp"), os.path.join(d, "iter_70")):
        with pytest.raises(ValueError, match="not a checkpoint"):
            CK.resolve_restore(d, bad)


def test_target_and_delta_iterations():
    assert list(CK.iteration_range(0, 3)) == [0, 1, 2]
    assert list(CK.iteration_range(2, 3)) == [2]                 # iters is the target
    assert list(CK.iteration_range(3, 3)) == [] and list(CK.iteration_range(5, 3)) == []
    assert list(CK.iteration_range(2, 3, iters_is_delta=True)) == [2, 3, 4]


def test_checkpoint_records_are_validated(tmp_path):
    d = str(tmp_path / "ck")
    p = CK.save_checkpoint(d, 1, _state(), keep=3)
    f = os.path.join(p, CK.STATE_FILE)
    rec = torch.load(f, weights_only=True)
    for change, reason in ((dict(format="x"), "format tag"), (dict(version=99), "version")):
        torch.save(dict(rec, **change), f)
        with pytest.raises(ValueError, match=reason):
            CK.load_checkpoint(p)
    torch.save({k: v for k, v in rec.items() if k != "run_id"}, f)
    with pytest.raises(ValueError, match="run_id"):
        CK.load_checkpoint(p)


def test_argument_mismatch_names_the_field():
    a = {"markets": 4, "agents": 4, "horizon": 32, "hidden": [256, 256]}
    CK.check_args(a, dict(a))
    for k, v in (("markets", 8), ("horizon", 16), ("hidden", [128, 128]), ("agents", 5)):
        with pytest.raises(ValueError, match=k):
            CK.check_args(a, dict(a, **{k: v}))


def _fake_blob(n=2, extra=512):
    h = K.SnapshotHeader()
    h.magic, h.version, h.n_markets = K.SNAP_MAGIC, K.SNAP_VERSION, n
    h.header_bytes = S.table_bytes(n)
    h.total_bytes = h.header_bytes + extra
    h.book_capacity, h.record_stride, h.n_hist, h.num_agents = 256, 8192, 4, 4
    c, _ = K.make_config({"num_of_agents": 4})
    h.cfg = c
    raw = bytes(h) + bytes(h.total_bytes - C.sizeof(h))
    return S.Snapshot(torch.frombuffer(bytearray(raw), dtype=torch.uint8), S.parse_header(raw))


def test_snapshot_files_validate_without_a_gpu(tmp_path):
    snap = _fake_blob()
    p = str(tmp_path / "env.snap")
    S.save_snapshot(p, snap)
    back = S.load_snapshot(p)
    assert torch.equal(back.blob, snap.blob) and back.header == snap.header and len(back) == 2
    rec = torch.load(p, weights_only=True)
    for change, reason in ((dict(format="policy"), "format tag"), (dict(version=2), "version"), (dict(blob=rec["blob"][:-16]), "truncated"),
                           (dict(blob=rec["blob"][:100]), "truncated"), (dict(blob=rec["blob"].float()), "uint8")):
        torch.save(dict(rec, **change), p)
        with pytest.raises(ValueError, match=reason):
            S.load_snapshot(p)
    bad = rec["blob"].clone()
    bad[0] ^= 0xFF
    torch.save(dict(rec, blob=bad), p)
    with pytest.raises(ValueError, match="magic"):
        S.load_snapshot(p)
    bad = rec["blob"].clone()
    bad[4] = 7
    torch.save(dict(rec, blob=bad), p)
    with pytest.raises(ValueError, match="version"):
        S.load_snapshot(p)


def test_snapshot_config_mismatch_names_the_field():
    snap = _fake_blob()

    class FakeEnv:
        book_capacity, n_hist, num_agents = 256, 4, 4
        cfg_struct = K.make_config({"num_of_agents": 4})[0]

        def state_bytes_per_market(self):
            return 8192
    assert S.mismatch(snap.header, FakeEnv()) is None
    env = FakeEnv()
    env.cfg_struct = K.make_config({"num_of_agents": 4, "tick_size": 2})[0]
    assert "tick_size" in S.mismatch(snap.header, env)
    env = FakeEnv()
    env.cfg_struct = K.make_config({"num_of_agents": 4, "book_spill": 4096})[0]
    assert S.mismatch(snap.header, env) is None                   # the ring size may differ
    env = FakeEnv()
    env.n_hist = 2
    assert "n_hist" in S.mismatch(snap.header, env)
    env = FakeEnv()
    env.episode_metrics_on = True
    assert "episode_metrics_on" in S.mismatch(snap.header, env)


def test_snapshot_header_matches_the_c_layout(tmp_path):
    import subprocess
    src = tmp_path / "h.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu\\n",sizeof(cda_snapshot_header),'
                   'offsetof(cda_snapshot_header,total_bytes),offsetof(cda_snapshot_header,cfg));return 0;}\n' % os.path.join(ROOT, "include", "cda.h"))
    exe = tmp_path / "h"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(K.SnapshotHeader), K.SnapshotHeader.total_bytes.offset, K.SnapshotHeader.cfg.offset] == [256, 16, 72]


@pytest.fixture(scope="module")
def hip_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_hip()
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib()


def test_entry_points_refuse_bad_arguments_before_the_device(hip_lib):
    L = hip_lib
    assert L.cda_snapshot_table_bytes(0) == 0 and L.cda_snapshot_table_bytes(1) == 512 and L.cda_snapshot_table_bytes(31) == 512
    assert L.cda_snapshot_table_bytes(32) == 768
    assert all(L.cda_snapshot_table_bytes(n) == S.table_bytes(n) for n in (1, 5, 31, 32, 100, 8192))
    assert L.cda_snapshot_offsets(None, 0, 1, None, None) == -1
    assert L.cda_snapshot_pack(None, 0, 1, None, None, 0, None) == -1
    assert L.cda_snapshot_restore(None, 0, None, 0, 0, 1, None, None) == -1
    h = K.SnapshotHeader()
    assert L.cda_snapshot_check_header(None, C.byref(h), 256) == -1


def test_snapshot_kernels_spill_nothing():
    """the new kernels: no VGPR spill, no scratch (read from the built library's code-object metadata, as test_kernel_resources does)"""
    import shutil
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_kernel_resources import OBJDUMP, READELF, _kernels
    if not (os.path.exists(READELF) and os.path.exists(OBJDUMP) and shutil.which(os.environ.get("HIPCC", "hipcc"))):
        pytest.skip("needs hipcc and the ROCm LLVM tools")
    ks, _ = _kernels()
    snap = {n: v for n, v in ks.items() if "k_snap_" in n}
    assert len(snap) == 4, sorted(snap)
    for n, v in snap.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (n, v)


def test_resumable_run_refusals():
    assert CK.check_resumable(None, 0, None) is False
    assert CK.check_resumable("d", 0, None) is True and CK.check_resumable(None, 0, True) is True
    for kw, reason in ((dict(checkpoint_dir=None, chkpt_freq=2, restore=None), "checkpoint_dir"), (dict(checkpoint_dir="d", chkpt_freq=-1, restore=None), ">= 0"),
                       (dict(checkpoint_dir="d", chkpt_freq=1, restore=None, world=2), "world"),
                       (dict(checkpoint_dir="d", chkpt_freq=1, restore=None, recorder=object()), "recorder")):
        with pytest.raises(ValueError, match=reason):
            CK.check_resumable(**kw)


def test_staged_extra_directories_move_into_the_checkpoint(tmp_path):
    d = str(tmp_path / "ck")
    extra = tmp_path / "staged"
    extra.mkdir()
    (extra / "league.json").write_text("{}")
    p = CK.save_checkpoint(d, 4, _state(), keep=3, extra_dirs={"league": str(extra)})
    assert os.path.isfile(os.path.join(p, "league", "league.json")) and not extra.exists()


def test_argument_record_builder_writes_the_loops_keys_exactly():
    """checkpoint.run_args - the part of a checkpoint's `args` both fused loops write - on stand-ins for the policy and the env: tanh / not tanh, separate / shared
    trunk, with / without scripted opponents.  The expected dicts are what the loops' inline code wrote before the builder existed, for the same inputs: check_args
    compares the union of the keys, so one key more, one less or one other value would refuse every checkpoint written until now."""
    import types
    from gym_continuousdoubleauction_amd import ppo
    from gym_continuousdoubleauction_amd.mlp import init_theta

    def policy(activation, vfs, head, hidden):
        theta = init_theta(168, generator=torch.Generator().manual_seed(0), state_dependent_log_std=head, hidden=hidden, vf_share_layers=vfs)
        return types.SimpleNamespace(theta=theta, activation=activation, vf_share_layers=vfs)
    ppo_objective = {"gamma": 0.99, "lam": 0.95, "clip": 0.2, "vf_coef": 0.5, "ent_coef": 0.01, "max_norm": 0.5, "kl_coef": 0.0, "kl_target": 0.01, "vf_clip": 0.0,
                     "bootstrap_truncation": 0.0, "reward_scale": 0.001}
    rllib_objective = {"gamma": 0.99, "lam": 1.0, "clip": 0.3, "vf_coef": 1.0, "ent_coef": 0.0, "max_norm": float("inf"), "kl_coef": 0.2, "kl_target": 0.01, "vf_clip": 10.0,
                       "bootstrap_truncation": 1.0, "reward_scale": 1.0}
    plain = CK.run_args(policy("tanh", False, False, (256, 256)), types.SimpleNamespace(n_markets=256, num_agents=4), 32, 2, ppo.PPO_DEFAULTS, 4, 5e-5, 262144, 0, True)
    assert plain == {"markets": 256, "agents": 4, "horizon": 32, "chains": 2, "objective": ppo_objective, "hidden": [256, 256], "state_dependent_log_std": False,
                     "epochs": 4, "lr": 5e-05, "minibatch": 262144, "seed": 0, "episode_metrics": True}
    assert CK.with_scripted(plain, [], trained_slots=None) == plain             # (train_fused without scripted opponents: the record as it is)
    other = CK.run_args(policy("relu", True, True, (128, 64)), types.SimpleNamespace(n_markets=48, num_agents=6), 16, 3, ppo.RLLIB_DEFAULTS, 2, 1e-4, 4096, 7, False)
    common = {"markets": 48, "agents": 6, "horizon": 16, "chains": 3, "objective": rllib_objective, "hidden": [128, 64], "state_dependent_log_std": True,
              "epochs": 2, "lr": 0.0001, "minibatch": 4096, "seed": 7, "episode_metrics": False, "activation": "relu", "vf_share_layers": True}
    assert other == common
    maker = {"law": 3, "size_mean": 0.05000000074505806, "size_sigma": 0.019999999552965164, "max_position": 200, "skew_position": 60, "max_orders": 3,
             "depth_levels": 1, "imb_num": 1, "imb_den": 1, "p_trade_q32": 0}
    taker = {"law": 2, "size_mean": 0.10000000149011612, "size_sigma": 0.05000000074505806, "max_position": 500, "skew_position": 0, "max_orders": 1,
             "depth_levels": 1, "imb_num": 1, "imb_den": 1, "p_trade_q32": 1073741824}
    imbalance = {"law": 4, "size_mean": 0.10000000149011612, "size_sigma": 0.05000000074505806, "max_position": 300, "skew_position": 0, "max_orders": 1,
                 "depth_levels": 3, "imb_num": 2, "imb_den": 1, "p_trade_q32": 0}
    # train_fused(trained_slots=2, opponents=[...]) ...
    assert CK.with_scripted(other, ["maker", "taker:p_trade_q32=1073741824"], trained_slots=2) == dict(common, scripted_opponents=[maker, taker], trained_slots=2)
    # ... and train_league_fused's own keys on top of the common ones, with a scripted module in the pool
    league = dict(other, max_step=32, trainable=1, max_champions=4, std_dev_multiplier=0.5, min_iterations_between_champions=1, original_opponent_weight=2.0,
                  champion_weight=1.5, run_id="lg")
    assert CK.with_scripted(league, ["imbalance:depth_levels=3"], scripted_weight=2.5) == {
        "markets": 48, "agents": 6, "horizon": 16, "max_step": 32, "chains": 3, "trainable": 1, "objective": rllib_objective, "hidden": [128, 64],
        "state_dependent_log_std": True, "epochs": 2, "lr": 0.0001, "minibatch": 4096, "seed": 7, "episode_metrics": False, "max_champions": 4,
        "std_dev_multiplier": 0.5, "min_iterations_between_champions": 1, "original_opponent_weight": 2.0, "champion_weight": 1.5, "run_id": "lg",
        "activation": "relu", "vf_share_layers": True, "scripted_opponents": [imbalance], "scripted_weight": 2.5}
    # an activation that is not tanh on separate networks, a shared trunk under tanh: one key each
    elu = CK.run_args(policy("elu", False, False, (256, 256)), types.SimpleNamespace(n_markets=256, num_agents=4), 32, 2, ppo.PPO_DEFAULTS, 4, 5e-5, 262144, 0, True)
    assert elu == dict(plain, activation="elu")
    shared = CK.run_args(policy("tanh", True, False, (256, 256)), types.SimpleNamespace(n_markets=256, num_agents=4), 32, 2, ppo.PPO_DEFAULTS, 4, 5e-5, 262144, 0, True)
    assert shared == dict(plain, vf_share_layers=True)


class _NoMarkets:
    """an env whose markets need no saving"""

    def snapshot(self):
        return None


def _save_points(tmp_path, iters, chkpt_freq, may_save=None, **kw):
    """the iterations a Run runs and the n_done it saves after, with a save function that only records"""
    run = CK.Run("ppo", checkpoint_dir=str(tmp_path / "ck"), chkpt_freq=chkpt_freq, iters=iters, **kw)
    if run.resumable:
        run.open({"markets": 4})
    saved = []
    for it in run.its:
        run.after_iteration(it, saved.append, may_save=may_save)
    return list(run.its), saved


def test_run_life_cycle_save_points_and_refusals(tmp_path):
    boundary = lambda n: n % 2 == 0                                           # noqa: E731 - the league's rule at two rollouts per episode
    assert _save_points(tmp_path, 5, 2) == ([0, 1, 2, 3, 4], [2, 4, 5])        # every second iteration and the final one
    assert _save_points(tmp_path, 4, 2) == ([0, 1, 2, 3], [2, 4])              # the final save is skipped when the last iteration was just saved
    assert _save_points(tmp_path, 3, 0) == ([0, 1, 2], [3])                    # chkpt_freq 0: the final one only
    assert _save_points(tmp_path, 5, 2, boundary) == ([0, 1, 2, 3, 4], [2, 4])  # ... and off an episode boundary
    assert _save_points(tmp_path, 4, 0, boundary) == ([0, 1, 2, 3], [4]) and _save_points(tmp_path, 3, 0, boundary) == ([0, 1, 2], [])
    assert _save_points(tmp_path, 0, 1) == ([], [])
    # not resumable: every iteration, no save, no argument record, no run id
    run = CK.Run("ppo", iters=3)
    saved = []
    for it in run.its:
        run.after_iteration(it, saved.append)
    assert (run.resumable, list(run.its), saved, run.args, run.state, run.run_id) == (False, [0, 1, 2], [], None, None, None)
    # a restore: the checkpoint's run id and iteration count; iters is the target, or - iters_is_delta - that many more
    d = str(tmp_path / "ck")
    CK.save_checkpoint(d, 3, {"kind": "ppo", "run_id": "first", "args": {"markets": 4}}, keep=3)
    assert _save_points(tmp_path, 5, 2, restore=True) == ([3, 4], [4, 5])
    assert _save_points(tmp_path, 3, 1, restore=True) == ([], [])               # at the target already: nothing runs, nothing is saved
    assert _save_points(tmp_path, 2, 0, restore=os.path.join(d, "iter_3"), iters_is_delta=True) == ([3, 4], [5])
    assert _save_points(tmp_path, 3, 2, boundary, restore=True, iters_is_delta=True) == ([3, 4, 5], [4, 6])
    run = CK.Run("ppo", checkpoint_dir=d, restore=True, iters=5)
    fresh = CK.Run("ppo", checkpoint_dir=d, iters=5)
    again = CK.Run("ppo", checkpoint_dir=d, iters=5)
    for r in (run, fresh, again):
        r.open({"markets": 4})
    assert run.run_id == "first" and run.path == os.path.join(d, "iter_3") and run.state["iteration"] == 3 and run.snapshot is None
    assert fresh.state is None and len(fresh.run_id) == 32 and fresh.run_id != again.run_id
    given = CK.Run("league", checkpoint_dir=d, run_id="league")
    given.open({"markets": 4})
    assert given.run_id == "league"
    # another loop's checkpoint, another run's arguments
    with pytest.raises(ValueError, match=r"is a 'ppo' checkpoint, not a league_train.train_league_fused one"):
        CK.Run("league", checkpoint_dir=d, restore=True).open({"markets": 4})
    CK.save_checkpoint(d, 4, {"kind": "league", "run_id": "lg", "args": {"markets": 4}}, keep=3)
    with pytest.raises(ValueError, match=r"is a 'league' checkpoint, not a ppo.train_fused one"):
        CK.Run("ppo", checkpoint_dir=d, restore=True).open({"markets": 4})
    for now, field in (({"markets": 8}, "markets"), ({"markets": 4, "activation": "relu"}, "activation"), ({}, "markets")):
        with pytest.raises(ValueError, match=f"checkpoint was written by a run with {field}"):
            CK.Run("ppo", checkpoint_dir=d, restore=os.path.join(d, "iter_3")).open(now)
    # the refusals of check_resumable are the constructor's
    for kw, reason in ((dict(chkpt_freq=2), "checkpoint_dir"), (dict(checkpoint_dir=d, world=2), "world"), (dict(checkpoint_dir=d, recorder=object()), "recorder")):
        with pytest.raises(ValueError, match=reason):
            CK.Run("ppo", **kw)
    # what a run saves: the loop's state under its kind, id and arguments
    run = CK.Run("ppo", checkpoint_dir=str(tmp_path / "w"), run_id="mine")
    run.open({"markets": 4})
    rec, _ = CK.load_checkpoint(run.save(2, {"kl_coef": 0.5}, _NoMarkets()))
    assert {k: rec[k] for k in ("kind", "run_id", "args", "kl_coef", "iteration")} == {"kind": "ppo", "run_id": "mine", "args": {"markets": 4}, "kl_coef": 0.5, "iteration": 2}
