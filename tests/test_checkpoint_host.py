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
