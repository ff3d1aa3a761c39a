"""CPU: the host side of order schedules (gym_continuousdoubleauction_amd/orders.py, checkpoint.with_order_schedule, cda_schedule_check_host) - packing rows of
per-step windows, cutting a recorded episode into them, the seed window, files, the digest, the attach rule on host data and the checkpoint's refusal.  No GPU."""
import os
import sys

import numpy as np
import pytest

from gym_continuousdoubleauction_amd import _capi as K
from gym_continuousdoubleauction_amd import checkpoint as CK
from gym_continuousdoubleauction_amd import orders as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS = [[[(0, 1, 0, 5, 50), (1, 1, 1, 4, 60)], [], [("mark",)]],
        [[], [(2, 0, 1, 3, 0)], [(3, 3, 0, 1, 50), (0, 2, 0, 2, 49), (1, 1, 1, 9, 70)]]]


def test_pack_schedule_offsets_and_round_trip():
    sched = OR.pack_schedule(ROWS)
    off, msgs = sched
    assert off.dtype == np.int64 and off.tolist() == [[0, 2, 2, 3], [3, 3, 4, 7]] and msgs.dtype == OR.MSG_DTYPE and len(msgs) == 7
    assert (sched.n_sched, sched.n_steps) == (2, 3)
    assert sched.window(1, 2)["price"].tolist() == [50, 49, 70] and len(sched.window(0, 1)) == 0
    assert int(msgs[2]["type"]) == OR.OP_MARK
    back = sched.rows()
    assert back[0][2] == [OR.MARK] and [m[:5] for m in back[1][2]] == [tuple(m) for m in ROWS[1][2]]
    for bad in ([], [[]], [[[]], [[], []]]):
        with pytest.raises(ValueError):
            OR.pack_schedule(bad)


def test_schedule_from_lob_actions_is_the_per_step_split_of_the_stream():
    rng = np.random.default_rng(3)
    T, A = 12, 4
    la = np.stack([rng.integers(-1, 2, (T, A)), rng.integers(0, 4, (T, A)), rng.integers(1, 9, (T, A)), rng.integers(1, 99, (T, A))], axis=2)
    la[la[:, :, 0] < 0] = (-1, 0, 0, 0)
    ex = np.zeros((T, A), np.int64)
    for t in range(T):
        acting = [a for a in range(A) if la[t, a, 0] >= 0]
        ex[t, :len(acting)] = rng.permutation(acting)
    whole = OR.from_lob_actions(la, ex)
    for traders in (None, (1, 3), (2,)):
        windows = OR.schedule_from_lob_actions(la, ex, traders=traders)
        assert len(windows) == T
        flat = [m for w in windows for m in w]
        assert flat == [m for m in whole if traders is None or m[0] in traders]
        assert all(m[5] == t for t, w in enumerate(windows) for m in w)
    with pytest.raises(ValueError):
        OR.schedule_from_lob_actions(la[0])


def test_the_seed_window_is_from_book():
    bids = np.array([[50, 5, 0, 1, 1], [49, 2, 1, 2, 2]], np.int32)
    asks = np.array([[52, 3, 2, 3, 3]], np.int32)
    rows = OR.schedule_with_seed(bids, asks, ROWS)
    assert len(rows) == 2 and all(len(r) == 4 for r in rows)
    for r, src in zip(rows, ROWS):
        assert r[0] == OR.from_book(bids, asks) and r[1:] == [list(w) for w in src]
    assert OR.pack_schedule(rows).step_offsets[:, 1].tolist() == [3, 3 + 3 + 3]


def test_files_and_the_digest(tmp_path):
    sched = OR.pack_schedule(ROWS)
    ms = np.array([0, 1, -1, 1], np.int32)
    path = str(tmp_path / "s.npz")
    OR.save_schedule(path, sched, market_schedule=ms, loop=True)
    back, ms_b, loop, clear = OR.load_schedule(path)
    assert np.array_equal(back.step_offsets, sched.step_offsets) and back.msgs.tobytes() == sched.msgs.tobytes()
    assert np.array_equal(ms_b, ms) and loop and not clear
    OR.save_schedule(path, sched)
    assert OR.load_schedule(path)[1:] == (None, False, False)
    base = OR.schedule_digest(sched, ms, loop=True)
    assert base == OR.schedule_digest(back, ms_b, loop=True) and len(base) == 64
    other = [base]
    off2 = sched.step_offsets.copy(); off2[0, 1] = 1
    other.append(OR.schedule_digest(OR.PackedSchedule(off2, sched.msgs), ms, loop=True))
    m2 = sched.msgs.copy(); m2[4]["tag"] = 9
    other.append(OR.schedule_digest(OR.PackedSchedule(sched.step_offsets, m2), ms, loop=True))
    other.append(OR.schedule_digest(sched, np.array([0, 1, 0, 1], np.int32), loop=True))
    other.append(OR.schedule_digest(sched, ms, loop=False))
    other.append(OR.schedule_digest(sched, ms, loop=True, clear_step_counters=True))
    assert len(set(other)) == len(other)


@pytest.fixture(scope="module")
def hip_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_hip()
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib()


def test_the_host_check_accepts_the_good_case_and_names_each_bad_one(hip_lib):
    sched = OR.pack_schedule(ROWS)
    good_so = np.array([0, 1, -1, 1, 0], np.int32)

    def both(so, off, n_msgs=len(sched.msgs)):
        so, off = np.ascontiguousarray(so, np.int32), np.ascontiguousarray(off, np.int64)
        rc = hip_lib.cda_schedule_check_host(4, len(so), so.ctypes.data, off.ctypes.data, off.shape[0], off.shape[1] - 1, n_msgs)
        msgs = np.zeros(n_msgs, OR.MSG_DTYPE)
        why = OR.schedule_check(OR.PackedSchedule(off, msgs), so, 4)
        assert (OR.SCHEDULE_FAULTS[rc] if rc > 0 else None) == why, (rc, why)       # the library's rule and its Python statement agree
        return rc, why

    assert both(good_so, sched.step_offsets) == (0, None)
    down = sched.step_offsets.copy(); down[1, 2] = 2
    assert both(good_so, down) == (3, "decreasing row")
    assert both(good_so, sched.step_offsets, n_msgs=6) == (4, "end beyond n_msgs")
    assert both([0, 2, 0, 0, 0], sched.step_offsets) == (1, "sched_of out of range") and both([0, -2, 0, 0, 0], sched.step_offsets)[0] == 1
    neg = sched.step_offsets.copy(); neg[0, 0] = -1
    assert both(good_so, neg) == (2, "negative start")
    so, off = good_so, sched.step_offsets
    for args in ((0, 5, so.ctypes.data, off.ctypes.data, 2, 3, 7), (K.MAX_AGENTS + 1, 5, so.ctypes.data, off.ctypes.data, 2, 3, 7), (4, 0, so.ctypes.data, off.ctypes.data, 2, 3, 7),
                 (4, 5, None, off.ctypes.data, 2, 3, 7), (4, 5, so.ctypes.data, None, 2, 3, 7), (4, 5, so.ctypes.data, off.ctypes.data, 0, 3, 7),
                 (4, 5, so.ctypes.data, off.ctypes.data, 2, 0, 7), (4, 5, so.ctypes.data, off.ctypes.data, 2, 3, -1)):
        assert hip_lib.cda_schedule_check_host(*args) == -1, args


def test_checkpoint_arguments_carry_the_digest_only_when_a_schedule_is_attached():
    args = {"horizon": 8, "seed": 3}
    assert CK.with_order_schedule(args, None) == args and CK.with_order_schedule(args, None) is not args
    d1 = OR.schedule_digest(OR.pack_schedule(ROWS), [0, 1], loop=False)
    d2 = OR.schedule_digest(OR.pack_schedule(ROWS), [0, 1], loop=True)
    with_1 = CK.with_order_schedule(args, d1)
    assert with_1 == dict(args, order_schedule=d1)
    CK.check_args(with_1, CK.with_order_schedule(args, d1))
    for saved, now in ((with_1, args), (args, with_1), (with_1, CK.with_order_schedule(args, d2))):      # written with one / resumed without, the reverse, another schedule
        with pytest.raises(ValueError, match="order_schedule"):
            CK.check_args(saved, now)


def test_the_command_lines_take_an_order_schedule():
    from gym_continuousdoubleauction_amd import league_train, ppo
    assert ppo.main(["--order-schedule", "s.npz"], parse_only=True).order_schedule == "s.npz"
    assert ppo.main([], parse_only=True).order_schedule is None
    assert league_train.main(["--fused", "--order-schedule", "s.npz"], parse_only=True).order_schedule == "s.npz"
    with pytest.raises(SystemExit):
        league_train.main(["--order-schedule", "s.npz"], parse_only=True)
