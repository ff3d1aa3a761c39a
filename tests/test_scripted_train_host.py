"""CPU: the host side of training against scripted opponents - the league mapper with scripted pool entries against numpy's own RandomState.choice, the
command lines, the canonical checkpoint arguments, the refusals that need no device, and the two new entry points of include/cda_mlp.h
(cda_gae_records_slots, cda_league_assign_scripted) with their prototypes."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mapper(A=8, k=2, fixed=None, champions=2):
    from gym_continuousdoubleauction_amd.league import LeagueSlotMapper
    m = LeagueSlotMapper(A, k, A - k if fixed is None else fixed, original_opponent_weight=1.0, champion_weight=3.0, scripted_weight=2.5)
    ids = [m.add_scripted(s) for s in ("maker", "taker:p_trade_q32=0x20000000", "imbalance")]
    for _ in range(champions):
        m.add_champion()
    return m, ids


def test_mapper_orders_and_weights_scripted_modules():
    m, ids = _mapper()
    assert ids == ["scripted_0_maker", "scripted_1_taker", "scripted_2_imbalance"]
    assert m.available_modules == [f"policy_{i}" for i in range(8)] + ids + ["champion_1", "champion_2"]
    w = np.array([1.0] * 6 + [2.5] * 3 + [3.0] * 2)
    assert np.array_equal(m.pool_probabilities(), w / w.sum())
    # a scripted module registered after a champion still sits before it; a later champion goes to the end
    late = m.add_scripted("pass")
    assert late == "scripted_3_pass" and m.available_modules[-4:] == ["scripted_2_imbalance", "scripted_3_pass", "champion_1", "champion_2"]
    assert m.add_champion() == "champion_3" and m.available_modules[-1] == "champion_3"
    assert [p.law for p in m.scripted_profiles()] == [3, 2, 4, 1] and m.scripted_profiles()[1].p_trade_q32 == 0x20000000
    with pytest.raises(ValueError, match="scripted"):
        m.remove(late)
    # the default weight is the reference rule's "otherwise"
    from gym_continuousdoubleauction_amd.league import LeagueSlotMapper
    d = LeagueSlotMapper(4, 1, 0, 2.0, 3.0)
    d.add_scripted("maker"); d.add_champion()
    assert d.pool() == ["scripted_0_maker", "champion_1"] and np.array_equal(d.pool_probabilities(), np.array([0.25, 0.75]))


@pytest.mark.parametrize("A,k,fixed", [(8, 2, None), (16, 1, None), (4, 3, None), (4, 1, 0)])
def test_assign_with_scripted_entries_is_numpys_choice(A, k, fixed):
    """assign() - unchanged, the specification - against np.random.RandomState((crc32(str(id)) + slot) % 2**32).choice(pool, p=probs) taken directly"""
    m, _ = _mapper(A, k, fixed)
    pool, probs = m.pool(), m.pool_probabilities()
    ids = [f"host-episode{e}-market{i}" for e in range(3) for i in range(16)]
    got = m.assign(ids)
    drawn = set()
    for row, eid in zip(got, ids):
        assert row[:k].tolist() == list(range(k))
        for slot in range(k, A):
            want = np.random.RandomState((zlib.crc32(str(eid).encode("utf-8")) + slot) % 2 ** 32).choice(pool, p=probs)
            assert m.available_modules[row[slot]] == want, (eid, slot)
            drawn.add(want.split("_")[0])
    assert drawn == ({"policy", "scripted", "champion"} if fixed != 0 else {"scripted", "champion"})


def test_command_lines():
    from gym_continuousdoubleauction_amd import league_train, ppo
    a = ppo.main(["--markets", "64", "--trained-slots", "2", "--opponent", "maker", "--opponent", "taker:p_trade_q32=1073741824"], parse_only=True)
    assert a.trained_slots == 2 and a.opponent == ["maker", "taker:p_trade_q32=1073741824"]
    d = ppo.main([], parse_only=True)
    assert d.trained_slots is None and d.opponent is None
    with pytest.raises(SystemExit):
        ppo.main(["--opponent", "maker"])                       # the two go together (refused before any device is touched)
    with pytest.raises(SystemExit):
        ppo.main(["--trained-slots", "1"])
    b = league_train.main(["--fused", "--scripted-opponent", "maker", "--scripted-opponent", "imbalance:depth_levels=3", "--scripted-weight", "2.5",
                                                "--random-opponents", "0"], parse_only=True)
    assert b.scripted_opponent == ["maker", "imbalance:depth_levels=3"] and b.scripted_weight == 2.5 and b.random_opponents == 0
    e = league_train.main(["--fused"], parse_only=True)
    assert e.scripted_opponent is None and e.scripted_weight == 1.0 and e.random_opponents is None
    with pytest.raises(SystemExit):
        league_train.main(["--scripted-opponent", "maker"])    # needs --fused


def test_canonical_checkpoint_arguments():
    from gym_continuousdoubleauction_amd import checkpoint as CK, scripted as S
    base = {"markets": 48, "seed": 0}
    assert CK.with_scripted(base, []) == base and CK.with_scripted(base, None, trained_slots=2) == base     # no scripts: the arguments a run always had
    a = CK.with_scripted(base, ["maker", "taker:p_trade_q32=1073741824"], trained_slots=2)
    b = CK.with_scripted(base, [S.NAMED["maker"], "taker"], trained_slots=2)                                # the named taker's default IS 2^30: the same profile
    assert a == b and a["trained_slots"] == 2 and "scripted_weight" not in a
    rec = a["scripted_opponents"]
    assert [r["law"] for r in rec] == [S.LAW_MAKER, S.LAW_TAKER] and rec[1]["p_trade_q32"] == 1 << 30
    assert set(rec[0]) == {"law", "size_mean", "size_sigma", "max_position", "skew_position", "max_orders", "depth_levels", "imb_num", "imb_den", "p_trade_q32"}
    assert rec[0]["size_mean"] == float(np.float32(0.05)) and all(type(v) in (int, float) for r in rec for v in r.values())
    CK.check_args(a, b)
    for other in (CK.with_scripted(base, ["taker", "maker"], trained_slots=2), CK.with_scripted(base, ["maker"], trained_slots=2),
                  CK.with_scripted(base, ["maker", "taker:max_position=7"], trained_slots=2), base):
        with pytest.raises(ValueError, match="scripted_opponents"):
            CK.check_args(a, other)
    with pytest.raises(ValueError, match="trained_slots"):
        CK.check_args(a, CK.with_scripted(base, ["maker", "taker"], trained_slots=1))
    lg = CK.with_scripted(base, ["maker"], scripted_weight=2.5)
    assert lg["scripted_weight"] == 2.5 and "trained_slots" not in lg
    with pytest.raises(ValueError, match="scripted_weight"):
        CK.check_args(lg, CK.with_scripted(base, ["maker"], scripted_weight=1.0))
    assert S.module_id(3, S.parse_profile("imbalance")) == "scripted_3_imbalance"


def test_opponent_placement():
    from gym_continuousdoubleauction_amd import scripted as S
    sl = S.opponent_slots(5, 4, 2, 3)
    assert sl.dtype == np.int32 and (sl[:, :2] == 0).all()
    for m in range(5):
        for j in range(2):
            assert sl[m, 2 + j] == 1 + (m + j) % 3
    for k in (0, 4, -1, 9):
        with pytest.raises(ValueError, match="trained_slots"):
            S.opponent_slots(5, 4, k, 3)


class _Env:
    """what the loops look at before they touch a device"""

    def __init__(self, slots=None, n=6, a=4):
        self.n_markets, self.num_agents = n, a
        self._slots = slots
        self.attached = self.cleared = 0

    @property
    def scripted(self):
        return self._slots is not None

    def scripted_slots(self):
        return self._slots if self._slots is not None else np.zeros((self.n_markets, self.num_agents), np.int32)

    def set_scripted(self, *a, **kw):
        self.attached += 1
        raise AssertionError("must be refused before anything is attached")


def test_refusals_that_need_no_device():
    from gym_continuousdoubleauction_amd import league_train, ppo
    from gym_continuousdoubleauction_amd.mlp import check_trained_slots
    good = np.array([[0, 0, 1, 2]] * 6, np.int32)
    check_trained_slots(good, 2)
    below, hole = good.copy(), good.copy()
    below[3, 1] = 1
    hole[4, 3] = 0
    with pytest.raises(ValueError, match="trained slot"):
        check_trained_slots(below, 2)
    with pytest.raises(ValueError, match="not scripted"):
        check_trained_slots(hole, 2)
    for k in (0, 4):
        with pytest.raises(ValueError, match="trained_slots"):
            check_trained_slots(good, k)
    quiet = dict(iters=1, log=lambda *_: None)
    # the shared loop: the caller's own scripts with a bad placement, no slot count, a data-parallel run
    with pytest.raises(ValueError, match="scripted"):
        ppo.train_fused(_Env(good), **quiet)                                      # (as before this feature: tests/test_hip_scripted.py)
    with pytest.raises(ValueError, match="trained slot"):
        ppo.train_fused(_Env(below), trained_slots=2, **quiet)
    with pytest.raises(ValueError, match="not scripted"):
        ppo.train_fused(_Env(hole), trained_slots=2, **quiet)
    with pytest.raises(ValueError, match="not scripted"):
        ppo.train_fused(_Env(None), trained_slots=2, **quiet)                     # nothing attached at all
    with pytest.raises(ValueError, match="trained_slots"):
        ppo.train_fused(_Env(good), trained_slots=4, **quiet)
    with pytest.raises(ValueError, match="data-parallel"):
        ppo.train_fused(_Env(good), trained_slots=2, world=2, allreduce=lambda t: t, **quiet)
    # ... and with opponents=
    for kw, what in ((dict(trained_slots=0), "trained_slots"), (dict(trained_slots=4), "trained_slots"), (dict(), "trained_slots"),
                     (dict(trained_slots=2, world=2, allreduce=lambda t: t), "data-parallel")):
        env = _Env(None)
        with pytest.raises(ValueError, match=what):
            ppo.train_fused(env, opponents=["maker"], **dict(quiet, **kw))
        assert env.attached == 0
    with pytest.raises(ValueError, match="unknown scripted opponent"):
        ppo.train_fused(_Env(None), opponents=["market_maker"], trained_slots=2, **quiet)
    with pytest.raises(ValueError, match="non-empty"):
        ppo.train_fused(_Env(None), opponents=[], trained_slots=2, **quiet)
    with pytest.raises(ValueError, match="scripted"):
        ppo.train_fused(_Env(good), opponents=["maker"], trained_slots=2, **quiet)
    # the league
    with pytest.raises(ValueError, match="scripted"):
        league_train.train_league_fused(_Env(good), **quiet)
    with pytest.raises(ValueError, match="scripted"):
        league_train.train_league_fused(_Env(good), scripted_opponents=["maker"], **quiet)
    for kw, what in ((dict(world=2, allreduce=lambda t: t), "data-parallel"), (dict(num_trainable=4), "num_trainable"), (dict(scripted_opponents=[]), "non-empty"),
                     (dict(scripted_opponents=["maker:law=2"]), "bad field"), (dict(scripted_opponents=["pass"] * 17), "at most")):
        env = _Env(None)
        with pytest.raises(ValueError, match=what):
            league_train.train_league_fused(env, **dict(dict(quiet, scripted_opponents=["maker"]), **kw))
        assert env.attached == 0


def test_mapper_refuses_a_device_assignment_without_the_slot_table():
    class _Bank:
        device = "cpu"
        slot_net = np.zeros((5, 8), np.int32)
    m, _ = _mapper()
    with pytest.raises(ValueError, match="slot_script"):
        m.assign_device(_Bank(), episode_ids=[f"e{i}" for i in range(5)])


@pytest.fixture(scope="module")
def hip_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_hip()
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib(), _lib


def test_new_entry_points_load_with_their_prototypes(hip_lib):
    """both symbols: declared in the learner-side header (include/cda_learner.h: one copy in the library, so in no rename list), bound with argtypes; NULL pointers
    and out-of-range sizes are CDA_ERR_INVALID before anything is launched (no GPU needed)"""
    import re
    L, _lib = hip_lib
    INVALID = -1
    hdr = open(os.path.join(ROOT, "include", "cda_learner.h")).read()
    var = open(os.path.join(ROOT, "gym_continuousdoubleauction_amd", "csrc", "cda_mlp_variant.h")).read()
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    protos = {"cda_gae_records_slots": [vp, vp, vp, vp, i32, i64, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp],
              "cda_league_assign_scripted": [vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp]}
    one = C.c_void_p(64)                                          # non-NULL, never dereferenced: the size checks fail first
    for name, argtypes in protos.items():
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, flags=re.M) and name not in var and name in _lib.LEARNER_SYMBOLS and name not in _lib.MLP_SYMBOLS
        n_args = len(re.search(r"^int\s+%s\s*\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1).split(","))
        assert n_args == len(argtypes)
        fn = getattr(L, name)
        assert list(fn.argtypes) == argtypes and fn.restype is C.c_int, name
        assert fn(*[None if t is vp else (0.0 if t is f32 else 0) for t in argtypes]) == INVALID, name
    gs = L.cda_gae_records_slots
    call = lambda T=8, N=8, A=4, k=2, rec=one, fin_index=None, fin_value=None: gs(one, one, one, one, T, N, A, k, 1.0, 0.99, 0.95, fin_index, fin_value, rec, one, None)   # noqa: E731
    assert call(k=0) == INVALID and call(k=5) == INVALID and call(T=0) == INVALID and call(N=0) == INVALID and call(A=17, k=1) == INVALID
    assert call(rec=None) == INVALID and call(fin_index=one) == INVALID and call(rec=C.c_void_p(68)) == INVALID
    asg = L.cda_league_assign_scripted
    acall = lambda N=8, A=4, k=2, P=3, script=one, slot_script=one: asg(one, N, A, k, one, one, script, P, one, slot_script, None, None)   # noqa: E731
    assert acall(P=0) == INVALID and acall(N=0) == INVALID and acall(A=17) == INVALID and acall(k=5) == INVALID and acall(k=-1) == INVALID
    assert acall(script=None) == INVALID and acall(slot_script=None) == INVALID
