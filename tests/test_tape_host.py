"""CPU: the trade tape's host side (gym_continuousdoubleauction_amd/tape.py) against the fixtures cut from the reference (tests/golden/tape_*.npz), and the
C-ABI's declarations.  No GPU."""
import glob
import os
import re
from decimal import Decimal

import numpy as np
import pytest

from gym_continuousdoubleauction_amd import tape as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "tape_*.npz")))
ENTRY_POINTS = ["cda_tape_enable", "cda_tape_capacity", "cda_tape_counts", "cda_tape_offsets", "cda_tape_pack", "cda_tape_last"]


def _load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_the_fixtures_the_issue_names_are_there():
    names = {os.path.basename(p)[len("tape_"):-4] for p in FIXTURES}
    assert {"aggr_s23", "A8_s3", "tick5_s301", "A16_aggr_s71", "reset_s51", "bankrupt_s61", "bigbook8_waves_s203"} <= names
    assert names & {"permshuf_s93", "perm8_s92", "perm_s91", "permshuf8_s94"}
    fills = {os.path.basename(p)[len("tape_"):-4]: len(_load(p)["rows"]) for p in FIXTURES}
    assert (fills["aggr_s23"], fills["A8_s3"], fills["tick5_s301"], fills["A16_aggr_s71"]) == (353, 527, 182, 895)
    for p in FIXTURES:
        assert os.path.getsize(p) < 1 << 20


def test_record_dtype_is_the_eight_words_of_the_header():
    assert TP.RECORD_DTYPE.itemsize == 32 and TP.TAPE_WORDS == 8
    hdr = open(os.path.join(ROOT, "include", "cda.h")).read()
    body = re.search(r"typedef struct cda_tape_record \{(.*?)\} cda_tape_record;", hdr, re.S).group(1)
    assert tuple(re.findall(r"int32_t (\w+);", body)) == TP.FIELDS
    assert "#define CDA_TAPE_WORDS   8" in hdr
    rows = np.arange(16, dtype=np.int32).reshape(2, 8)
    rec = TP.as_records(rows)
    assert rec["time"].tolist() == [0, 8] and rec["sides_step"].tolist() == [7, 15] and rec["counter_left"].tolist() == [5, 13]
    assert np.array_equal(TP.as_rows(rec), rows)
    with pytest.raises(ValueError):
        TP.as_rows(np.zeros((3, 7), np.int32))


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_reference_records_against_the_reference_s_own_repr(path):
    fx = _load(path)
    rows = fx["rows"]
    recs = TP.to_reference_records(rows)
    assert len(recs) == len(rows) and len(fx["repr_idx"]) > 0
    for i, s in zip(fx["repr_idx"], fx["repr"]):
        ref = eval(str(s), {"Decimal": Decimal, "np": np, "__builtins__": {}})
        got = recs[int(i)]
        assert got == ref, (i, got, ref)
        # the reference's value types: Decimal prices, Decimal or None left-overs, nothing on the initiating side
        assert isinstance(got["price"], Decimal) and isinstance(ref["price"], Decimal)
        assert (got["counter_party"]["new_book_quantity"] is None) == (ref["counter_party"]["new_book_quantity"] is None)
        if ref["counter_party"]["new_book_quantity"] is not None:
            assert isinstance(got["counter_party"]["new_book_quantity"], Decimal) and isinstance(ref["counter_party"]["new_book_quantity"], Decimal)
        assert got["init_party"]["order_id"] is None and got["init_party"]["new_book_quantity"] is None
        assert list(got) == list(ref) and list(got["counter_party"]) == list(ref["counter_party"])      # same keys, same order
    # the packed word: sides and the step index
    assert np.array_equal(TP.pack_sides_step(TP.counter_side(rows), TP.init_side(rows), TP.step_index(rows)), rows[:, 7])
    assert np.array_equal(TP.counter_side(rows) ^ 1, TP.init_side(rows))                 # a fill crosses the book
    assert (np.diff(TP.step_index(rows)[fx["episode"] == 0]) >= 0).all()
    assert np.array_equal(fx["tape_len"][-1:], [int((fx["episode"] == fx["episode"].max()).sum())] if len(rows) else [0])


def test_npz_round_trip(tmp_path):
    fx = _load(os.path.join(GOLD, "tape_reset_s51.npz"))
    rows = fx["rows"]
    off = np.array([0, 40, len(rows)], np.int64)
    path = str(tmp_path / "t.npz")
    TP.save_tape(path, rows, offsets=off, dropped=np.zeros(2, np.int64), episode=fx["episode"], module=np.array([3, 5], np.int32))
    back = TP.load_tape(path)
    assert np.array_equal(back["records"], rows) and back["records"].dtype == np.int32
    assert np.array_equal(back["offsets"], off) and np.array_equal(back["episode"], fx["episode"]) and back["module"].tolist() == [3, 5]
    assert np.array_equal(back["market"], np.repeat([0, 1], [40, len(rows) - 40])) and tuple(back["fields"]) == TP.FIELDS
    assert TP.to_reference_records(back["records"]) == TP.to_reference_records(rows)


def test_entry_points_are_declared_bound_and_exported():
    import subprocess
    import __graft_entry__ as G
    from gym_continuousdoubleauction_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cda.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|int64_t) %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS
    so = G.build_hip()
    nm = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(r" T %s$" % name, nm, re.M), name
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert getattr(L, name).argtypes, name
