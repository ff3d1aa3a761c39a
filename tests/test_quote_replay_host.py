"""CPU: tests/quote_replay.py QuoteReplay - the host replay the services fuzz holds the quote tape to - on one hand-worked life of a market on a ring of five
records: a reset, a restore that moves the clock forward, one that moves it back, a ring that wraps.  Every expected row, count, lost, step0 and partial below is
written out by hand from the episode rule's text (quotes.roll) and the ring's arithmetic (record j lies in slot j % 5: the ring holds the last five records)."""
import numpy as np

from gym_continuousdoubleauction_amd import quotes as Q
from quote_replay import QuoteReplay


def _row(j, t):
    """record number j, written at step t: recognisable words"""
    return [t, 3, 100 + j, 110 + j, 1 + j, 2 + j, 1, 1]


def _rows(pairs):
    return np.array([_row(j, t) for j, t in pairs], np.int32).reshape(-1, 8)


def _held(rp, episode):
    rows, count, lost, step0, partial = rp.held(0, episode)
    return rows.tolist(), (count, lost, step0, partial)


def test_one_life_of_a_market_on_a_ring_of_five_worked_by_hand():
    rp = QuoteReplay(2, 5)
    j = 0

    def run(steps):
        nonlocal j
        for t in steps:
            rp.visit(0, t, _row(j, t))
            j += 1
        rp.clock(0, steps[-1] + 1)

    # 1. three steps of a first episode: records 0 1 2
    run([0, 1, 2])
    assert _held(rp, "current") == (_rows([(0, 0), (1, 1), (2, 2)]).tolist(), (3, 0, 0, 0))
    assert _held(rp, "previous") == ([], (0, 0, 0, 0))
    # 2. a reset: the clock is at 0, nothing recorded yet - the readers roll: what was current is previous
    rp.clock(0, 0)
    assert _held(rp, "current") == ([], (0, 0, 0, 0))
    assert _held(rp, "previous") == (_rows([(0, 0), (1, 1), (2, 2)]).tolist(), (3, 0, 0, 0))
    assert rp.meta[0]["n_episode"] == 3 and rp.meta[0]["n_prev"] == 0      # (the roll is lazy: the stored row changes with the next visit)
    # 3. four steps of the second episode: records 3 .. 6; the ring of five holds records 2 .. 6, so the previous episode keeps its last record only
    run([0, 1, 2, 3])
    assert _held(rp, "current") == (_rows([(3, 0), (4, 1), (5, 2), (6, 3)]).tolist(), (4, 0, 0, 0))
    assert _held(rp, "previous") == (_rows([(2, 2)]).tolist(), (1, 2, 2, 0))
    # 4. a restore moves the clock forward, 4 -> 9: the current episode restarts there, empty and partial; its four records become a gap
    rp.clock(0, 9)
    assert _held(rp, "current") == ([], (0, 0, 9, 1))
    assert _held(rp, "previous") == (_rows([(2, 2)]).tolist(), (1, 2, 2, 0))
    assert rp.rolled(0) == {"n_total": 7, "n_episode": 0, "n_prev": 3, "first": 9, "prev_first": 0, "gap": 4, "flags": Q.PARTIAL}
    run([9, 10])                                               # records 7 8: the ring holds 4 .. 8, the previous episode (records 0 .. 2) is gone
    assert _held(rp, "current") == (_rows([(7, 9), (8, 10)]).tolist(), (2, 0, 9, 1))
    assert _held(rp, "previous") == ([], (0, 3, 3, 0))
    # 5. a restore moves the clock back, 11 -> 4: again a restart; the gap grows by the two records; six steps wrap the ring inside the episode
    rp.clock(0, 4)
    assert rp.rolled(0) == {"n_total": 9, "n_episode": 0, "n_prev": 3, "first": 4, "prev_first": 0, "gap": 6, "flags": Q.PARTIAL}
    run([4, 5, 6, 7, 8, 9])                                    # records 9 .. 14: the ring holds 10 .. 14 = the steps 5 .. 9; the record of step 4 is lost
    assert _held(rp, "current") == (_rows([(10, 5), (11, 6), (12, 7), (13, 8), (14, 9)]).tolist(), (5, 1, 5, 1))
    assert _held(rp, "previous") == ([], (0, 3, 3, 0))
    # 6. the reset behind it: the partial episode becomes the previous one, flag and all
    rp.clock(0, 0)
    assert _held(rp, "current") == ([], (0, 0, 0, 0))
    assert _held(rp, "previous") == (_rows([(10, 5), (11, 6), (12, 7), (13, 8), (14, 9)]).tolist(), (5, 1, 5, 1))
    assert rp.rolled(0) == {"n_total": 15, "n_episode": 0, "n_prev": 6, "first": 0, "prev_first": 4, "gap": 0, "flags": Q.PREV_PARTIAL}
    assert len(rp.records[0]) == 15 and [int(r[0]) for r in rp.records[0]] == [0, 1, 2, 0, 1, 2, 3, 9, 10, 4, 5, 6, 7, 8, 9]
    # the other market was never visited
    rows, *about = rp.held(1, "current")
    assert rows.shape == (0, 8) and about == [0, 0, 0, 0] and rp.rolled(1) == Q.new_meta()


def test_a_restore_onto_the_expected_step_is_no_restore():
    """the clock put where the recorder expects it anyway (first + n_episode): the rule cannot tell, and neither does the replay"""
    rp = QuoteReplay(1, 8)
    for t in range(3):
        rp.visit(0, t, _row(t, t))
    rp.clock(0, 3)
    before = rp.rolled(0)
    rp.clock(0, 3)                                             # "restored" to step 3
    assert rp.rolled(0) == before and rp.held(0)[1:] == (3, 0, 0, 0)
