"""CPU: the host statement of the tape's two reductions (tape.bars_from_records, tape.flows_from_records) on a hand-written tape whose bars and flows are
written out literally below, their invariants on the nine reference tapes tests/golden/tape_*.npz, and the resources of the two device kernels read from the
built code object (the method of tests/test_tape_kernels.py)."""
import os

import numpy as np
import pytest

import golden_util as G
from test_tape_kernels import needs_tools
from test_kernel_resources import _kernels

FIXTURES = ["A16_aggr_s71", "A8_s3", "aggr_s23", "bankrupt_s61", "bigbook8_waves_s203", "perm8_s92", "permshuf_s93", "reset_s51", "tick5_s301"]
SELF_TRADES = [60, 53, 95, 7, 406, 34, 36, 22, 36]

BUY, SELL = 1, 2                 # the two low bits of sides_step: initiator bid / counterparty ask, and the other way round


def _row(time, price, qty, counter, init, step, sides):
    return [time, price, qty, counter, 100 + time, -1, init, step << 2 | sides]


# twelve fills, bars of two steps: bar 0 = steps 0, 1 (two fills in step 0), bar 1 = steps 2, 3 (one self-trade), bar 2 empty, bar 3 = steps 6, 7, and two fills
# in steps 8 and 9 that four bars do not cover
HAND = np.array([
    _row(1, 50, 3, 1, 0, 0, BUY),
    _row(2, 52, 2, 2, 0, 0, BUY),
    _row(3, 49, 5, 0, 3, 1, SELL),
    _row(4, 51, 4, 2, 2, 2, BUY),
    _row(5, 51, 1, 1, 3, 3, SELL),
    _row(6, 60, 2, 0, 1, 6, BUY),
    _row(7, 58, 7, 3, 1, 6, BUY),
    _row(8, 61, 1, 1, 0, 7, SELL),
    _row(9, 57, 2, 2, 0, 7, SELL),
    _row(10, 59, 3, 1, 1, 7, BUY),
    _row(11, 70, 1, 0, 2, 8, BUY),
    _row(12, 71, 2, 3, 2, 9, SELL),
], np.int32)
# open, high, low, close, n_trades, n_self, volume, buy_volume, notional
HAND_BARS = [(50, 52, 49, 49, 3, 0, 10, 5, 50 * 3 + 52 * 2 + 49 * 5),
             (51, 51, 51, 51, 2, 1, 5, 4, 51 * 4 + 51 * 1),
             (0, 0, 0, 0, 0, 0, 0, 0, 0),
             (60, 61, 57, 59, 5, 1, 15, 12, 60 * 2 + 58 * 7 + 61 * 1 + 57 * 2 + 59 * 3)]
# (init_id, counter_id): (quantity, notional, fills)
HAND_FLOWS = {(0, 1): (4, 150 + 61, 2), (0, 2): (4, 104 + 114, 2), (3, 0): (5, 245, 1), (2, 2): (4, 204, 1), (3, 1): (1, 51, 1), (1, 0): (2, 120, 1),
              (1, 3): (7, 406, 1), (1, 1): (3, 177, 1), (2, 0): (1, 70, 1), (2, 3): (2, 142, 1)}


def test_bars_and_flows_of_a_hand_written_tape():
    from gym_continuousdoubleauction_amd import tape as T
    bars, beyond = T.bars_from_records(HAND, 2, 4)
    assert bars.dtype == T.BAR_DTYPE and bars.shape == (4,) and beyond == 2
    assert bars.tolist() == HAND_BARS
    # the twelve int32 words of a bar, as the device writes them, carry the same structure
    words = bars.view(np.int32).reshape(4, 12)
    assert np.array_equal(T.as_bars(words), bars) and words[0].tolist() == [50, 52, 49, 49, 3, 0, 10, 0, 5, 0, 499, 0]
    # one more bar takes in steps 8 and 9
    bars5, beyond5 = T.bars_from_records(HAND, 2, 5)
    assert beyond5 == 0 and bars5[:4].tolist() == HAND_BARS and bars5[4].tolist() == (70, 71, 70, 71, 2, 0, 3, 1, 70 + 142)
    # one bar over everything
    one, _ = T.bars_from_records(HAND, 16, 1)
    assert one[0].tolist() == (50, 71, 49, 71, 12, 2, 33, 22, int((HAND[:, 1].astype(np.int64) * HAND[:, 2]).sum()))
    flows = T.flows_from_records(HAND, 4)
    want = np.zeros((4, 4, 3), np.int64)
    for (i, c), v in HAND_FLOWS.items():
        want[i, c] = v
    assert flows.dtype == np.int64 and np.array_equal(flows, want)
    assert int(np.trace(flows[:, :, 2])) == 2 and int(flows[:, :, 0].sum()) == 33
    for bad in ((0, 4), (2, 0)):
        with pytest.raises(ValueError):
            T.bars_from_records(HAND, *bad)
    with pytest.raises(ValueError):
        T.flows_from_records(HAND, 3)                      # agent 3 trades on this tape
    empty, n = T.bars_from_records(np.zeros((0, 8), np.int32), 3, 2)
    assert n == 0 and empty.tolist() == [(0,) * 9] * 2 and int(T.flows_from_records(np.zeros((0, 8), np.int32), 2).sum()) == 0


@pytest.mark.parametrize("name,n_self", list(zip(FIXTURES, SELF_TRADES)))
def test_invariants_on_the_reference_tapes(name, n_self):
    from gym_continuousdoubleauction_amd import tape as T
    with np.load(os.path.join(G.GOLD, f"tape_{name}.npz")) as z:
        rows, episode = z["rows"], z["episode"]
    cfg = G.load(name)["config"]
    agents, max_step = int(cfg["num_of_agents"]), int(cfg["max_step"])
    self_total = 0
    for ep in np.unique(episode):
        r = rows[episode == ep]
        assert (np.diff(r[:, 7] >> 2) >= 0).all() and (r[:, 7] >> 2).max() < max_step            # a bar is one run of records
        flows = T.flows_from_records(r, agents)
        self_total += int(np.trace(flows[:, :, 2]))
        for bar_steps in (1, 7, 64, max_step):
            n_bars = -(-max_step // bar_steps)
            bars, beyond = T.bars_from_records(r, bar_steps, n_bars)
            assert beyond == 0 and len(bars) == n_bars
            live = bars["n_trades"] > 0
            assert int(bars["volume"].sum()) == int(r[:, 2].astype(np.int64).sum()) and int(bars["n_trades"].sum()) == len(r)
            assert (bars["low"][live] <= bars["open"][live]).all() and (bars["open"][live] <= bars["high"][live]).all()
            assert (bars["low"][live] <= bars["close"][live]).all() and (bars["close"][live] <= bars["high"][live]).all()
            assert (bars["low"][live] > 0).all() and (bars["buy_volume"] <= bars["volume"]).all()
            assert not bars[~live].view(np.int32).any()
            # the flows add up to the bars
            assert int(flows[:, :, 0].sum()) == int(bars["volume"].sum()) and int(flows[:, :, 1].sum()) == int(bars["notional"].sum())
            assert int(flows[:, :, 2].sum()) == int(bars["n_trades"].sum()) and int(np.trace(flows[:, :, 2])) == int(bars["n_self"].sum())
        # fewer bars than the episode needs: the rest is counted, not folded in
        short, beyond = T.bars_from_records(r, 7, 3)
        assert beyond == int(((r[:, 7] >> 2) >= 21).sum()) and int(short["n_trades"].sum()) == len(r) - beyond
    assert self_total == n_self


@needs_tools
def test_the_bar_and_flow_kernels_exist_once_and_keep_everything_in_registers():
    ks, bodies = _kernels()
    for stem in ("k_tape_bars", "k_tape_flows"):
        inst = {n: v for n, v in ks.items() if stem in n}
        assert len(inst) == 1, (stem, sorted(inst))
        (n, v), = inst.items()
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (n, v)
        assert not any("scratch_" in l for l in bodies[n]), n
    bars, = [n for n in bodies if "k_tape_bars" in n]
    assert sum("global_store_dwordx4" in l for l in bodies[bars]) >= 3, bars                    # a bar is three 16-byte stores
    assert sum("global_load_dwordx" in l for l in bodies[bars]) >= 2                                # a record is two vector loads (narrowed to the words that are used)
    assert not any("global_atomic" in l or "flat_atomic" in l for l in bodies[bars])
    flows, = [n for n in bodies if "k_tape_flows" in n]
    assert any("ds_add_u64" in l for l in bodies[flows]) and not any("global_atomic" in l or "flat_atomic" in l for l in bodies[flows])
    # the tape's header stays 32 bytes per market with the remembered episode in it
    src = open(os.path.join(os.path.dirname(G.GOLD), "..", "gym_continuousdoubleauction_amd", "csrc", "cda_market.hpp")).read()
    assert "int32_t n_prev;" in src and 'static_assert(sizeof(TapeMeta) == 32, "TapeMeta layout");' in src
