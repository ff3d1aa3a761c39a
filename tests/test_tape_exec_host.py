"""CPU: the host statement of the tape's execution report (tape.exec_from_records: per-agent inventory, turnover and mark-outs - the specification of
CDAVecEnv.tape_exec) against a deliberately naive step-by-step loop over plain ints on the nine reference tapes tests/golden/tape_*.npz and on hand-written tapes
whose answers are written out below; the fold over modules and the ratios (tape.exec_by_module, tape.exec_summary); the share of fills the mark-outs of the GPU
parity test actually score; and the resources of the device kernel read from the built code object (the method of tests/test_tape_kernels.py)."""
import os

import numpy as np
import pytest

import golden_util as G
from test_tape_kernels import needs_tools
from test_kernel_resources import _kernels

FIXTURES = ["A16_aggr_s71", "A8_s3", "aggr_s23", "bankrupt_s61", "bigbook8_waves_s203", "perm8_s92", "permshuf_s93", "reset_s51", "tick5_s301"]
HORIZONS = (0, 1, 5, 20)         # what tests/test_hip_tape_exec.py asks of the device on the same tapes
MIN_SCORED_SHARE = 0.90          # ... of the non-self fills at the shortest non-zero horizon: a mark-out test whose fills are all open checks nothing

BUY, SELL = 1, 2                 # the two low bits of sides_step: initiator bid / counterparty ask, and the other way round


def naive_exec(rows, agents, horizons):
    """One pass over the steps 0 .. S_last with plain ints: the fills of a step move the positions one by one, the step's close is its last print (or the close
    before it), the position at the end of every step is written down; mark-outs are then looked up in the list of closes."""
    rows = [[int(x) for x in r] for r in np.asarray(rows).reshape(-1, 8)]
    names = ("buy_qty", "sell_qty", "buy_notional", "sell_notional", "maker_qty", "maker_fills", "taker_qty", "taker_fills", "self_qty", "self_fills",
             "final_pos", "max_long", "max_short", "abs_pos_steps", "first_step", "last_step")
    st = [dict.fromkeys(names, 0) for _ in range(agents)]
    for s in st:
        s["first_step"] = s["last_step"] = -1
    marks = [[[[0, 0, 0, 0] for _ in range(2)] for _ in horizons] for _ in range(agents)]
    if rows:
        s_last = rows[-1][7] >> 2
        close, pos, k, last_price = [], [0] * agents, 0, None
        for t in range(s_last + 1):
            while k < len(rows) and rows[k][7] >> 2 == t:
                _, price, qty, counter, _, _, init, ss = rows[k]
                last_price = price
                k += 1
                if counter == init:
                    st[init]["self_qty"] += qty
                    st[init]["self_fills"] += 1
                    continue
                for who, side, role in ((counter, ss & 1, "maker"), (init, (ss >> 1) & 1, "taker")):
                    s = st[who]
                    s["buy_qty" if side == 0 else "sell_qty"] += qty
                    s["buy_notional" if side == 0 else "sell_notional"] += price * qty
                    s[role + "_qty"] += qty
                    s[role + "_fills"] += 1
                    pos[who] += qty if side == 0 else -qty
                    s["max_long"], s["max_short"] = max(s["max_long"], pos[who]), min(s["max_short"], pos[who])
                    if s["first_step"] < 0:
                        s["first_step"] = t
                    s["last_step"] = t
            close.append(last_price)
            for a in range(agents):
                st[a]["abs_pos_steps"] += abs(pos[a])
        assert k == len(rows)
        for a in range(agents):
            st[a]["final_pos"] = pos[a]
        for _, price, qty, counter, _, _, init, ss in rows:
            if counter == init:
                continue
            for h, kk in enumerate(horizons):
                due = (ss >> 2) + kk
                for who, side, role in ((counter, ss & 1, 0), (init, (ss >> 1) & 1, 1)):
                    if due > s_last:
                        marks[who][h][role][3] += 1
                    else:
                        marks[who][h][role][0] += (1 if side == 0 else -1) * (close[due] - price) * qty
                        marks[who][h][role][1] += qty
                        marks[who][h][role][2] += 1
    return np.array([[s[f] for f in names] for s in st], np.int64).reshape(agents, 16), np.array(marks, np.int64).reshape(agents, len(horizons), 2, 4)


def _episodes(name):
    with np.load(os.path.join(G.GOLD, f"tape_{name}.npz")) as z:
        rows, episode = z["rows"], z["episode"]
    return [rows[episode == e] for e in np.unique(episode)], int(G.load(name)["config"]["num_of_agents"])


@pytest.mark.parametrize("name", FIXTURES)
def test_the_restatement_equals_a_naive_loop_on_every_reference_tape(name):
    from gym_continuousdoubleauction_amd import tape as T
    assert T.STAT_FIELDS == ("buy_qty", "sell_qty", "buy_notional", "sell_notional", "maker_qty", "maker_fills", "taker_qty", "taker_fills", "self_qty", "self_fills",
                             "final_pos", "max_long", "max_short", "abs_pos_steps", "first_step", "last_step")
    episodes, agents = _episodes(name)
    for rows in episodes:
        cuts = [rows, rows[len(rows) // 3:], rows[:len(rows) // 2]] if len(rows) > 8 else [rows]      # (a tape whose head is lost; one that stops early)
        for r in cuts:
            stats, marks = T.exec_from_records(r, agents, HORIZONS)
            want_s, want_m = naive_exec(r, agents, HORIZONS)
            assert stats.dtype == np.int64 and marks.dtype == np.int64 and stats.shape == (agents, 16) and marks.shape == (agents, 4, 2, 4)
            assert np.array_equal(stats, want_s), (name, np.argwhere(stats != want_s)[:6])
            assert np.array_equal(marks, want_m), (name, np.argwhere(marks != want_m)[:6])
            # what must hold of any tape
            g = {f: stats[:, i] for i, f in enumerate(T.STAT_FIELDS)}
            assert np.array_equal(g["buy_qty"] - g["sell_qty"], g["final_pos"]) and int(g["final_pos"].sum()) == 0
            assert np.array_equal(g["buy_qty"] + g["sell_qty"], g["maker_qty"] + g["taker_qty"]) and int(g["maker_qty"].sum()) == int(g["taker_qty"].sum())
            flows = T.flows_from_records(r, agents)
            off = flows[:, :, 0].sum() - np.trace(flows[:, :, 0])
            assert int((g["maker_qty"] + g["taker_qty"]).sum()) == 2 * int(off) and np.array_equal(g["self_fills"], np.diagonal(flows[:, :, 2]))
            assert (g["max_long"] >= np.maximum(g["final_pos"], 0)).all() and (g["max_short"] <= np.minimum(g["final_pos"], 0)).all()
            assert np.array_equal(marks[:, :, :, 2] + marks[:, :, :, 3], np.broadcast_to(np.stack([g["maker_fills"], g["taker_fills"]], 1)[:, None, :], (agents, 4, 2)))
            assert not marks[:, 0, :, 3].any()                                          # horizon 0 marks at the step's own close: never open


def test_the_mark_outs_of_the_parity_fixtures_are_mostly_scored():
    """The GPU parity test replays every fixture and reads the episode the tape then holds as current: its last.  At the shortest non-zero horizon only the
    fills of the episode's last step(s) can be open."""
    from gym_continuousdoubleauction_amd import tape as T
    shortest = min(k for k in HORIZONS if k > 0)
    h = HORIZONS.index(shortest)
    for name in FIXTURES:
        episodes, agents = _episodes(name)
        _, marks = T.exec_from_records(episodes[-1], agents, HORIZONS)
        line = []
        for j, k in enumerate(HORIZONS):
            scored, opened = int(marks[:, j, 1, 2].sum()), int(marks[:, j, 1, 3].sum())      # every non-self fill has exactly one taker
            line.append(f"k={k}: {scored}/{scored + opened} = {scored / max(1, scored + opened):.3f}")
        print(f"{name}: scored share of non-self fills  " + "  ".join(line))
        scored, opened = int(marks[:, h, 1, 2].sum()), int(marks[:, h, 1, 3].sum())
        assert scored + opened > 0 and scored >= MIN_SCORED_SHARE * (scored + opened), (name, scored, opened)


def _row(time, price, qty, counter, init, step, sides):
    return [time, price, qty, counter, 100 + time, -1, init, step << 2 | sides]


# agent 0 buys 5, sells 8 (crossing zero inside step 2, with two fills in that step), agent 1 is its counterparty, agent 2 trades with itself once and with agent
# 1 in the last step (6), agent 3 never trades.  Closes by step: 50, 50, 47, 47, 47, 55, 60.
HAND = np.array([
    _row(1, 50, 5, 1, 0, 0, BUY),      # step 0: 0 buys 5 from 1 at 50            pos0 = +5, pos1 = -5
    _row(2, 48, 3, 1, 0, 2, SELL),     # step 2: 0 sells 3 to 1 (1 rests as bid)  pos0 = +2, pos1 = -2
    _row(3, 47, 5, 0, 1, 2, BUY),      # step 2: 1 buys 5 from 0 (0 rests as ask) pos0 = -3, pos1 = +3
    _row(4, 55, 4, 2, 2, 5, BUY),      # step 5: 2 trades with itself
    _row(5, 60, 2, 1, 2, 6, BUY),      # step 6: 2 buys 2 from 1 at 60            pos2 = +2, pos1 = +1
], np.int32)


def test_a_hand_written_tape():
    from gym_continuousdoubleauction_amd import tape as T
    stats, marks = T.exec_from_records(HAND, 4, (0, 1, 4, 5))
    g = {f: stats[:, i].tolist() for i, f in enumerate(T.STAT_FIELDS)}
    assert g["buy_qty"] == [5, 8, 2, 0] and g["sell_qty"] == [8, 7, 0, 0]
    assert g["buy_notional"] == [250, 48 * 3 + 47 * 5, 120, 0] and g["sell_notional"] == [48 * 3 + 47 * 5, 250 + 120, 0, 0]
    assert g["maker_qty"] == [5, 5 + 3 + 2, 0, 0] and g["maker_fills"] == [1, 3, 0, 0] and g["taker_qty"] == [8, 5, 2, 0] and g["taker_fills"] == [2, 1, 1, 0]
    assert g["self_qty"] == [0, 0, 4, 0] and g["self_fills"] == [0, 0, 1, 0]
    assert g["final_pos"] == [-3, 1, 2, 0] and g["max_long"] == [5, 3, 2, 0] and g["max_short"] == [-3, -5, 0, 0]
    # |position| at the end of the steps 0 .. 6; the +2 that agent 0 held between its two fills of step 2 is never weighted
    assert g["abs_pos_steps"] == [5 + 5 + 3 + 3 + 3 + 3 + 3, 5 + 5 + 3 + 3 + 3 + 3 + 1, 2, 0]
    assert g["first_step"] == [0, 0, 6, -1] and g["last_step"] == [2, 6, 6, -1]
    assert not stats[3, :14].any() and not marks[3].any()                               # the agent without fills
    # k = 0: the step's own close (step 2 closes at 47, so the fill at 48 is marked against 47)
    assert marks[0, 0].tolist() == [[0, 5, 1, 0], [(50 - 50) * 5 - (47 - 48) * 3, 8, 2, 0]]
    assert marks[1, 0].tolist() == [[-(50 - 50) * 5 + (47 - 48) * 3 + 0, 10, 3, 0], [0, 5, 1, 0]]
    # k = 1: the fills of step 6 are open; step 1 has no print of its own and closes at 50, step 3 at 47
    assert marks[0, 1].tolist() == [[-(47 - 47) * 5, 5, 1, 0], [(50 - 50) * 5 - (47 - 48) * 3, 8, 2, 0]]
    assert marks[1, 1].tolist() == [[-(50 - 50) * 5 + (47 - 48) * 3, 8, 2, 1], [(47 - 47) * 5, 5, 1, 0]]
    assert marks[2, 1].tolist() == [[0, 0, 0, 0], [0, 0, 0, 1]]
    # k = 4: a fill of step 2 lands exactly on S_last = 6 and is marked at 60; k = 5 is one past it
    assert marks[0, 2].tolist() == [[-(60 - 47) * 5, 5, 1, 0], [(47 - 50) * 5 - (60 - 48) * 3, 8, 2, 0]]
    assert marks[0, 3].tolist() == [[0, 0, 0, 1], [(55 - 50) * 5, 5, 1, 1]]
    assert marks[1, 2].tolist() == [[-(47 - 50) * 5 + (60 - 48) * 3, 8, 2, 1], [(60 - 47) * 5, 5, 1, 0]]
    want_s, want_m = naive_exec(HAND, 4, (0, 1, 4, 5))
    assert np.array_equal(stats, want_s) and np.array_equal(marks, want_m)
    # an empty tape; bad arguments
    stats, marks = T.exec_from_records(np.zeros((0, 8), np.int32), 3, (1,))
    assert stats.tolist() == [[0] * 14 + [-1, -1]] * 3 and marks.shape == (3, 1, 2, 4) and not marks.any()
    for bad in ((), (-1,), tuple(range(9))):
        with pytest.raises(ValueError):
            T.exec_from_records(HAND, 4, bad)
    with pytest.raises(ValueError):
        T.exec_from_records(HAND, 2, (1,))                                              # agent 2 trades on this tape
    with pytest.raises(ValueError):
        T.exec_from_records(HAND[::-1], 4, (1,))                                        # not in tape order


def test_the_fold_over_modules_and_the_ratios():
    import torch
    from gym_continuousdoubleauction_amd import tape as T
    hz = (0, 1, 4)
    a = T.exec_from_records(HAND, 4, hz)
    b = T.exec_from_records(HAND[:3], 4, hz)
    stats, marks = torch.from_numpy(np.stack([a[0], b[0]])), torch.from_numpy(np.stack([a[1], b[1]]))
    slot_module = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 2]], dtype=torch.int32)          # module 3 plays nowhere
    st, mk = T.exec_by_module(stats, marks, slot_module, 4)
    assert st.dtype == torch.int64 and tuple(st.shape) == (4, 16) and tuple(mk.shape) == (4, 3, 2, 4)
    rows = {0: [(0, 0), (1, 1)], 1: [(0, 1), (0, 2), (1, 0)], 2: [(0, 3), (1, 2), (1, 3)], 3: []}
    s, m = stats.numpy(), marks.numpy()
    for mod, members in rows.items():
        want = np.zeros(16, np.int64)
        want[14:] = -1
        wm = np.zeros((3, 2, 4), np.int64)
        for i, x in members:
            for f in T.STAT_ADDITIVE:
                want[T.STAT[f]] += s[i, x, T.STAT[f]]
            want[T.STAT["max_long"]] = max(want[T.STAT["max_long"]], s[i, x, T.STAT["max_long"]])
            want[T.STAT["max_short"]] = min(want[T.STAT["max_short"]], s[i, x, T.STAT["max_short"]])
            want[T.STAT["last_step"]] = max(want[T.STAT["last_step"]], s[i, x, T.STAT["last_step"]])
            if s[i, x, T.STAT["first_step"]] >= 0:
                want[T.STAT["first_step"]] = s[i, x, T.STAT["first_step"]] if want[T.STAT["first_step"]] < 0 else min(want[T.STAT["first_step"]], s[i, x, T.STAT["first_step"]])
            wm += m[i, x]
        assert st[mod].tolist() == want.tolist(), (mod, st[mod].tolist(), want.tolist())
        assert np.array_equal(mk[mod].numpy(), wm), mod
    assert st[2].tolist()[14:] == [-1, -1] and st[3].tolist() == [0] * 14 + [-1, -1]      # slots that never traded; a module without slots
    with pytest.raises(ValueError):
        T.exec_by_module(stats, marks, slot_module, 2)
    with pytest.raises(ValueError):
        T.exec_by_module(stats, marks[:, :3], slot_module, 4)
    # the ratios of agent 0 of the hand-written tape
    r = T.exec_summary(a[0][0], a[1][0], horizons=hz, steps=7)
    assert r["buy_vwap"] == 50.0 and r["sell_vwap"] == (48 * 3 + 47 * 5) / 8 and r["turnover"] == 13 and r["turnover_notional"] == 250 + 144 + 235 and r["fills"] == 3
    assert r["maker_share"] == 5 / 13 and r["final_pos"] == -3 and r["max_long"] == 5 and r["max_short"] == -3 and r["mean_abs_position"] == 25 / 7
    assert r["markouts"]["k4"]["maker"] == {"pnl": -65, "qty": 5, "fills": 1, "open_fills": 0, "pnl_per_share": -13.0, "coverage": 1.0}
    assert r["markouts"]["k4"]["taker"]["pnl_per_share"] == (-15 - 36) / 8
    # nothing divides by zero: the agent without fills, and a row whose every mark-out is open
    r = T.exec_summary(a[0][3], a[1][3])
    assert r["buy_vwap"] is None and r["sell_vwap"] is None and r["maker_share"] is None and r["mean_abs_position"] is None and r["turnover"] == 0
    assert r["markouts"][0]["maker"] == {"pnl": 0, "qty": 0, "fills": 0, "open_fills": 0, "pnl_per_share": None, "coverage": None}
    r = T.exec_summary(*(x[2] for x in T.exec_from_records(HAND, 4, (1,))), horizons=(1,))
    assert r["markouts"]["k1"]["taker"] == {"pnl": 0, "qty": 0, "fills": 0, "open_fills": 1, "pnl_per_share": None, "coverage": 0.0} and r["buy_vwap"] == 60.0
    r = T.exec_summary(st[1], mk[1], horizons=hz, steps=21)                               # ... and a module's row, as tensors
    assert r["turnover"] == int(st[1, 0] + st[1, 1]) and r["mean_abs_position"] == int(st[1, 13]) / 21
    with pytest.raises(ValueError):
        T.exec_summary(a[0], a[1])


@needs_tools
def test_the_exec_kernel_exists_once_and_keeps_everything_in_registers_and_lds():
    ks, bodies = _kernels()
    inst = {n: v for n, v in ks.items() if "k_tape_exec" in n}
    assert len(inst) == 1, sorted(inst)
    (n, v), = inst.items()
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 128, (n, v)
    body = bodies[n]
    assert not any("scratch_" in l for l in body), n
    assert not any("global_atomic" in l or "flat_atomic" in l for l in body), n          # nothing depends on scheduling
    assert any("ds_add_u64" in l for l in body) and any("ds_max_i64" in l for l in body) and any("ds_min_i64" in l for l in body), n
    assert sum("global_load_dword" in l for l in body) >= 3                               # the record's two words and the probes of the mark search
    assert not any(l.split()[0].startswith("s_") and "store" in l.split()[0] for l in body if l.split()), n      # plain vector stores only
    # the instances that existed before are all still there, as many as before
    for stem, count in (("k_stepILb", 8), ("k_tstepILb", 4), ("k_policy_step", 14), ("k_tape_bars", 1), ("k_tape_flows", 1), ("k_tape_run", 2), ("k_tape_last", 1),
                        ("k_tape_pack", 1), ("k_tape_offsets", 1)):
        assert len([x for x in ks if stem in x]) == count, (stem, sorted(x for x in ks if stem in x))
