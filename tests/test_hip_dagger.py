"""GPU: the label tap (csrc/cda_scripted_label.inc k_script_label; CDAVecEnv.set_label_tap / label_actions; the rollout chains; imitate.dagger) against the numpy
specification (scripted.actions_from_views / label_spec / mix_played), word for word.  The specification's views come from HOST dumps (get_book through book.py,
get_state) or from a replay of one market on the CPU oracle, never from the kernel under test.

Shapes: 23 markets (no multiple of the four waves of a workgroup), launches that start behind market 0, 1 / 2 / 5 / 16 agents, both tiles, ticks 1 and 5, and two
markets seeded with more orders per side than the tile holds - the ring is walked - whose orders 63 and 64 (the last lane of the first pass and the first of the
second) share a price wherever two agents exist to place them."""
import dataclasses

import numpy as np
import pytest
import torch

import oracle_lib as O
from gym_continuousdoubleauction_amd import _capi as K
from gym_continuousdoubleauction_amd import scripted as S
from test_hip_scripted import KEYS, MIXED, mixed_slots
from test_scripted_host import IMB, MAKER, PASS, TAKER, views_of_books

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 23
DEEP = (0, 1)                                                            # the seeded markets: tick 1 and tick 5
# the label laws: every law, depth_levels 1 / 4 / 10 side by side in every market, a taker that draws
LABELS = [dataclasses.replace(MAKER, max_position=30, skew_position=10, max_orders=3, size_mean=0.02, size_sigma=0.02),
          dataclasses.replace(IMB, depth_levels=1, imb_num=1, imb_den=1, max_position=25, size_mean=0.04, size_sigma=0.02),
          dataclasses.replace(IMB, depth_levels=10, imb_num=3, imb_den=2, max_position=60, size_mean=0.04, size_sigma=0.02),
          dataclasses.replace(TAKER, p_trade_q32=1 << 31, max_position=40, size_mean=0.05, size_sigma=0.05),
          dataclasses.replace(IMB, depth_levels=4, imb_num=1, imb_den=1, max_position=10 ** 6, size_mean=0.03, size_sigma=0.01),
          dataclasses.replace(MAKER, max_position=8, skew_position=0, max_orders=70, size_mean=0.03, size_sigma=0.0), PASS]


def tick_of(m):
    return 1 if m % 2 == 0 else 5


def deep_side(side, a, tick, count):
    """`count` resting orders of one side in queue order (best first), one per price except orders 63 and 64, which share one (two agents needed)"""
    rows, price = [], 2000 * tick if side == 0 else 2003 * tick
    for k in range(count):
        if not (k == 64 and a >= 2):
            price += -tick if side == 0 else tick
        rows.append((price, 1 + k % 3, k - 63 if k in (63, 64) and a >= 2 else k % a, k, k))                 # (orders 63, 64: agents 0 and 1)
    return np.array(rows, np.int32)


def build_env(a, tile, auto_reset=False, steps=30, seed=900):
    """23 markets at ticks 1 / 5; markets 0 and 1 seeded deep and left alone (no scripted slot there), the others played for `steps` steps by the mixed laws"""
    from gym_continuousdoubleauction_amd import CDAVecEnv
    cfg = {"num_of_agents": a, "init_cash": 10 ** 10, "max_step": 4096, "is_render": False, "book_capacity": tile, "auto_reset": auto_reset}
    env = CDAVecEnv(cfg, n_markets=N, device=DEV, with_info=False, market_configs=[{"tick_size": tick_of(i)} for i in range(N)])
    env.reset(seed=seed)
    count = env.book_capacity + 40
    for m in DEEP:
        _, summary = env.seed_books(deep_side(0, a, tick_of(m), count), deep_side(1, a, tick_of(m), count), market=m)
        assert summary.cpu().numpy()[0].tolist()[:3] == [2 * count, 0, 0], summary
    slots = mixed_slots(N, a)
    slots[list(DEEP)] = 0
    env.set_scripted(slots, MIXED, seed=77, market_index_base=1000)
    env.run_scripted(steps)                                              # (the unscripted slots pass: the seeded markets only move their clocks)
    books = [env.get_book(i) for i in range(N)]
    for m in DEEP:                                                       # the seeded books stand: beyond the tile, and (two agents) a level across the pass boundary
        for rows in books[m]:
            assert len(rows) == count > env.book_capacity and (a < 2 or rows[63][0] == rows[64][0]) and rows[62][0] != rows[63][0]
    assert sum(len(b) + len(s) for b, s in books[2:]) > 0
    return env, cfg


def label_table(a):
    m, j = np.meshgrid(np.arange(N), np.arange(a), indexing="ij")
    t = (1 + (m * 3 + j * 5 + m // 4) % len(LABELS)).astype(np.int32)
    t[(m + 2 * j) % 7 == 3] = 0                                          # ... and slots that are not labelled
    t[5] = 0                                                             # a market without a labelled slot
    for d in DEEP:                                                       # the deep markets: both imbalance depths and the 70-order maker wherever there is room
        t[d, :] = np.array([3, 2, 6, 5, 1, 4, 7, 3, 2, 6, 5, 1, 4, 7, 3, 2], np.int32)[:a]
    return t


def host_views(env, depth, markets=None):
    """the views of markets x agents from host dumps"""
    a = env.num_agents
    markets = range(env.n_markets) if markets is None else markets
    states = [env.get_state(i) for i in markets]
    return views_of_books([env.get_book(i) for i in markets], a, [[int(s.acc[j].net_position) for j in range(a)] for s in states], [int(s.t_step) for s in states],
                          [tick_of(i) for i in markets], depth)


def spec_labels(env, table, profiles, seed, counter, draw, base=0):
    pix = np.maximum(table - 1, 0)
    depth = np.array([p.depth_levels for p in profiles])[pix]
    m, j = np.meshgrid(np.arange(env.n_markets), np.arange(env.num_agents), indexing="ij")
    acts, labelled, _ = S.label_spec(profiles, table, host_views(env, depth), seed, counter, base + m, draw, j)
    return acts, labelled


def same_words(got, want, where, tag):
    for k, g, w in zip(KEYS, got, want):
        assert np.array_equal(np.ascontiguousarray(g[where]).view(np.uint32), np.ascontiguousarray(w[where]).view(np.uint32)), (tag, k, np.argwhere((g != w) & where)[:4])


def minus_seven(a):
    out = {k: torch.full((N, a), -7, dtype=torch.float32 if k in ("size_mean", "size_sigma") else torch.int32, device=DEV) for k in KEYS}
    return out


# ---- 1. label_actions against the specification ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,tile", [(1, 0), (2, 512), (5, 0), (16, 512), (16, 0)])
def test_label_actions_equal_the_specification(a, tile):
    env, _ = build_env(a, tile)
    table = label_table(a)
    assert {LABELS[v - 1].law for v in table[table > 0].tolist()} == set(S.LAWS.values()) and (table == 0).any()          # every law appears
    if a >= 2:                                                           # ... and profiles of different depth_levels within one market
        assert all(len({LABELS[v - 1].depth_levels for v in table[d].tolist()}) >= 2 for d in DEEP)
    (want, labelled) = spec_labels(env, table, LABELS, seed=41, counter=6, draw=9, base=500)
    out = env.label_actions(table, LABELS, seed=41, counter=6, draw=9, market_index_base=500, out=minus_seven(a))
    got = tuple(out[k].cpu().numpy() for k in KEYS)
    same_words(got, want, labelled, "whole range")
    for k, g in zip(KEYS, got):                                          # where the table is 0 nothing was written
        assert (g[~labelled] == -7).all(), k
    if a >= 5:                                                           # the laws do different things on these books, the deep ones included
        assert len(set(got[0][labelled].tolist())) >= 4 and len(set(got[0][list(DEEP)][labelled[list(DEEP)]].tolist())) >= 2
    # a launch that starts behind market 0 and ends before the last: the markets outside keep their bytes; the counter read on the device
    ctr = torch.tensor([6], dtype=torch.int64, device=DEV)
    part = env.label_actions(table, LABELS, seed=41, counter=ctr, draw=9, market_index_base=500, out=minus_seven(a), first_market=3, n_markets=17)
    inside = labelled.copy()
    inside[:3] = False; inside[20:] = False
    gp = tuple(part[k].cpu().numpy() for k in KEYS)
    same_words(gp, want, inside, "markets 3 .. 19")
    for k, g in zip(KEYS, gp):
        assert (g[~inside] == -7).all(), k
    # the env's own scripted slots and the markets are untouched: the state dumps are what they were
    assert (env.flags().cpu().numpy() == 0).all() and (env.check_invariants().cpu().numpy() == 0).all()
    env.close()


# ---- 2. a labelled slot against an attached slot ----------------------------------------------------------------------------------------------
def test_a_label_with_an_attached_slot_s_keys_is_that_slot_s_action():
    env, _ = build_env(5, 0)
    slots, profiles = env.scripted_slots(), env.scripted_profiles()
    assert any(p.law == S.LAW_TAKER for p in profiles)
    for draw, counter in ((30, 0), (31, 4)):
        mine = env.scripted_actions(draw=draw, counter=counter)
        lab = env.label_actions(slots, profiles, seed=77, counter=counter, draw=draw, market_index_base=1000, out=minus_seven(5))
        on = torch.from_numpy(slots != 0).to(DEV)
        for k in KEYS:
            assert torch.equal(mine[k][on].view(torch.int32), lab[k][on].view(torch.int32)), (k, draw)
    taker = torch.from_numpy(np.isin(slots, [1 + i for i, p in enumerate(profiles) if p.law == S.LAW_TAKER])).to(DEV)
    assert int((lab["category"][taker] != 0).sum()) > 0                  # the taker's draws among them
    env.close()


# ---- 3 .. 6: the tap inside the rollout chains --------------------------------------------------------------------------------------------------
A, LEARNER, T = 5, 2, 8
TAP_SEED, TAP_BASE = 91, 3000


def chain_env():
    """the env of build_env with auto_reset; slots 0, 1 are the policy's everywhere, slots 2 .. 4 scripted outside the deep markets"""
    env, cfg = build_env(A, 0, auto_reset=True)
    slots = env.scripted_slots().copy()
    slots[:, :LEARNER] = 0
    env.set_scripted(slots, MIXED, seed=13, market_index_base=64)
    return env, cfg


def tap_table(env):
    """the learner slots labelled (maker / taker by market), the deep markets' unscripted slots too, and some scripted slots labelled by ANOTHER law"""
    t = np.zeros((N, A), np.int32)
    t[:, 0] = 1
    t[:, 1] = np.where(np.arange(N) % 3 == 0, 4, 6)
    t[list(DEEP), 2:] = (3, 5, 2)
    t[2:, 3] = 2
    t[8:, 4] = 3
    assert ((t != 0) & (env.scripted_slots() != 0)).any() and ((t == 0) & (env.scripted_slots() != 0)).any()
    return t


def chains_on(env, seed=5):
    from gym_continuousdoubleauction_amd import mlp
    return mlp.RolloutChains(env, mlp.FusedPolicy(DEV, seed=1), T, groups=2, seed=seed)


def run_chain(env):
    ch = chains_on(env)
    b = {k: v.cpu().numpy() for k, v in ch.run().items()}
    torch.cuda.synchronize()
    return ch, b


def tap_host(env):
    return {k: env.label_tap[k].cpu().numpy() for k in KEYS + ("played",)}


ROLLOUT_KEYS = KEYS + ("a_cont", "logp", "record", "obs", "reward", "terminated", "truncated", "value")


def test_the_tap_is_a_reader(monkeypatch):
    monkeypatch.setenv("CDA_POLICY_STEP", "0")
    tapped, cfg = chain_env()
    table = tap_table(tapped)
    start = tapped.get_state(DEEP[1])                                    # the tick-5 deep market, before the rollout: what the host replay starts from
    tapped.set_label_tap(table, LABELS, rows=T, seed=TAP_SEED, market_index_base=TAP_BASE, mix=0.0)
    ch, b = run_chain(tapped)
    plain, _ = chain_env()
    _, b0 = run_chain(plain)
    for k in ROLLOUT_KEYS:                                               # every rollout buffer, bit for bit
        assert np.array_equal(b[k].view(np.uint8), b0[k].view(np.uint8)), k
    monkeypatch.delenv("CDA_POLICY_STEP")                                # ... and the no-tap twin under the default setting: the tap only turns the one-launch path off
    dflt, _ = chain_env()
    _, b1 = run_chain(dflt)
    for k in ROLLOUT_KEYS:
        assert np.array_equal(b1[k].view(np.uint8), b0[k].view(np.uint8)), ("default", k)
    tap = tap_host(tapped)
    labelled = table != 0
    assert (tap["played"][:, labelled] == 0).all() and (tap["played"] == 0).all()
    assert not (tap["category"][:, ~labelled] != 0).any()                # rows of unlabelled slots keep their zeros
    # the labels of every row: the specification on a host replay of the deep tick-5 market (the CPU oracle started from the market's state dump)
    m = DEEP[1]
    counter = int(ch.counter.item())
    ora = O.OracleEnv({"num_of_agents": A, "init_cash": cfg["init_cash"], "max_step": cfg["max_step"], "is_render": False, "tick_size": tick_of(m)}, n_markets=1)
    ora.reset(seeds=np.array([1], dtype=np.uint64))
    ora.set_state(0, start)
    pix = np.maximum(table[m] - 1, 0)[None, :]
    depth = np.array([p.depth_levels for p in LABELS])[pix]
    seen = set()
    for t in range(T):
        s = ora.get_state(0)
        views = views_of_books([ora.get_book(0)], A, [[int(s.acc[j].net_position) for j in range(A)]], [int(s.t_step)], [tick_of(m)], depth)
        want, lab, _ = S.label_spec(LABELS, table[m][None, :], views, TAP_SEED, counter, TAP_BASE + m, t, np.arange(A)[None, :])
        got = tuple(tap[k][t, m][None, :] for k in KEYS)
        same_words(got, want, lab, f"row {t}")
        seen |= set(want[0][lab].tolist())
        ora.step(*(b[k][t, m:m + 1] for k in KEYS))
    assert len(seen) >= 2
    # ... and row 0 of EVERY market: label_actions (which the first test holds to the specification) with the tap's keys on a fresh twin, whose state is the
    # one the rollout started from
    fresh, _ = chain_env()
    row0 = fresh.label_actions(table, LABELS, seed=TAP_SEED, counter=counter, draw=0, market_index_base=TAP_BASE)
    for k in KEYS:
        assert np.array_equal(tap[k][0][labelled].view(np.uint32), row0[k].cpu().numpy()[labelled].view(np.uint32)), k
    for e in (tapped, plain, dflt, fresh):
        assert (e.flags().cpu().numpy() == 0).all()
        e.close()
    ora.close()


def test_mixing(monkeypatch):
    monkeypatch.setenv("CDA_POLICY_STEP", "0")
    table_of = {}
    runs = {}
    for mix in (0.0, 1.0, 0.5):
        env, _ = chain_env()
        table_of[mix] = table = tap_table(env)
        env.set_label_tap(table, LABELS, rows=T + 2, seed=TAP_SEED, market_index_base=TAP_BASE, mix=mix)        # (more rows than steps: the rows behind stay zero)
        ch, b = run_chain(env)
        runs[mix] = (b, tap_host(env), int(ch.counter.item()))
        scripted = env.scripted_slots() != 0
        assert (env.flags().cpu().numpy() == 0).all() and (env.check_invariants().cpu().numpy() == 0).all()
        env.close()
    labelled = table != 0
    mixable, both = labelled & ~scripted, labelled & scripted
    assert mixable[:, :LEARNER].all() and mixable[list(DEEP)].all() and both.any()
    # mix = 1: every labelled, unscripted slot played its label at every row, as a scripted slot plays its law
    b, tap, counter = runs[1.0]
    assert (tap["played"][:T, mixable] == 1).all() and (tap["played"][:T, ~mixable] == 0).all() and (tap["played"][T:] == 0).all()
    for k in KEYS:
        assert np.array_equal(b[k][:, mixable].view(np.uint32), tap[k][:T, mixable].view(np.uint32)), k
    assert (b["logp"][:, mixable] == 0).all() and (b["a_cont"][:, mixable] == 0).all()
    rec = b["record"].view(np.int32)[:, mixable]
    assert np.array_equal(rec[..., 0], b["category"][:, mixable]) and np.array_equal(rec[..., 1], b["price"][:, mixable]) and (rec[..., 3:6] == 0).all()
    # a slot both scripted and labelled played its attached law: at row 0 what it plays in the mix = 0 twin
    b0, tap0, counter0 = runs[0.0]
    assert counter0 == counter
    for k in KEYS:
        assert np.array_equal(b[k][0][scripted].view(np.uint32), b0[k][0][scripted].view(np.uint32)), k
    # mix = 0.5: `played` is the specification's draw for every (row, market, agent)
    bh, taph, counterh = runs[0.5]
    rows, mk, ag = np.meshgrid(np.arange(T), np.arange(N), np.arange(A), indexing="ij")
    want = np.where(mixable[None], S.mix_played(TAP_SEED, counterh, TAP_BASE + mk, rows, ag, 1 << 31), 0)
    assert np.array_equal(taph["played"][:T], want) and 0 < want[:, mixable].mean() < 1
    on, off = want == 1, (want == 0) & mixable[None]
    for k in KEYS:
        assert np.array_equal(bh[k][on].view(np.uint32), taph[k][:T][on].view(np.uint32)), k           # played: the label
        assert np.array_equal(bh[k][0][off[0]].view(np.uint32), b0[k][0][off[0]].view(np.uint32)), k   # not played, row 0: the policy's sample of the mix = 0 twin
        assert np.array_equal(taph[k][0].view(np.uint32), tap0[k][0].view(np.uint32)), k               # row 0's labels do not depend on the mix (later rows diverge by design)
    assert (bh["logp"][0][off[0]] != 0).any()


def test_beta_changes_inside_a_captured_graph():
    env, _ = chain_env()
    table = tap_table(env)
    env.set_label_tap(table, LABELS, rows=T, seed=TAP_SEED, market_index_base=TAP_BASE, mix=0.0)
    ch = chains_on(env)
    ch.run()
    torch.cuda.synchronize()
    assert ch.graphs is not None and len(ch.graphs) == 2                 # captured
    graphs, epoch = [id(g) for g in ch.graphs], env.label_epoch
    learner = np.zeros((N, A), bool)
    learner[:, :LEARNER] = True
    assert (tap_host(env)["played"] == 0).all()
    env.set_label_mix(1.0)
    ch.run()
    torch.cuda.synchronize()
    assert [id(g) for g in ch.graphs] == graphs and env.label_epoch == epoch       # no re-capture
    p1 = tap_host(env)["played"]
    assert (p1[:, learner] == 1).all()
    env.set_label_mix(0.5)
    ch.run()
    torch.cuda.synchronize()
    counter = int(ch.counter.item())
    rows, mk, ag = np.meshgrid(np.arange(T), np.arange(N), np.arange(LEARNER), indexing="ij")
    assert np.array_equal(tap_host(env)["played"][:, :, :LEARNER], S.mix_played(TAP_SEED, counter, TAP_BASE + mk, rows, ag, 1 << 31))
    assert [id(g) for g in ch.graphs] == graphs and env.label_epoch == epoch
    env.close()


def test_refusals():
    from gym_continuousdoubleauction_amd import league_train, mlp, ppo
    from gym_continuousdoubleauction_amd._lib import lib
    env, _ = chain_env()
    table = tap_table(env)
    assert int(lib().cda_label_tap_attached(env._h)) == 0 and env.label_tap is None
    ch = chains_on(env)
    ch.run()
    torch.cuda.synchronize()
    e0 = int(lib().cda_label_tap_epoch(env._h))
    env.set_label_tap(table, LABELS, rows=T - 1, seed=1)
    assert int(lib().cda_label_tap_epoch(env._h)) == e0 + 1 and env.label_epoch == 1 and int(lib().cda_label_tap_attached(env._h)) == 1
    assert int(lib().cda_policy_step_supported(env._h)) == 0
    with pytest.raises(RuntimeError, match="label tap"):                 # attached after the capture
        ch.run()
    with pytest.raises(ValueError, match="rows"):                        # a horizon beyond the tap's rows
        chains_on(env)
    for train in (ppo.train_fused, league_train.train_league_fused):
        with pytest.raises(ValueError, match="label tap"):
            train(env, iters=1)
    # t >= rows from the C entry point: refused before any launch, nothing written
    g = torch.Generator().manual_seed(2)
    bufs = [torch.randint(-99, 99, (N, A), generator=g, dtype=torch.int32).to(DEV) for _ in range(5)]
    bufs = [b if i in (0, 3, 4) else b.view(torch.float32) for i, b in enumerate(bufs)]
    before, tap_before = [b.clone() for b in bufs], {k: env.label_tap[k].clone() for k in KEYS + ("played",)}
    st = torch.cuda.current_stream().cuda_stream
    for t in (T - 1, T, 10 ** 6):
        assert lib().cda_scripted_step_actions(env._h, 0, N, None, t, *(b.data_ptr() for b in bufs), None, None, None, st) == K.ERR_INVALID, t
    torch.cuda.synchronize()
    assert all(torch.equal(b.view(torch.int32), c.view(torch.int32)) for b, c in zip(bufs, before))
    assert all(torch.equal(env.label_tap[k], tap_before[k]) for k in tap_before)
    assert lib().cda_scripted_step_actions(env._h, 0, N, None, T - 2, *(b.data_ptr() for b in bufs), None, None, None, st) == 0       # the last row is fine
    torch.cuda.synchronize()
    assert bool((env.label_tap["category"][T - 2] != 0).any()) and not bool(env.label_tap["category"][:T - 2].any())
    # an invalid table or mix word changes nothing
    e1 = int(lib().cda_label_tap_epoch(env._h))
    tap = env.label_tap
    big = torch.full((N, A), len(LABELS) + 1, dtype=torch.int32, device=DEV)
    bad_mix = torch.tensor([(1 << 32) + 1], dtype=torch.int64, device=DEV)
    outs = [tap[k].data_ptr() for k in KEYS] + [tap["played"].data_ptr()]
    assert lib().cda_label_tap_attach(env._h, big.data_ptr(), tap["profiles"].data_ptr(), len(LABELS), 0, 0, tap["mix_q32"].data_ptr(), T, *outs) == K.ERR_INVALID
    assert lib().cda_label_tap_attach(env._h, tap["slot_label"].data_ptr(), tap["profiles"].data_ptr(), len(LABELS), 0, 0, bad_mix.data_ptr(), T, *outs) == K.ERR_INVALID
    bad = torch.from_numpy(S.profiles_array([dataclasses.replace(MAKER, depth_levels=11)], validate=False).view(np.uint8).copy()).to(DEV)
    assert lib().cda_label_tap_attach(env._h, torch.ones_like(big).data_ptr(), bad.data_ptr(), 1, 0, 0, tap["mix_q32"].data_ptr(), T, *outs) == K.ERR_INVALID
    assert int(lib().cda_label_tap_epoch(env._h)) == e1 and int(lib().cda_label_tap_attached(env._h)) == 1
    with pytest.raises(ValueError):
        env.set_label_tap(table, LABELS, rows=0)
    with pytest.raises(ValueError):
        env.set_label_tap(table, LABELS, rows=T, mix=1.5)
    env.clear_label_tap()
    assert int(lib().cda_label_tap_epoch(env._h)) == e1 + 1 and env.label_tap is None and int(lib().cda_label_tap_attached(env._h)) == 0
    with pytest.raises(RuntimeError):
        env.set_label_mix(0.5)
    # ... and a RolloutChains captured under a tap refuses to run once it is gone
    env.set_label_tap(table, LABELS, rows=T, seed=1)
    ch2 = chains_on(env)
    ch2.run()
    torch.cuda.synchronize()
    env.clear_label_tap()
    with pytest.raises(RuntimeError, match="label tap"):
        ch2.run()
    env.close()


# ---- 7. DAgger learns ------------------------------------------------------------------------------------------------------------------------
def test_dagger_learns(tmp_path):
    """256 x 4, horizon 32, four iterations, the maker's labels for slot 0 against taker opponents.  beta = 0.5 (then 0.25, 0.125, 0.0625): at the default beta = 1
    every learner sample of iteration 0 is mixed in, and the on-policy agreement of that iteration is over no sample at all.  No threshold: the last iteration is
    held against the run's own untrained start."""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd import imitate as IM
    from gym_continuousdoubleauction_amd.evaluate import evaluate
    env = CDAVecEnv({"num_of_agents": 4, "init_cash": 1000000, "max_step": 64, "is_render": False, "auto_reset": True}, n_markets=256, device=DEV, with_info=False)
    keep = {}
    policy, hist = IM.dagger(env, "maker", opponents=["taker"], learner_slots=1, iters=4, horizon=32, beta=0.5, seed=2, log=lambda s: None, keep=keep)
    torch.cuda.synchronize()
    first, last = hist[0], hist[-1]
    print("dagger maker: held-out NLL", first["held_before"]["nll"], "->", last["held"]["nll"], "on-policy agreement", [h["on_policy_agreement"] for h in hist],
          "beta", [h["beta"] for h in hist])
    assert len(hist) == 4 and [h["beta"] for h in hist] == [0.5, 0.25, 0.125, 0.0625]
    assert not env.scripted and env.label_tap is None                    # detached on exit
    assert last["held"]["nll"] < first["held_before"]["nll"]
    assert last["on_policy_agreement"] > first["on_policy_agreement"]
    buf = keep["buffer"]
    assert buf.filled == 4 and buf.demos.count == 4 * 32 * 224 and buf.demos.weight_sum == float(buf.demos.count)      # 224 training markets x 32 steps x the one learner slot, four times
    assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    path = str(tmp_path / "dagger.pt")
    mlp.save_policy(path, policy)
    assert torch.equal(mlp.load_policy(path, DEV).theta, policy.theta)
    res = evaluate(env, path, episodes=1, seed=1)
    assert res and (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    env.close()


def test_dagger_s_other_placements():
    """the two placements the run above does not take: the league's random modules behind the learner (opponents=None: a PolicyBank chain, its row 0 refreshed from
    the learner ahead of every rollout), and scripted opponents whose own slots are labelled too (label_opponents: every slot of a market is a demonstration)"""
    import math
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd import imitate as IM
    env = CDAVecEnv({"num_of_agents": 4, "init_cash": 1000000, "max_step": 64, "is_render": False, "auto_reset": True}, n_markets=64, device=DEV, with_info=False)
    for kw, slots in ((dict(opponents=None, learner_slots=2), 2), (dict(opponents=["taker", "imbalance"], learner_slots=1, label_opponents=True), 4)):
        keep = {}
        policy, hist = IM.dagger(env, "maker", iters=2, horizon=16, beta=0.5, aggregate=1, seed=3, log=lambda s: None, keep=keep, **kw)
        torch.cuda.synchronize()
        assert len(hist) == 2 and not env.scripted and env.label_tap is None
        assert all(math.isfinite(h["held"]["nll"]) and math.isfinite(h["train"]["nll"]) and 0.0 <= h["on_policy_agreement"] <= 1.0 for h in hist)
        assert hist[-1]["held"]["nll"] < hist[0]["held_before"]["nll"]
        assert keep["train"].count == 16 * 56 * slots and keep["buffer"].filled == 1 and keep["buffer"].demos.count == keep["train"].count      # 56 training markets
        assert (env.flags() == 0).all() and (env.check_invariants() == 0).all()
    with pytest.raises(ValueError):
        IM.dagger(env, "maker", opponents=None, label_opponents=True, iters=1, horizon=16)
    env.close()
