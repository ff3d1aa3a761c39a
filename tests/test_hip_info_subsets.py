"""GPU: cda_step with a SUBSET of the info tensors (include/cda.h cda_info_ptrs: any pointer may be NULL), through the C ABI, against the CPU oracle bit for bit.

The device code carries no null test: cda_step hands the kernel the env's own sink buffer in place of every pointer the caller left NULL (csrc/cda_hip.hip
fill_step_args).  What a caller must see is unchanged: each tensor it asked for is the oracle's, each buffer it did not hand over keeps its bytes, and obs / reward /
flags never depend on the set.

Every run: one shape, reset, one market prefilled far beyond the LDS tile (cold: the out-of-line general build steps it - slow_step<true>, with the tape on
slow_tstep<true> behind k_tstep<true>), 12 steps of seeded random actions whose sizes are large enough for sweeps of several fills, every step's outputs into its own
region of ONE canary-filled device slab that is read back once.  Pointer sets: all 20, none (info_out NULL), each tensor alone, the complement of each, 20 seeded
random subsets."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SHAPES = ((8, 1), (37, 5), (64, 16))
STEPS = 12
CANARY = 0xA5
SIZES = {"mkt_max_size": 40, "limit_size_multiple": 3}      # market orders of up to ~40 against resting orders of 1 .. 5: a sweep takes several fills


def _names():
    from gym_continuousdoubleauction_amd import _capi as K
    return [f[0] for f in K.INFO_FIELDS]


def pointer_sets():
    """(label, frozenset of tensor names | None = info_out NULL)"""
    names = _names()
    sets = [("all", frozenset(names)), ("none", None)]
    sets += [("only_" + n, frozenset([n])) for n in names]
    sets += [("all_but_" + n, frozenset(names) - {n}) for n in names]
    rng = np.random.default_rng(20)
    for k in range(20):
        pick = rng.random(len(names)) < rng.uniform(0.15, 0.85)
        sets.append((f"random_{k}", frozenset(n for n, p in zip(names, pick) if p)))
    return sets


def _config(A):
    return dict({"num_of_agents": A, "init_cash": 1000000, "max_step": 64, "is_render": False}, **SIZES)


def _actions(N, A, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(STEPS):
        cat = rng.integers(0, 9, (N, A)).astype(np.int32)
        cat = np.where(rng.random((N, A)) < 0.4, rng.choice([1, 5], (N, A)), cat).astype(np.int32)        # more market orders: sweeps
        out.append((cat, rng.uniform(-1, 1, (N, A)).astype(np.float32), rng.uniform(0, 1, (N, A)).astype(np.float32),
                    rng.integers(0, 10, (N, A)).astype(np.int32), rng.integers(0, 3, (N, A)).astype(np.int32)))
    return out


def _cold_market(N):
    return N // 2


def _start(env, N, A, seed):
    """reset + the cold market's book (product or oracle: the same calls)"""
    from fuzz_cases import prefill_book
    env.reset(seeds=(seed + np.arange(N)).astype(np.uint64))
    prefill_book(env, _cold_market(N), np.random.default_rng(seed + 1), A, 400, 400)


_ORACLE = {}


def oracle_run(N, A):
    """the 12 steps on the CPU oracle, once per shape: per step {name: array} of obs, reward, terminated, truncated and the 20 info tensors (read-only copies)"""
    if (N, A) not in _ORACLE:
        import oracle_lib as O
        ora = O.OracleEnv(_config(A), n_markets=N)
        _start(ora, N, A, 500 + N)
        assert sum(ora.book_size(_cold_market(N))) + A > (256 if A <= 8 else 512)          # market_is_cold (csrc/cda_kernels.inc)
        steps = []
        for acts in _actions(N, A, 900 + N):
            obs, rew, term, trunc, info = ora.step(*acts)
            rec = {"obs": obs.copy(), "reward": rew.copy(), "terminated": term.copy(), "truncated": trunc.copy()}
            rec.update({k: v.copy() for k, v in info.items()})
            for v in rec.values():
                v.setflags(write=False)
            steps.append(rec)
        assert not ora.flags().any()
        ora.close()
        _ORACLE[(N, A)] = steps
    return _ORACLE[(N, A)]


def fills_of(rec):
    """fills per market of one step: a fill counts once in each party's num_trades_step"""
    return rec["num_trades_step"].sum(axis=1) // 2


class Slab:
    """ONE device allocation with a region per (step, output): obs | reward | terminated | truncated | the 20 info tensors, 16-byte aligned each"""

    def __init__(self, N, A, obs_dim, steps=STEPS):
        import torch
        from gym_continuousdoubleauction_amd import _capi as K
        self.fields = [("obs", np.float32, (N, obs_dim)), ("reward", np.float64, (N, A)), ("terminated", np.uint8, (N,)), ("truncated", np.uint8, (N,))]
        np_of = {C.c_int32: np.int32, C.c_double: np.float64, C.c_uint8: np.uint8, K.Dec: K.DEC_DTYPE}
        for name, ct, per_agent, dims in K.INFO_FIELDS:
            self.fields.append((name, np_of[ct], ((N, A) if per_agent else (N,)) + tuple(dims)))
        self.off, off = {}, 0
        for name, dt, shape in self.fields:
            self.off[name] = off
            off += (int(np.prod(shape)) * np.dtype(dt).itemsize + 15) // 16 * 16
        self.step_bytes, self.steps = off, steps
        self.dev = torch.empty(off * steps, dtype=torch.uint8, device="cuda:0")
        self.base = self.dev.data_ptr()

    def ptr(self, t, name):
        return self.base + t * self.step_bytes + self.off[name]

    def fill(self):
        self.dev.fill_(CANARY)

    def host(self):
        h = self.dev.cpu().numpy()
        out = []
        for t in range(self.steps):
            rec = {}
            for name, dt, shape in self.fields:
                o = t * self.step_bytes + self.off[name]
                rec[name] = h[o:o + int(np.prod(shape)) * np.dtype(dt).itemsize]
            out.append(rec)
        return out


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Driver:
    """an env of the product, its action streams on the device and its slab; play(names) = reset, prefill, 12 cda_step calls with that pointer set"""

    def __init__(self, N, A, tape=False):
        import torch
        from hip_env import HipEnv
        self.N, self.A = N, A
        self.h = HipEnv(_config(A), n_markets=N, with_info=False)
        if tape:
            self.h.env.enable_tape(1024)
        self.acts = [[torch.from_numpy(x).to("cuda:0") for x in step] for step in _actions(N, A, 900 + N)]
        self.slab = Slab(N, A, self.h.env.obs_dim)

    def step(self, t, names, slab=None):
        import torch
        from gym_continuousdoubleauction_amd import _capi as K
        from gym_continuousdoubleauction_amd._lib import lib
        slab = slab or self.slab
        ptrs = K.InfoPtrs()
        for n in names or ():
            setattr(ptrs, n, slab.ptr(t, n))
        rc = lib().cda_step(self.h.env._h, *[x.data_ptr() for x in self.acts[t]], None, slab.ptr(t, "obs"), slab.ptr(t, "reward"), slab.ptr(t, "terminated"),
                            slab.ptr(t, "truncated"), None if names is None else C.byref(ptrs), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    def start(self):
        _start(self.h, self.N, self.A, 500 + self.N)

    def play(self, names):
        self.start()
        self.slab.fill()
        for t in range(STEPS):
            self.step(t, names)
        return self.slab.host()

    def close(self):
        self.h.close()


def check(label, names, got, want, fields):
    """got: Slab.host() of a run with the pointer set `names`; want: the oracle's steps"""
    info_names = set(_names())
    for t, (g, w) in enumerate(zip(got, want)):
        for name, _dt, _shape in fields:
            if name in info_names and (names is None or name not in names):
                assert (g[name] == CANARY).all(), f"{label}: step {t}: {name} was not asked for and was written"
            else:
                assert np.array_equal(g[name], _bytes(w[name])), f"{label}: step {t}: {name} differs from the oracle"


@pytest.mark.parametrize("tape", (False, True), ids=("notape", "tape"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_pointer_set_matches_the_oracle(shape, tape):
    N, A = shape
    want = oracle_run(N, A)
    most = max(int(fills_of(r).max()) for r in want)
    print(f"{N} x {A}: the busiest market-step has {most} fills")
    if A > 1:
        assert most >= 2, "the test's books are idle: no step with two or more fills"
    else:                                                    # an agent never trades with itself: a one-agent market cannot fill - its orders must at least reach the book
        assert most == 0 and sum(int(r["order_step_placed"].sum()) for r in want) >= STEPS, "the one-agent books are idle"
    d = Driver(N, A, tape)
    try:
        for label, names in pointer_sets():
            check(label, names, d.play(names), want, d.slab.fields)
        assert not d.h.flags().any()
    finally:
        d.close()


def test_two_envs_of_different_size_each_keep_their_own_sink():
    """two envs in one process, stepped alternately, the small one first: a sink shared between them, or sized for the wrong one, is an out-of-bounds store of the
    large env's 64 x 16 x 40 bytes"""
    sets = pointer_sets()
    a, b = Driver(8, 1), Driver(64, 16)
    try:
        for k in (2, 17, 30, 45, 55):                       # the small env: nav alone, last_price alone, a complement, two random subsets; the large one, from the list's other end: two random subsets, a complement, reward_terms alone, cash alone
            (la, na), (lb, nb) = sets[k], sets[len(sets) - 1 - k]
            a.start(); b.start()
            a.slab.fill(); b.slab.fill()
            for t in range(STEPS):
                a.step(t, na)
                b.step(t, nb)
            check(la, na, a.slab.host(), oracle_run(8, 1), a.slab.fields)
            check(lb, nb, b.slab.host(), oracle_run(64, 16), b.slab.fields)
    finally:
        a.close(); b.close()


def test_destroy_frees_the_sink():
    """create, step, destroy 50 small envs: the device memory in use is what it was before them"""
    import torch

    def one(k):
        d = Driver(8, 1)
        try:
            d.start()
            d.step(0, frozenset(["nav", "reward_terms"]) if k % 2 else None)
            torch.cuda.synchronize()
        finally:
            d.close()
        del d

    one(1); one(0)                                           # whatever the first env of a process leaves behind for good (code objects, the caching allocator's blocks)
    seen = []
    for _ in range(3):                                       # the figure is the device's, not the process's: a leak shows in every round, another process's allocation in one
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for k in range(50):
            one(k)
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        print(f"free device memory before {free0}, after {free1}")
        seen.append((free0, free1))
        if free1 == free0:
            break
    assert seen[-1][1] == seen[-1][0], seen
