"""Multi-GPU sharding of the market batch: one process per GPU (torch.distributed; backend "nccl" is
RCCL on ROCm, "gloo" in the CPU tests).

Markets are fully independent (each owns its book, accounts and RNG - SURVEY §8e), so the simulation
needs NO collective: rank r steps the contiguous block [r*N/G, (r+1)*N/G).  Seeds derive from the GLOBAL
market index, so results do not depend on the GPU count.  The only exchange is the hand-back of the
per-market outputs to a central learner, and of those only what is NEW each step travels: of the n_hist x 42
observation that is the newest frame, so a market hands back ONE compact record - f32 frame[42] | f64 reward[A] |
terminated | truncated | restarted, 208 B at 4 agents instead of the 706 B of observation + reward + flags
(`cda_set_handback`, include/cda.h) - and the receiving side rebuilds the stacked observation (shift by one frame,
append; `cda_handback_unpack`, one launch).

`ShardedVecEnv` steps its shard as the env's group chains (CDAVecEnv(groups=G): G independent chains of k_step launches
on G streams) and every chain carries ITS OWN collective: on stream g, k_step(group g, t) -> all_gather(records of group g)
-> unpack -> k_step(group g, t+1) ..., with one communicator per chain, so no dependency edge ever crosses streams and a
chain's transfer runs underneath the other chains' kernels.  On the fully connected xGMI node each rank pushes a group's
records (1024 markets x 208 B = 213 KB at 4096 x 4, G = 4) directly to its 7 peers, one link each.
`gather()` is the simple synchronous packed variant (whole observations) for any env and uneven shards.
"""
import ctypes as C
import os

import torch


def shard_range(rank, world, n_total):
    """Contiguous block partition of the market axis: (first, count) of `rank`.  Every rank holds n_total // world
    markets; a remainder goes to the LAST rank (the slab all-gather pads every shard to the largest one)."""
    if not 0 <= rank < world or n_total < world:
        raise ValueError(f"need 0 <= rank < world <= n_markets_total, got rank={rank} world={world} n_markets_total={n_total}")
    per = n_total // world
    return rank * per, per + (n_total - per * world if rank == world - 1 else 0)


def shard_pad(world, n_total):
    """Markets of the largest shard (what every rank's slab is laid out for)."""
    return n_total // world + n_total % world


def global_seeds(seed_base, first, count):
    """Seed of global market i = seed_base + i (uint64 bit pattern carried in an int64 tensor)."""
    return (torch.arange(first, first + count, dtype=torch.int64) + int(seed_base))


def slab_layout(n, obs_dim, num_agents):
    """Byte offsets of one rank's per-step outputs inside its output slab (16-byte padded)."""
    o_obs = 0
    o_rew = o_obs + n * obs_dim * 4
    o_rew = (o_rew + 7) // 8 * 8
    o_term = o_rew + n * num_agents * 8
    o_trunc = o_term + n
    total = (o_trunc + n + 15) // 16 * 16
    return {"n": n, "obs_dim": obs_dim, "num_agents": num_agents,
            "obs": o_obs, "reward": o_rew, "terminated": o_term, "truncated": o_trunc, "bytes": total}


def slab_views(slab, lay):
    """Typed views (no copies) into uint8 slab(s) of shape [..., bytes]:
    obs f32[..., n, obs_dim], reward f64[..., n, A], terminated u8[..., n], truncated u8[..., n]."""
    n, od, a = lay["n"], lay["obs_dim"], lay["num_agents"]
    lead = slab.shape[:-1]
    obs = slab[..., lay["obs"]:lay["obs"] + n * od * 4].view(torch.float32).view(*lead, n, od)
    rew = slab[..., lay["reward"]:lay["reward"] + n * a * 8].view(torch.float64).view(*lead, n, a)
    term = slab[..., lay["terminated"]:lay["terminated"] + n]
    trunc = slab[..., lay["truncated"]:lay["truncated"] + n]
    return obs, rew, term, trunc


def pack_outputs(obs, reward, terminated, truncated, out=None):
    """[n, obs_dim] f32, [n, A] f64, [n] bool, [n] bool -> [n, obs_dim + 2A + 2] f32 (bit-preserving)."""
    n, od = obs.shape
    a2 = reward.shape[1] * 2
    if out is None:
        out = torch.empty((n, od + a2 + 2), dtype=torch.float32, device=obs.device)
    out[:, :od].copy_(obs)
    out[:, od:od + a2].copy_(reward.contiguous().view(torch.float32))
    out[:, od + a2].copy_(terminated.to(torch.float32))
    out[:, od + a2 + 1].copy_(truncated.to(torch.float32))
    return out


def unpack_outputs(packed, obs_dim, num_agents):
    od, a2 = obs_dim, 2 * num_agents
    obs = packed[:, :od]
    reward = packed[:, od:od + a2].contiguous().view(torch.float64)
    terminated = packed[:, od + a2] != 0
    truncated = packed[:, od + a2 + 1] != 0
    return obs, reward, terminated, truncated


def handback_stride(num_agents):
    """bytes of one hand-back record (cda_handback_stride): f32 frame[42] | f64 reward[A] | u8 terminated, truncated, restarted | pad to 8"""
    return (42 * 4 + num_agents * 8 + 3 + 7) // 8 * 8


def _hip_unpack(records, n_segments, seg_records, seg_row_stride, row0, num_agents, n_hist, obs, reward, term, trunc, n_rows_total=0):
    """the product's receiving side: one launch of cda_handback_unpack on the CURRENT stream"""
    from ._lib import check, lib
    check(lib().cda_handback_unpack(records.data_ptr(), int(n_segments), int(seg_records), int(seg_row_stride), int(row0), int(num_agents), int(n_hist), int(n_rows_total),
                                    obs.data_ptr(), reward.data_ptr(), term.data_ptr(), trunc.data_ptr(),
                                    torch.cuda.current_stream(obs.device).cuda_stream), "cda_handback_unpack")


#: deadline (seconds) of a steady-state native collective call and of the device work behind it (CDA_HANDBACK_TIMEOUT_S)
HANDBACK_TIMEOUT_S = float(os.environ.get("CDA_HANDBACK_TIMEOUT_S", "60"))
#: deadline of the communicators' set-up, per communicator (CDA_COMM_INIT_TIMEOUT_S): a cold ncclCommInitRank over 8 GPUs can take tens of seconds, and a rank
#: builds one communicator per chain - the set-up deadline is this times the number of communicators, and missing it falls back to torch.distributed (every rank
#: agrees on that through an all-reduce) instead of ending the process
COMM_INIT_TIMEOUT_S = float(os.environ.get("CDA_COMM_INIT_TIMEOUT_S", "90"))


def _guarded(fn, what, streams=(), timeout=None, device=None, on_timeout="exit"):
    """Run `fn` (a native call that enqueues collectives) under a host watchdog: the call itself in a worker thread (RCCL sets its
    connections up lazily, inside the first collective, and that can block on the host), then every stream it enqueued on polled to
    completion - both against one deadline.  A collective that never completes makes the process EXIT non-zero with a diagnostic inside
    `timeout` seconds instead of hanging until somebody kills the job (torch.distributed's own timeout guards only ITS collectives);
    on_timeout="raise": a call that does not RETURN in time raises TimeoutError instead (the set-up path: the caller falls back).
    device: the HIP device the call must run on - the current device is a property of the host THREAD and a fresh thread starts on device 0, so the
    worker selects it before calling `fn` (without this every rank but 0 of a multi-GPU node would build its communicators on GPU 0)."""
    import sys
    import threading
    import time
    timeout = HANDBACK_TIMEOUT_S if timeout is None else float(timeout)
    box = {}

    def run():
        try:
            if device is not None and torch.device(device).type == "cuda":
                torch.cuda.set_device(torch.device(device))
            box["ret"] = fn()
        except BaseException as e:  # noqa: BLE001 - re-raised on the caller's thread
            box["err"] = e
    t0 = time.monotonic()
    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(timeout)
    if th.is_alive():
        if on_timeout == "raise":
            raise TimeoutError(f"{what}: the native call did not return within {timeout:.0f} s")
        print(f"[cda watchdog] {what}: the native call did not return within {timeout:.0f} s (a collective that cannot be set up or enqueued); exiting", file=sys.stderr, flush=True)
        os._exit(3)
    if "err" in box:
        raise box["err"]
    for s in streams:
        while not s.query():
            if time.monotonic() - t0 > timeout:
                print(f"[cda watchdog] {what}: the device did not finish the enqueued collectives within {timeout:.0f} s; exiting", file=sys.stderr, flush=True)
                os._exit(3)
            time.sleep(0.002)
    return box.get("ret")


def make_grad_allreduce(dist=None, group=None):
    """The one collective of a data-parallel learner (SURVEY 8(e) "if the learner is itself data-parallel over the same shards, the all-gather can be skipped
    entirely"): callable(tensor) -> the tensor summed in place over the ranks, on the caller's stream semantics of torch.distributed (RCCL: enqueued behind the
    current stream's work, the current stream ordered behind it; gloo: through the host).  mlp.FusedUpdate calls it on the 0.9-MB gradient between the reduce and
    the optimiser launches of every minibatch step; ppo.train_fused also on the two advantage sums of a rollout.
    op = "min" / "max": the same collective with ReduceOp.MIN / MAX - what the episode metrics' non-additive columns travel with, once per iteration and outside the
    timed region (episode_metrics.allreduce_tables)."""
    import torch.distributed as tdist
    d = dist or tdist

    def allreduce(t, op="sum"):
        if op not in ("sum", "min", "max"):
            raise ValueError(f"op must be 'sum', 'min' or 'max' (got {op!r})")
        d.all_reduce(t, op={"sum": d.ReduceOp.SUM, "min": d.ReduceOp.MIN, "max": d.ReduceOp.MAX}[op], group=group)
        return t
    return allreduce


class _Rccl:
    """RCCL through ctypes: only what the native hand-back needs - communicators the C side can call ncclAllGather on
    (cda_step_groups_handback issues the collectives itself, on the chains' own HIP streams).  The library is the copy PyTorch
    already loaded; it is re-opened RTLD_GLOBAL so that libcda_hip.so finds `ncclAllGather` in the process."""
    _inst = None

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]

    def __init__(self):
        cands = [os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so"), "librccl.so", "librccl.so.1"]
        err = None
        for c in cands:
            try:
                self.lib = C.CDLL(c, mode=C.RTLD_GLOBAL)
                break
            except OSError as e:  # noqa: PERF203
                err = e
        else:
            raise RuntimeError(f"RCCL not found: {err}")
        self.lib.ncclGetUniqueId.argtypes = [C.POINTER(self.UniqueId)]
        self.lib.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, self.UniqueId, C.c_int]
        self.lib.ncclCommDestroy.argtypes = [C.c_void_p]

    @classmethod
    def get(cls):
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst

    def draw_ids(self, dist, rank, world, n):
        """n unique ids: rank 0 draws them, torch.distributed carries them to the others - on the CALLER's thread (a process-group collective)"""
        ids = []
        for _ in range(n):
            uid = self.UniqueId()
            if rank == 0:
                rc = self.lib.ncclGetUniqueId(C.byref(uid))
                if rc != 0:
                    raise RuntimeError(f"ncclGetUniqueId: {rc}")
            ids.append(C.string_at(C.byref(uid), 128) if rank == 0 else None)    # (all 128 bytes: `.internal` would stop at the first NUL)
        if world > 1:
            dist.broadcast_object_list(ids, src=0)
        return ids

    def init_comm(self, raw_id, rank, world):
        """ncclCommInitRank on the CURRENT device of the calling thread (the guarded worker selects the rank's device first)"""
        uid = self.UniqueId()
        C.memmove(C.byref(uid), raw_id, 128)
        comm = C.c_void_p()
        rc = self.lib.ncclCommInitRank(C.byref(comm), world, uid, rank)
        if rc != 0:
            raise RuntimeError(f"ncclCommInitRank: {rc}")
        return comm

    def new_comm(self, dist, rank, world):
        """one communicator over all ranks (id exchange + init on the calling thread's current device)"""
        return self.init_comm(self.draw_ids(dist, rank, world, 1)[0], rank, world)


class ShardedVecEnv:
    """This rank's shard of a global batch of `n_markets_total` markets, and - with `handback=True` - the learner-side arrays
    of the WHOLE batch on this rank's device, refreshed every step from the all-gathered hand-back records:

        obs f32[n_total, n_hist*42], reward f64[n_total, A], terminated / truncated u8[n_total]     (`.full`)

    env_factory(config, n_local, device, groups) builds the local stepper (default: the HIP CDAVecEnv on this rank's GPU with
    `groups` chains and hand-back records; the CPU tests inject a stand-in with the same interface) and `unpack` the receiving
    side (default: the HIP kernel behind cda_handback_unpack; the CPU tests inject a restatement)."""

    def __init__(self, config, n_markets_total, device=None, env_factory=None, dist=None, groups=1, handback=False, unpack=None, transport="auto",
                 force_collective=False, market_configs=None):
        if market_configs is not None:
            raise ValueError("ShardedVecEnv does not take per-market parameters (market_configs) yet: build a CDAVecEnv per device with market_configs instead")
        import torch.distributed as tdist
        self.dist = dist or tdist
        self.rank = self.dist.get_rank() if self.dist.is_initialized() else 0
        self.world = self.dist.get_world_size() if self.dist.is_initialized() else 1
        self.n_total = int(n_markets_total)
        self.first, self.n_local = shard_range(self.rank, self.world, self.n_total)
        self.use_handback = bool(handback)
        # Uneven shards under the hand-back: every rank steps and sends the SAME number of records - the largest shard (the last rank's); the
        # other ranks pad theirs with up to world - 1 markets nobody reads (seeded beyond the global range, fed pass actions), and the
        # receiving side skips the padding (cda_set_handback_geometry).  Equal shards: nothing changes.
        self.n_env = shard_pad(self.world, self.n_total) if self.use_handback else self.n_local
        self.per = self.n_total // self.world
        self.uneven = self.use_handback and self.n_env != self.per
        if env_factory is None:
            from .vec_env import CDAVecEnv
            env_factory = lambda cfg, n, dev, g: CDAVecEnv(cfg, n_markets=n, device=dev, with_info=False, groups=g, handback=self.use_handback)   # noqa: E731
        self.env = env_factory(config, self.n_env, device, int(groups))
        self.obs_dim = self.env.obs_dim
        self.num_agents = self.env.num_agents
        self.n_hist = self.obs_dim // 42
        self._packed = None
        self._padded = None
        self._gathered = None
        self._pad_acts = None
        self.layout = slab_layout(self.n_local, self.obs_dim, self.num_agents)
        self.full = None
        self.transport_note = None
        if self.use_handback:
            self._unpack = unpack or _hip_unpack
            self._unpack_takes_total = unpack is None
            rec = self.env.handback
            dev = rec.device
            self.group_ranges = list(getattr(self.env, "group_ranges", None) or [(0, self.n_env)])
            self.group_streams = list(getattr(self.env, "group_streams", None) or [])
            stride = rec.shape[1]
            self._gbuf = [torch.zeros((self.world, cnt, stride), dtype=torch.uint8, device=dev) for _, cnt in self.group_ranges]
            self._rows_total = self.n_total if self.uneven else 0
            native_ok = dev.type == "cuda" and unpack is None and hasattr(self.env, "_h")
            if native_ok:
                from ._lib import check, lib
                check(lib().cda_set_handback_geometry(self.env._h, self.per if self.uneven else 0, self._rows_total), "cda_set_handback_geometry")
            # Transport.  "rccl" (the default on HIP devices when the process group runs on RCCL, or with one rank): the whole step -
            # every chain's k_step, ncclAllGather and rebuild - is ONE native call (cda_step_groups_handback); the library calls RCCL
            # itself on the chains' streams.  "torch": torch.distributed collectives issued from Python, chain by chain (~25 us of host
            # time per chain and step, tools/handback_host_probe.py) - the path of the gloo tests and of anything that is not RCCL.
            # Either way one communicator per chain, so that the chains' collectives may be in flight together.  "auto" = rccl where it
            # is available AND its start-up self-check passes on every rank (below); CDA_HANDBACK_TRANSPORT overrides "auto".
            asked = transport
            if transport == "auto":
                transport = os.environ.get("CDA_HANDBACK_TRANSPORT", "auto")
            if transport not in ("auto", "rccl", "torch"):
                raise ValueError(f"transport must be auto, rccl or torch, got {transport!r}")
            if transport == "auto":
                on_rccl = self.world == 1 or self.dist.get_backend() == "nccl"
                transport = "rccl" if (native_ok and on_rccl) else "torch"
            elif transport == "rccl" and not native_ok:
                raise ValueError("transport 'rccl' needs the HIP env (the library issues ncclAllGather itself)")
            self.transport = transport
            self._pgs, self._comms = [], None
            self.full = (torch.zeros((self.n_total, self.obs_dim), dtype=torch.float32, device=dev),
                         torch.zeros((self.n_total, self.num_agents), dtype=torch.float64, device=dev),
                         torch.zeros(self.n_total, dtype=torch.uint8, device=dev), torch.zeros(self.n_total, dtype=torch.uint8, device=dev))
            if transport == "rccl":
                G = len(self.group_ranges)
                if self.world > 1 or force_collective:       # (force_collective: a one-rank communicator, so that one GPU runs the real RCCL call)
                    comms, err = [], None
                    try:
                        rccl = _Rccl.get()
                        ids = rccl.draw_ids(self.dist, self.rank, self.world, G)          # the process-group broadcast stays on this thread; only RCCL's own calls are guarded
                        comms = _guarded(lambda: [rccl.init_comm(i, self.rank, self.world) for i in ids], "ncclCommInitRank", timeout=COMM_INIT_TIMEOUT_S * G,
                                         device=dev, on_timeout="raise")
                    except Exception as e:  # noqa: BLE001 - every rank must take the same branch below
                        err = e
                    if self._all_ranks_agree(err is None, dev):
                        self._comm_handles = comms
                        self._comms = (C.c_void_p * G)(*[c.value for c in comms])
                    else:                                    # some rank could not build its communicators: all ranks use torch.distributed
                        import sys
                        print(f"[ShardedVecEnv] rank {self.rank}: native RCCL communicators unavailable ({err}); falling back to torch.distributed", file=sys.stderr)
                        for c in comms:
                            _Rccl.get().lib.ncclCommDestroy(c)
                        transport = self.transport = "torch"
                        self.transport_note = f"asked {asked}: RCCL communicators unavailable"
                else:
                    _Rccl_optional_load()
                self._gptrs = (C.c_void_p * G)(*[b.data_ptr() for b in self._gbuf])
            if transport != "rccl" or (self.world > 1 and dev.type == "cuda"):
                # (the torch groups also serve the self-check of the native transport)
                self._pgs = [self.dist.new_group(ranks=list(range(self.world))) if self.world > 1 else None for _ in self.group_ranges]
            if transport == "rccl" and self._comms is not None:
                ok = self._native_selfcheck(dev)
                if not ok:
                    import sys
                    print(f"[ShardedVecEnv] rank {self.rank}: the native hand-back disagreed with torch.distributed on the self-check records; using torch.distributed",
                          file=sys.stderr)
                    for c in self._comm_handles:
                        _Rccl.get().lib.ncclCommDestroy(c)
                    self._comm_handles, self._comms = None, None
                    self.transport = "torch"
                    self.transport_note = f"asked {asked}: native self-check failed"
                else:
                    self.transport_note = "start-up self-check against torch.distributed passed on every rank"

    def _all_ranks_agree(self, ok, dev):
        t = torch.tensor([1.0 if ok else 0.0], device=dev)
        if self.world > 1:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
        return float(t.item()) >= 1.0

    def _native_selfcheck(self, dev):
        """One hand-back of synthetic records through the native transport (under the host watchdog) and one through torch.distributed,
        into two scratch sets of learner-side arrays; every rank compares and the verdicts are combined (MIN): a native path that hangs
        exits the process inside a minute, one that delivers wrong bytes is replaced by torch.distributed - before anything is timed."""
        from ._lib import check, lib
        env = self.env
        rec = env.handback
        g = torch.Generator().manual_seed(1234 + self.rank)
        saved = rec.clone()
        rec.copy_(torch.randint(0, 256, rec.shape, dtype=torch.uint8, generator=g).to(dev))
        a_set = tuple(torch.zeros_like(t) for t in self.full)
        b_set = tuple(torch.zeros_like(t) for t in self.full)
        streams = self.group_streams or [torch.cuda.current_stream(dev)]
        torch.cuda.synchronize(dev)
        ok = True
        try:
            arr = self._stream_array()
            _guarded(lambda: check(lib().cda_handback_groups(env._h, len(self.group_ranges), arr, self._comms, self.world, self._gptrs,
                                                             *[t.data_ptr() for t in a_set]), "cda_handback_groups"),
                     "native hand-back self-check", streams=streams, device=dev)
            torch.cuda.synchronize(dev)
            for gi, (first, cnt) in enumerate(self.group_ranges):
                buf = torch.zeros_like(self._gbuf[gi])
                mine = rec[first:first + cnt]
                if self.world > 1:
                    self.dist.all_gather_into_tensor(buf.view(-1), mine.reshape(-1), group=self._pgs[gi])
                else:
                    buf[0].copy_(mine)
                _hip_unpack(buf, self.world, cnt, self.per if self.uneven else self.n_env, first, self.num_agents, self.n_hist, *b_set, n_rows_total=self._rows_total)
            torch.cuda.synchronize(dev)
            ok = all(torch.equal(x.view(torch.uint8) if x.dtype != torch.uint8 else x, y.view(torch.uint8) if y.dtype != torch.uint8 else y) for x, y in zip(a_set, b_set))
        except Exception as e:  # noqa: BLE001 - a failing native path is a verdict, not a crash
            import sys
            print(f"[ShardedVecEnv] rank {self.rank}: native hand-back self-check raised {e!r}", file=sys.stderr)
            ok = False
        rec.copy_(saved)
        torch.cuda.synchronize(dev)
        return self._all_ranks_agree(ok, dev)

    # ------------------------------------------------------------------ the hand-back
    def _stream_ctx(self, g):
        if self.group_streams:
            return torch.cuda.stream(self.group_streams[g])
        import contextlib
        return contextlib.nullcontext()

    def _handback_group(self, g):
        """on chain g's stream: all-gather the chain's records, then one unpack launch into the full arrays"""
        first, cnt = self.group_ranges[g]
        mine = self.env.handback[first:first + cnt]
        buf = self._gbuf[g]
        if self.world > 1:
            self.dist.all_gather_into_tensor(buf.view(-1), mine.reshape(-1), group=self._pgs[g])
        else:
            buf[0].copy_(mine)
        stride_rows = self.per if self.uneven else self.n_env
        if self._unpack_takes_total:
            self._unpack(buf, self.world, cnt, stride_rows, first, self.num_agents, self.n_hist, *self.full, n_rows_total=self._rows_total)
        elif self.uneven:
            self._unpack(buf, self.world, cnt, stride_rows, first, self.num_agents, self.n_hist, *self.full, self._rows_total)
        else:
            self._unpack(buf, self.world, cnt, stride_rows, first, self.num_agents, self.n_hist, *self.full)

    def _stream_array(self):
        G = len(self.group_ranges)
        if self.group_streams:
            return (C.c_void_p * G)(*[s.cuda_stream for s in self.group_streams])
        return (C.c_void_p * G)(torch.cuda.current_stream(self.full[0].device).cuda_stream)

    def handback(self):
        """Enqueue the hand-back of the step (or reset) just enqueued: per chain, on the chain's own stream.  `full` is complete
        for chain g's rows when its stream gets there; join() orders the caller's stream after all of them."""
        if self.transport == "rccl":
            from ._lib import check, lib
            check(lib().cda_handback_groups(self.env._h, len(self.group_ranges), self._stream_array(), self._comms, self.world, self._gptrs,
                                            *[t.data_ptr() for t in self.full]), "cda_handback_groups")
            return
        for g in range(len(self.group_ranges)):
            with self._stream_ctx(g):
                self._handback_group(g)

    def join(self):
        if hasattr(self.env, "join"):
            self.env.join()

    def reset(self, seed_base=0):
        """seed_base = s: global market i is seeded s + i; None: every market keeps its RNG stream (reset(seed=None))."""
        seeds = None
        if seed_base is not None:
            seeds = global_seeds(seed_base, self.first, self.n_local)
            if self.n_env > self.n_local:                  # padding markets: seeded beyond the global range, never read by anybody
                seeds = torch.cat([seeds, global_seeds(seed_base, self.n_total + self.rank * self.world, self.n_env - self.n_local)])
        obs = self.env.reset(seed=seeds)
        if self.use_handback:               # the reset wrote `restarted` records: the full observation restarts from them
            if self.group_streams:
                self.env.fork()
            self.handback()
            self.join()
        return obs[:self.n_local]

    def _pad(self, acts, present):
        """uneven shards: the local action rows followed by pass actions (absent agents) for the padding markets"""
        if self.n_env == self.n_local:
            return acts, present
        n_extra = self.n_env - self.n_local
        out = []
        for x in acts:
            x = torch.as_tensor(x)
            out.append(torch.cat([x.reshape(self.n_local, self.num_agents), torch.zeros((n_extra, self.num_agents), dtype=x.dtype, device=x.device)]))
        ref = out[0]
        ps = torch.ones((self.n_local, self.num_agents), dtype=torch.uint8, device=ref.device) if present is None else torch.as_tensor(present).to(torch.uint8).reshape(self.n_local, self.num_agents)
        ps = torch.cat([ps.to(ref.device), torch.zeros((n_extra, self.num_agents), dtype=torch.uint8, device=ref.device)])
        return out, ps

    def _local(self, out):
        if self.n_env == self.n_local:
            return out
        obs, rew, term, trunc, info = out
        return obs[:self.n_local], rew[:self.n_local], term[:self.n_local], trunc[:self.n_local], info

    def step(self, category, size_mean, size_sigma, price, price_offset, present=None, pipelined=False):
        """Actions for THIS rank's markets ([n_local, A]); returns the local outputs.  With hand-back the full arrays follow on the
        chains' streams; pipelined=True leaves the fork / join with the caller's stream out (see CDAVecEnv.step)."""
        if not self.use_handback:
            return self.env.step(category, size_mean, size_sigma, price, price_offset, present)
        (category, size_mean, size_sigma, price, price_offset), present = self._pad((category, size_mean, size_sigma, price, price_offset), present)
        if self.transport == "rccl":
            return self._local(self._step_native(category, size_mean, size_sigma, price, price_offset, present, pipelined))
        if self.group_streams:
            if not pipelined:
                self.env.fork()             # the chains start after whatever the caller's stream holds (the actions a policy just wrote)
            out = self.env.step(category, size_mean, size_sigma, price, price_offset, present, pipelined=True)
        else:
            out = self.env.step(category, size_mean, size_sigma, price, price_offset, present)
        self.handback()
        if not pipelined:
            self.join()
        return self._local(out)

    def _step_native(self, category, size_mean, size_sigma, price, price_offset, present, pipelined):
        """every chain's step, collective and rebuild in ONE host call (cda_step_groups_handback)"""
        import torch as _t
        from ._lib import check, lib
        env = self.env
        cat, sm, ss = env._prep(category, _t.int32), env._prep(size_mean, _t.float32), env._prep(size_sigma, _t.float32)
        pr, po = env._prep(price, _t.int32), env._prep(price_offset, _t.int32)
        ps = None if present is None else env._prep(present, _t.uint8)
        if self.group_streams and (not pipelined or env._need_fork):
            env.fork()
        if len(env._views) > 1:                     # out_buffers > 1: the rotation CDAVecEnv.step performs
            env._cur = (env._cur + 1) % len(env._views)
            env._bind_outputs()
        if not hasattr(self, "_full_ptrs"):
            self._full_ptrs = [t.data_ptr() for t in self.full]
            self._streams_c = self._stream_array() if self.group_streams else None
        streams = self._streams_c if self._streams_c is not None else self._stream_array()
        with _t.cuda.device(env.device):
            check(lib().cda_step_groups_handback(env._h, len(self.group_ranges), cat.data_ptr(), sm.data_ptr(), ss.data_ptr(), pr.data_ptr(), po.data_ptr(),
                                                 ps.data_ptr() if ps is not None else None, *env._out_ptrs[env._cur], env._info_ref, streams,
                                                 self._comms, self.world, self._gptrs, *self._full_ptrs), "cda_step_groups_handback")
        env._keep_prev, env._keep = getattr(env, "_keep", None), (cat, sm, ss, pr, po, ps)
        if not pipelined:
            self.join()
        return env.obs, env.reward, env._term.view(_t.bool), env._trunc.view(_t.bool), env.info

    def gather(self, obs, reward, terminated, truncated):
        """All-gather the per-market outputs of every rank -> global (obs, reward, terminated, truncated)."""
        self._packed = pack_outputs(obs, reward, terminated, truncated, self._packed)
        if self.world == 1:
            return unpack_outputs(self._packed, self.obs_dim, self.num_agents)
        n_pad, cols = shard_pad(self.world, self.n_total), self._packed.shape[1]
        send = self._packed
        if n_pad != self.n_local:           # uneven shards (the last rank holds the remainder): every contribution is padded to the largest
            if self._padded is None:
                self._padded = torch.zeros((n_pad, cols), dtype=torch.float32, device=send.device)
            self._padded[:self.n_local].copy_(send)
            send = self._padded
        if self._gathered is None:
            self._gathered = torch.empty((self.world * n_pad, cols), dtype=torch.float32, device=send.device)
        self.dist.all_gather_into_tensor(self._gathered, send)
        g = self._gathered
        if self.n_total % self.world:
            g = torch.cat([g[r * n_pad: r * n_pad + shard_range(r, self.world, self.n_total)[1]] for r in range(self.world)], dim=0)
        return unpack_outputs(g, self.obs_dim, self.num_agents)

    def close(self):
        if getattr(self, "_comm_handles", None):
            if self.full is not None and self.full[0].is_cuda:
                torch.cuda.synchronize(self.full[0].device)
            for c in self._comm_handles:
                _Rccl.get().lib.ncclCommDestroy(c)
            self._comm_handles = None
        self.env.close()


def _Rccl_optional_load():
    """one rank needs no collective; loading RCCL is then optional"""
    try:
        _Rccl.get()
    except Exception:  # noqa: BLE001
        pass
