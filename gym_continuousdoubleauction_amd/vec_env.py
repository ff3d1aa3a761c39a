"""CDAVecEnv - N independent continuous-double-auction markets stepped in lockstep on one MI355X.

Host-side mirror of the reference env surface (continuousDoubleAuction_env.py:21-309) for a batch:
`reset()` / `step()` over torch tensors that stay resident in HBM.  All compute happens in the HIP
kernels behind the C-ABI (include/cda.h); PyTorch is only used for device memory and streams.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _capi as K
from ._lib import CDAError, check, lib

_TORCH_OF = {C.c_int32: torch.int32, C.c_double: torch.float64, C.c_uint8: torch.uint8}

DEC_DTYPE = K.DEC_DTYPE

ACTION_KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset")

# what set_scripted keeps: the two resident device tables (slot_script i32 [N, A], profiles u8 [n, 64]), the Profile objects, the draws' keys, and the slot table on the host
AttachedScripts = collections.namedtuple("AttachedScripts", "slot_script profiles_dev profiles seed market_index_base slots_host")
# what set_stateful keeps: the three resident device tensors (slots i32 [N, A], profiles u8 [n, 64], state i64 [N, A, 4]), the Profile objects, the keys, the host slot table
AttachedStateful = collections.namedtuple("AttachedStateful", "slot_table profiles_dev state profiles seed market_index_base slots_host")
# what set_order_schedule keeps: the three resident device tables (sched_of i32 [N], step_offsets i64 [n_sched, S + 1], msgs u8 [total, 16]), the host form and the digest
AttachedSchedule = collections.namedtuple("AttachedSchedule", "sched_of step_offsets msgs packed sched_of_host loop clear_step_counters digest")


class CDAVecEnv:
    """Batched env.  Tensors: actions [N,A]; obs f32[N, n_hist*42]; reward f64[N,A];
    terminated/truncated bool[N] (the reference's "__all__" flags); info = dict of SoA tensors."""

    def __init__(self, config=None, n_markets=1, device="cuda:0", with_info=True, out_buffers=1, groups=1, handback=False, group_streams=None,
                 market_configs=None):
        """market_configs: None (every market runs `config`) or a list of n_markets override dicts, one per market, holding only per-market keys
        (market_params.PER_MARKET_KEYS); missing keys come from `config`.  A row is validated before the device is touched."""
        self.cfg_struct, self.config = K.make_config(config)
        self.n_markets = int(n_markets)
        rows = None
        if market_configs is not None:
            from .market_params import rows_of
            if len(market_configs) != self.n_markets:
                raise ValueError(f"market_configs holds {len(market_configs)} configs for {self.n_markets} markets")
            rows = rows_of(self.config, list(market_configs))
        self.per_market = False             # whether rows were ever written (a snapshot then carries its markets' rows)
        self.host_epoch = 0                 # bumped by every host-side call that changes the markets (reset / step / run_random / place_order / set_state): consumers that keep
                                            # their own copy of the observations across calls (mlp.RolloutChains) compare it to know when theirs is stale
        self.tape_epoch = 0                 # bumped by enable_tape / disable_tape: graphs captured on this env's step launches hold the setting they were captured under
        self._tape_cursor = None            # drain_tape's default cursor (i64 [N], device) while the tape is on
        self.quote_epoch = 0                # bumped by enable_quotes / disable_quotes: captured graphs hold the recorder's launch (or none) of their capture
        self.depth_epoch = 0                # bumped by enable_depth / disable_depth: likewise for the depth recorder's launch
        self.order_tape_epoch = 0           # bumped by enable_order_tape / disable_order_tape: likewise for the order recorder's launch
        self.script_epoch = 0               # bumped by set_scripted / clear_scripted: graphs captured on this env's rollout chains hold the scripted launches (or none) of then
        self._script = None                 # set_scripted: an AttachedScripts (None while nothing is attached)
        self.stateful_epoch = 0             # bumped by set_stateful / clear_stateful: likewise for the stateful launch (or none)
        self._stateful = None               # set_stateful: an AttachedStateful (None while nothing is attached)
        self._schedule = None               # set_order_schedule: an AttachedSchedule (None while nothing is attached)
        self.label_epoch = 0                # bumped by set_label_tap / clear_label_tap (not by set_label_mix): captured graphs hold the tap's launch and buffers of their capture
        self.label_tap = None               # set_label_tap: a dict of the tap's tensors and settings (None while no tap is attached)
        self.num_agents = self.cfg_struct.num_agents
        self.n_hist = self.cfg_struct.n_hist
        self.obs_dim = self.n_hist * K.SNAPSHOT_DIM
        self.max_step = self.cfg_struct.max_step
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise CDAError("CDAVecEnv needs a HIP device (torch device 'cuda:<i>'); there is no CPU fallback")
        if not torch.cuda.is_available():
            raise CDAError("no GPU visible to PyTorch-ROCm; the HIP path cannot run and there is no CPU fallback")
        self.device_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.agents = [f"agent_{i}" for i in range(self.num_agents)]
        h = C.c_void_p()
        check(lib().cda_create(C.byref(self.cfg_struct), self.n_markets, self.device_index, C.byref(h)), "cda_create")
        self._h = h
        if rows is not None:
            self._write_rows(0, rows)
        self.book_capacity = int(lib().cda_book_capacity(h))     # LDS book tile: 256 or 512 resting orders per market (config['book_capacity'])
        self.book_spill = int(lib().cda_book_spill(h))           # HBM spill ring behind it: orders per side (config['book_spill']; 0 = none)
        self.book_spill_wanted = int(lib().cda_book_spill_wanted(h))   # ... and what an unbounded-inside-an-episode book needs
        if self.book_spill < self.book_spill_wanted:
            import warnings
            warnings.warn(f"the HBM spill ring was cut to {self.book_spill} orders per side ({self.book_spill_wanted} needed for a book that can never overflow inside an "
                          f"episode of {self.max_step} steps): device memory; a rest beyond tile + ring is dropped and flagged (CDA_FLAG_BOOK_OVERFLOW)", RuntimeWarning, stacklevel=2)
        N, A, dev = self.n_markets, self.num_agents, self.device
        # The per-step outputs of one launch live in ONE contiguous slab (obs | reward | terminated | truncated),
        # so a multi-GPU caller hands them to its peers with a single collective and no packing pass
        # (parallel.slab_layout describes the byte offsets).  out_buffers > 1 rotates the slab every step:
        # step t+1 writes a different slab while step t's is still being read by an all-gather in flight.
        from .parallel import slab_layout, slab_views
        self.slab_layout = slab_layout(N, self.obs_dim, A)
        self.with_info = bool(with_info)
        # ONE device allocation holds the output slab(s) and, behind them, every info tensor (16-byte aligned each):
        # a host-side consumer (the dict facades) moves a whole step's outputs with a single D2H copy of `packed`.
        B, sb = max(1, int(out_buffers)), self.slab_layout["bytes"]
        self.info_layout, off = {}, B * sb
        if self.with_info:
            for name, ct, per_agent, dims in K.INFO_FIELDS:
                shape = ((N, A) if per_agent else (N,)) + tuple(dims)
                shape = shape + (16,) if ct is K.Dec else shape
                dt = torch.uint8 if ct is K.Dec else _TORCH_OF[ct]
                nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
                self.info_layout[name] = (off, dt, shape, nbytes)
                off += (nbytes + 15) // 16 * 16
        self._all = torch.zeros(off, dtype=torch.uint8, device=dev)
        self._slabs = self._all[:B * sb].view(B, sb)
        self._views = [slab_views(self._slabs[b], self.slab_layout) for b in range(B)]
        self._out_ptrs = [tuple(t.data_ptr() for t in v) for v in self._views]
        self._step_call = lib().cda_step
        self._cur = 0
        self._bind_outputs()
        self.info = {}
        self._info_ptrs = K.InfoPtrs()
        for name, (o, dt, shape, nbytes) in self.info_layout.items():
            t = self._all[o:o + nbytes].view(dt).view(shape)
            self.info[name] = t
            setattr(self._info_ptrs, name, t.data_ptr())
        self._info_ref = C.byref(self._info_ptrs) if self.with_info else None
        # handback: every step / reset also writes ONE compact record per market of what is new (newest frame | reward | flags; see
        # cda_set_handback in include/cda.h) - what a multi-GPU caller all-gathers instead of the whole observation (parallel.py)
        self.handback = None
        if handback:
            self.handback_stride = int(lib().cda_handback_stride(A))
            self.handback = torch.zeros((N, self.handback_stride), dtype=torch.uint8, device=dev)
            check(lib().cda_set_handback(h, self.handback.data_ptr()), "cda_set_handback")
        # groups > 1: step() launches the batch as `groups` contiguous market groups, each an independent chain of
        # launches on its own stream (cda_step_groups).  Markets never interact, so nothing is lost - and a group's
        # slowest market no longer stalls the markets of the other groups.  See group_streams / join().
        self.groups = int(groups)
        if not 1 <= self.groups <= min(K.MAX_GROUPS, self.n_markets):
            raise ValueError(f"groups must be in 1..{min(K.MAX_GROUPS, self.n_markets)}")
        self.group_ranges = []
        for g in range(self.groups):
            first, cnt = C.c_int32(), C.c_int32()
            lib().cda_group_range(self.n_markets, self.groups, g, C.byref(first), C.byref(cnt))
            self.group_ranges.append((first.value, cnt.value))
        self.group_streams = []
        if self.groups > 1:
            from .streams import concurrent_streams
            if group_streams is not None:                   # the caller's own streams (e.g. a second groups > 1 env of the process)
                if len(group_streams) != self.groups:
                    raise ValueError(f"need {self.groups} group streams")
                self.group_streams = list(group_streams)
            else:
                self.group_streams = list(concurrent_streams(dev, self.groups))     # streams on DISTINCT hardware queues (measured once per process)
            self._stream_arr = (C.c_void_p * self.groups)(*[s.cuda_stream for s in self.group_streams])
            self._groups_call = lib().cda_step_groups
            self._fork_ev = torch.cuda.Event()
            self._join_ev = [torch.cuda.Event() for _ in range(self.groups)]
            self._need_fork = True

    @property
    def packed(self):
        """uint8 view of everything a step writes: [output slab(s) | info tensors] (`slab_layout`, `info_layout`)."""
        return self._all

    def unpack_host(self, host):
        """numpy views (no copies) into a HOST copy of `packed` (a uint8 numpy array or CPU tensor): the current
        slab's (obs, reward, terminated, truncated) and the info dict."""
        h = host.numpy() if isinstance(host, torch.Tensor) else host
        lay, sb = self.slab_layout, self.slab_layout["bytes"]
        base = self._cur * sb
        n, od, a = lay["n"], lay["obs_dim"], lay["num_agents"]
        obs = h[base + lay["obs"]: base + lay["obs"] + n * od * 4].view(np.float32).reshape(n, od)
        rew = h[base + lay["reward"]: base + lay["reward"] + n * a * 8].view(np.float64).reshape(n, a)
        term = h[base + lay["terminated"]: base + lay["terminated"] + n]
        trunc = h[base + lay["truncated"]: base + lay["truncated"] + n]
        info = {}
        for name, (o, dt, shape, nbytes) in self.info_layout.items():
            npdt = {torch.uint8: np.uint8, torch.int32: np.int32, torch.float64: np.float64}[dt]
            info[name] = h[o:o + nbytes].view(npdt).reshape(shape)
        return obs, rew, term, trunc, info

    # ------------------------------------------------------------------ host-resident step I/O (the dict facades)
    def bind_host_io(self):
        """The dict facades' step I/O without a copy in either direction: ONE pinned host block with the layout of `packed` (slab 0 | info tensors) that the step
        kernel WRITES over the fabric (its outputs are write-only, nontemporal stores), and action arrays the kernel READS from pinned host memory (pinned host
        memory is device-addressable at its own address on ROCm).  A one-market step then costs one launch and one stream synchronisation: no H2D / D2H copy call,
        no second trip through the caching allocator.  Returns the block as a uint8 numpy array (valid after `sync_host_io()`); groups == 1 only."""
        if self.groups != 1:
            raise CDAError("host-resident step I/O is for single-launch envs (groups == 1)")
        if getattr(self, "_hio", None) is None:
            host = torch.zeros(self._all.numel(), dtype=torch.uint8).pin_memory()
            base = host.data_ptr()
            lay = self.slab_layout
            outs = (base + lay["obs"], base + lay["reward"], base + lay["terminated"], base + lay["truncated"])
            ptrs = K.InfoPtrs()
            for name, (o, _dt, _shape, _nbytes) in self.info_layout.items():
                setattr(ptrs, name, base + o)
            self._hio = (host, outs, ptrs, C.byref(ptrs) if self.with_info else None)
        return self._hio[0].numpy()

    def step_host_io(self, action_ptrs):
        """cda_step with the six action arrays at `action_ptrs` (category, size_mean, size_sigma, price, price_offset, present: pinned host or device addresses) and the
        outputs into the block of bind_host_io(), on the caller's current stream.  Nothing is valid on the host before sync_host_io()."""
        self.host_epoch += 1
        _host, outs, _ptrs, info_ref = self._hio
        stream = torch.cuda.current_stream(self.device)
        if torch.cuda.current_device() == self.device_index:
            rc = self._step_call(self._h, *action_ptrs, *outs, info_ref, stream.cuda_stream)
        else:
            with torch.cuda.device(self.device):
                rc = self._step_call(self._h, *action_ptrs, *outs, info_ref, stream.cuda_stream)
        if rc != 0:
            check(rc, "cda_step")
        self._hio_stream = stream

    def reset_host_io(self, seed=None, mask=None):
        """reset() whose observation lands in the block of bind_host_io() (slab 0's obs) instead of the device tensor."""
        self.reset(seed=seed, mask=mask, _obs_ptr=self._hio[1][0])
        self._hio_stream = torch.cuda.current_stream(self.device)

    def sync_host_io(self):
        self._hio_stream.synchronize()

    def _bind_outputs(self):
        self.out_slab = self._slabs[self._cur]
        self.obs, self.reward, self._term, self._trunc = self._views[self._cur]

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None):
            lib().cda_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ reset / step
    def reset(self, seed=None, mask=None, _obs_ptr=None):
        """reset(seed=None): every selected market keeps its RNG stream (a never-seeded market is seeded
        with its index).  seed=int s: market i is seeded SeedSequence(s + i).  seed=array/tensor of N
        unsigned 64-bit seeds: per market.  mask: bool/uint8 [N] selecting the markets to reset.
        (_obs_ptr: where the first observations go instead of `self.obs` - reset_host_io.)"""
        seeds_t = None
        if seed is not None:
            if isinstance(seed, (int, np.integer)):
                arr = (np.uint64(int(seed)) + np.arange(self.n_markets, dtype=np.uint64)).astype(np.uint64)
            elif isinstance(seed, torch.Tensor):
                arr = seed.detach().cpu().numpy().astype(np.int64).view(np.uint64)
            else:
                arr = np.ascontiguousarray(seed, dtype=np.uint64)
            if arr.shape != (self.n_markets,):
                raise ValueError(f"need {self.n_markets} seeds, got shape {arr.shape}")
            seeds_t = torch.from_numpy(arr.view(np.int64).copy()).to(self.device)
        mask_t = None
        if mask is not None:
            mask_t = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous()
            if mask_t.shape != (self.n_markets,):
                raise ValueError("mask must have shape [n_markets]")
        self.host_epoch += 1
        self.join()                         # (groups > 1: the reset is issued on the caller's stream, after every group's last step)
        with torch.cuda.device(self.device):
            check(lib().cda_reset(self._h, seeds_t.data_ptr() if seeds_t is not None else None,
                                  mask_t.data_ptr() if mask_t is not None else None,
                                  self.obs.data_ptr() if _obs_ptr is None else _obs_ptr, self._stream()), "cda_reset")
        self._keep = (seeds_t, mask_t)
        if self.groups > 1:
            self._need_fork = True          # the group streams must see this reset (issued on the caller's stream)
        return self.obs

    # ------------------------------------------------------------------ per-market parameters (include/cda.h cda_market_params)
    def _write_rows(self, first, rows):
        if hasattr(self, "groups"):
            self.join()                     # (in the constructor nothing has been launched yet)
        with torch.cuda.device(self.device):
            check(lib().cda_set_market_params(self._h, int(first), len(rows), rows), "cda_set_market_params")
        self.per_market = True

    def market_rows(self, first=0, n=None):
        """the rows of markets [first, first + n) as a numpy array of market_params.ROW_DTYPE"""
        from .market_params import rows_to_numpy
        n = self.n_markets - int(first) if n is None else int(n)
        rows = (K.MarketParams * n)()
        check(lib().cda_get_market_params(self._h, int(first), n, rows), "cda_get_market_params")
        return rows_to_numpy(rows)

    def set_market_rows(self, first, rows_np):
        """write numpy rows (market_params.ROW_DTYPE) to markets [first, first + len(rows_np)), validated first; no reset"""
        from .market_params import rows_from_numpy, validate_rows
        rows = rows_from_numpy(rows_np)
        validate_rows(self.config, rows)
        self._write_rows(first, rows)

    def set_market_configs(self, configs, markets=None, seeds=None):
        """Give markets `markets` (default: all, in order) the override dicts `configs` (one per market; missing keys from the env's config) and
        reset exactly those markets: seeds=None keeps their RNG streams (reset(seed=None)), an int s seeds market i with s + i, a sequence seeds
        the listed markets one by one.  Every row is validated before anything is written; the other markets are untouched."""
        from .market_params import rows_of
        idx = np.arange(self.n_markets) if markets is None else np.asarray(markets, dtype=np.int64).reshape(-1)
        if len(configs) != len(idx):
            raise ValueError(f"{len(configs)} configs for {len(idx)} markets")
        if len(idx) == 0:
            return self.obs
        if idx.min() < 0 or idx.max() >= self.n_markets or len(np.unique(idx)) != len(idx):
            raise ValueError("markets must be distinct indices in [0, n_markets)")
        rows = rows_of(self.config, list(configs))
        seed_arr = None
        if seeds is not None:
            seed_arr = np.zeros(self.n_markets, dtype=np.uint64)
            if isinstance(seeds, (int, np.integer)):
                seed_arr[idx] = np.uint64(int(seeds)) + idx.astype(np.uint64)
            else:
                sv = np.asarray(seeds, dtype=np.uint64).reshape(-1)
                if len(sv) != len(idx):
                    raise ValueError(f"{len(sv)} seeds for {len(idx)} markets")
                seed_arr[idx] = sv
        order = np.argsort(idx, kind="stable")
        start = 0
        while start < len(order):                          # one table write per run of consecutive markets
            end = start + 1
            while end < len(order) and idx[order[end]] == idx[order[end - 1]] + 1:
                end += 1
            run = (K.MarketParams * (end - start))(*[rows[int(j)] for j in order[start:end]])
            self._write_rows(int(idx[order[start]]), run)
            start = end
        mask = np.zeros(self.n_markets, dtype=np.uint8)
        mask[idx] = 1
        return self.reset(seed=seed_arr, mask=mask)

    def market_config(self, i):
        """market i's effective config dict (the env's config with its row merged in)"""
        from .market_params import row_dict
        if not 0 <= int(i) < self.n_markets:
            raise IndexError(f"market {i} outside [0, {self.n_markets})")
        row = K.MarketParams()
        check(lib().cda_get_market_params(self._h, int(i), 1, C.byref(row)), "cda_get_market_params")
        out = dict(self.config)
        out.update(row_dict(row))
        return out

    # ------------------------------------------------------------------ market groups (groups > 1)
    def fork(self):
        """Order every group stream after the work enqueued so far on the caller's current stream (the reset, the
        actions a policy just produced).  step() does it by itself after reset() and join()."""
        self._fork_ev.record(torch.cuda.current_stream(self.device))
        for s in self.group_streams:
            s.wait_event(self._fork_ev)
        self._need_fork = False

    def sync(self):
        """Host-side barrier: wait until the device has finished everything enqueued on ANY stream (the group streams included).
        Afterwards no stream has pending work, so the next step() needs no fork and a consumer needs no join - unlike join(),
        this puts no dependency edge into any stream."""
        torch.cuda.synchronize(self.device)
        if self.groups > 1:
            self._need_fork = False

    def join(self):
        """Order the caller's current stream after every group's last step, so that the outputs can be consumed there;
        the next step() forks again.  A caller that pipelines per group works inside `torch.cuda.stream(group_streams[g])`
        on the rows `group_ranges[g]` instead and never joins."""
        if self.groups > 1:
            cur = torch.cuda.current_stream(self.device)
            for ev, s in zip(self._join_ev, self.group_streams):
                ev.record(s)
                cur.wait_event(ev)
            self._need_fork = True

    def _prep(self, x, dtype):
        if (isinstance(x, torch.Tensor) and x.dtype == dtype and x.device == self.device and x.is_contiguous()
                and x.numel() == self.n_markets * self.num_agents):
            return x                        # the hot loop's case: already a resident tensor of the ABI's layout
        t = torch.as_tensor(x)
        if t.device != self.device or t.dtype != dtype:
            t = t.to(device=self.device, dtype=dtype)
        t = t.reshape(self.n_markets, self.num_agents)
        return t.contiguous()

    def step(self, category, size_mean=None, size_sigma=None, price=None, price_offset=None, present=None, pipelined=False):
        """One env step for all markets.  `category` may also be a dict holding the five action tensors.  `present` u8[N,A]
        (optional): 0 = the agent is not in this step's action dict; non-zero values also carry the dict's iteration order
        (agents are processed by ascending value, ties by agent index - see include/cda.h).

        groups > 1: pipelined=True sends the launches to the group streams with no edge to the caller's stream: the caller orders things itself (fork() /
        join() / sync(), or per-group work on group_streams[g]) - what bench.py's free-running loop and the rollout chains do; a group's slowest market
        then overlaps the other groups' next steps.  The default (pipelined=False) is ordered AFTER everything enqueued on the caller's current stream (the
        tensors a policy just wrote) and the caller's stream AFTER the step, so it composes like any other stream-ordered op - since round 6 as ONE launch of
        the whole batch on the caller's stream: a step that is joined at once has no tail to overlap, and the fork + join event edges of G chains cost more
        than G concurrent launches gain (bench.py value_ordered_per_step: 202 M with the edges, the one launch's rate without; results are identical)."""
        if isinstance(category, dict):
            d = category
            present = d.get("present", present)
            category, size_mean, size_sigma, price, price_offset = (d[k] for k in ACTION_KEYS)
        self.host_epoch += 1
        cat = self._prep(category, torch.int32)
        sm = self._prep(size_mean, torch.float32)
        ss = self._prep(size_sigma, torch.float32)
        pr = self._prep(price, torch.int32)
        po = self._prep(price_offset, torch.int32)
        ps = None if present is None else self._prep(present, torch.uint8)
        if len(self._views) > 1:
            self._cur = (self._cur + 1) % len(self._views)
            self._bind_outputs()
        if self.groups > 1 and not pipelined and not self._need_fork:
            self.join()                     # the group streams hold steps the caller's stream has not seen: order it after them (and the next pipelined step forks)
        if self.groups > 1 and pipelined:
            if self._need_fork:
                self.fork()
            fn = self._groups_call
            call = (self._h, self.groups, cat.data_ptr(), sm.data_ptr(), ss.data_ptr(), pr.data_ptr(), po.data_ptr(),
                    ps.data_ptr() if ps is not None else None, *self._out_ptrs[self._cur], self._info_ref, self._stream_arr)
        else:
            fn = self._step_call
            call = (self._h, cat.data_ptr(), sm.data_ptr(), ss.data_ptr(), pr.data_ptr(), po.data_ptr(),
                    ps.data_ptr() if ps is not None else None, *self._out_ptrs[self._cur],
                    self._info_ref, torch.cuda.current_stream(self.device).cuda_stream)
        if torch.cuda.current_device() == self.device_index:
            rc = fn(*call)
        else:                               # the library selects its own device; keep the caller's current one intact
            with torch.cuda.device(self.device):
                rc = fn(*call)
        if rc != 0:
            check(rc, "cda_step")
        # keep the inputs of the last TWO steps alive: a pipelined caller may have step t still reading them on a group stream
        # when step t+1 is enqueued (the caching allocator would otherwise hand the memory out again on the caller's stream)
        self._keep_prev = getattr(self, "_keep", None)
        self._keep = (cat, sm, ss, pr, po, ps)
        return self.obs, self.reward, self._term.view(torch.bool), self._trunc.view(torch.bool), self.info

    def run_random(self, n_steps, action_seed=0, market_index_base=0):
        """The reference's `CDA_rand.run_random` for every market, in ONE kernel launch: uniform random agents (the
        counter-based sampler of include/cda_random_agents.h) play up to `n_steps` steps, each market stopping at its own
        episode end.  Returns (obs f32[N,obs_dim], episode_return f64[N,A], terminated, truncated, steps_taken i32[N]);
        bit-identical to `n_steps` calls of step() on `random_actions(t)`."""
        if self._schedule is not None:
            raise CDAError("run_random() cannot honour the attached order schedule (the whole episode runs inside one launch; cda_run_random answers "
                           "CDA_ERR_UNSUPPORTED): step the env, or clear_order_schedule() first")
        self.host_epoch += 1
        N, A, dev = self.n_markets, self.num_agents, self.device
        self.join()
        if not hasattr(self, "_rr_steps"):
            self._rr_return = torch.zeros((N, A), dtype=torch.float64, device=dev)
            self._rr_steps = torch.zeros(N, dtype=torch.int32, device=dev)
        with torch.cuda.device(self.device):
            check(lib().cda_run_random(self._h, int(n_steps), int(action_seed) & (2 ** 64 - 1), int(market_index_base) & (2 ** 64 - 1),
                                       self.obs.data_ptr(), self._rr_return.data_ptr(), self._term.data_ptr(), self._trunc.data_ptr(),
                                       self._rr_steps.data_ptr(), self._stream()), "cda_run_random")
        return self.obs, self._rr_return, self._term.view(torch.bool), self._trunc.view(torch.bool), self._rr_steps

    def random_actions_device(self, step0, n_steps, action_seed=0, market_index_base=0):
        """The same stream generated on the device: five [n_steps, N, A] tensors for steps step0 .. step0 + n_steps - 1."""
        N, A, dev = self.n_markets, self.num_agents, self.device
        cat, price, off = (torch.empty((n_steps, N, A), dtype=torch.int32, device=dev) for _ in range(3))
        mean, sigma = (torch.empty((n_steps, N, A), dtype=torch.float32, device=dev) for _ in range(2))
        with torch.cuda.device(self.device):
            check(lib().cda_random_actions(int(action_seed) & (2 ** 64 - 1), int(market_index_base) & (2 ** 64 - 1), int(step0), int(n_steps), N, A,
                                           cat.data_ptr(), mean.data_ptr(), sigma.data_ptr(), price.data_ptr(), off.data_ptr(), self._stream()),
                  "cda_random_actions")
        return cat, mean, sigma, price, off

    def random_actions(self, step, action_seed=0, market_index_base=0):
        """The five [N,A] action arrays (numpy, host) the random agents of `run_random` play at step `step`."""
        N, A = self.n_markets, self.num_agents
        cat, price, off = (np.zeros((N, A), np.int32) for _ in range(3))
        mean, sigma = (np.zeros((N, A), np.float32) for _ in range(2))
        check(lib().cda_random_actions_host(int(action_seed) & (2 ** 64 - 1), int(market_index_base) & (2 ** 64 - 1), int(step), N, A,
                                            cat.ctypes.data, mean.ctypes.data, sigma.ctypes.data, price.ctypes.data, off.ctypes.data),
              "cda_random_actions_host")
        return cat, mean, sigma, price, off

    # ------------------------------------------------------------------ diagnostics
    def place_order(self, market, trader, type_, side, size, price=1):
        self.host_epoch += 1
        check(lib().cda_place_order(self._h, market, trader, type_, side, size, price), "cda_place_order")

    def mark_to_mkt(self, market=0):
        check(lib().cda_mark_to_mkt(self._h, market), "cda_mark_to_mkt")

    def get_state(self, market=0):
        s = K.MarketState()
        torch.cuda.synchronize(self.device)
        check(lib().cda_get_state(self._h, market, C.byref(s)), "cda_get_state")
        return s

    def get_book(self, market=0, side=None):
        """One market's book, whole, in queue order (best price first, FIFO inside a level): int32 [n, 5] rows of
        (price, qty, owner, order_id, timestamp); side 0 bids, 1 asks, None = (bids, asks).  Unlike get_state() this is
        not limited to the first BOOK_CAP_MAX orders of a side."""
        if side is None:
            return self.get_book(market, 0), self.get_book(market, 1)
        torch.cuda.synchronize(self.device)
        n = C.c_int32()
        check(lib().cda_get_book(self._h, market, side, None, 0, C.byref(n)), "cda_get_book")
        buf = (K.Order * max(n.value, 1))()
        check(lib().cda_get_book(self._h, market, side, C.cast(buf, C.c_void_p), n.value, C.byref(n)), "cda_get_book")
        return np.ctypeslib.as_array(buf).view(np.int32).reshape(-1, 5)[: n.value].copy()

    def set_state(self, market, state):
        self.host_epoch += 1
        torch.cuda.synchronize(self.device)
        check(lib().cda_set_state(self._h, market, C.byref(state)), "cda_set_state")

    def raw_snapshot(self):
        self.join()
        raw = torch.zeros((self.n_markets, K.RAW_DIM), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().cda_get_raw_snapshot(self._h, raw.data_ptr(), self._stream()), "cda_get_raw_snapshot")
        return raw

    def flags(self):
        self.join()
        f = torch.zeros(self.n_markets, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().cda_last_flags(self._h, f.data_ptr(), self._stream()), "cda_last_flags")
        return f

    def book_peak(self):
        """Census: the most resting orders (both sides together) each market has held since its last reset, int32[N]."""
        self.join()
        p = torch.zeros(self.n_markets, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().cda_book_peak(self._h, p.data_ptr(), self._stream()), "cda_book_peak")
        return p

    def check_invariants(self):
        """Structural invariants of every market on the device (include/cda.h CDA_INV_*): int32[N] of violation bits, 0 = sides
        sorted by price, book uncrossed, quantities positive, cash_on_hold == value of own resting orders, positions
        net to zero."""
        self.join()
        v = torch.zeros(self.n_markets, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().cda_check_invariants(self._h, v.data_ptr(), self._stream()), "cda_check_invariants")
        return v

    def nav_conservation(self, tolerance=1e-6):
        """The reference's end-of-episode invariant for every market, computed on the device in the ledger's own decimal
        arithmetic: (float(|sum of NAV - A * init_cash|) f64[N], violated bool[N])."""
        self.join()
        err = torch.zeros(self.n_markets, dtype=torch.float64, device=self.device)
        bad = torch.zeros(self.n_markets, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().cda_nav_conservation(self._h, float(tolerance), err.data_ptr(), bad.data_ptr(), self._stream()), "cda_nav_conservation")
        return err, bad.view(torch.bool)

    # ------------------------------------------------------------------ every episode checked and summarised on the device
    def enable_episode_metrics(self, on=True, nav_tolerance=1e-6):
        """From now on every step tallies what the reference's callback tallies per episode, and every episode END is checked (exact sum of NAV against
        num_agents x init_cash, `nav_tolerance` = the callback's) and credited on the device, in the cold paths that handle it - the in-kernel auto reset
        included (include/cda.h cda_episode_metrics_enable; train/callbk/league_based_self_play_callback.py:541-755)."""
        check(lib().cda_episode_metrics_enable(self._h, 1 if on else 0, float(nav_tolerance)), "cda_episode_metrics_enable")
        self.episode_metrics_on = bool(on)
        self.episode_metrics_tolerance = float(nav_tolerance)

    def collect_episode_metrics(self, module_of=None, n_modules=1, clear=True, out=None):
        """The episodes that ended since the last collection, reduced on the device (two launches, a fixed order): (f64 [n_modules, EM_AGENT_FIELDS] per-module
        sums over the (episode, agent) pairs module m played - module_of i32 [N, A], None = one module -, f64 [EM_ENV_FIELDS] per-env sums); device tensors,
        columns = _capi.EM_*.  episode_metrics.summarise() turns them into the callback's metrics."""
        self.join()
        if out is None:                                     # (both are written whole by the second launch)
            out = (torch.empty((int(n_modules), K.EM_AGENT_FIELDS), dtype=torch.float64, device=self.device), torch.empty(K.EM_ENV_FIELDS, dtype=torch.float64, device=self.device))
        if module_of is not None:
            assert module_of.dtype == torch.int32 and module_of.is_contiguous() and module_of.numel() == self.n_markets * self.num_agents and module_of.device == self.device
        with torch.cuda.device(self.device):
            check(lib().cda_episode_metrics_collect(self._h, module_of.data_ptr() if module_of is not None else None, int(n_modules), out[0].data_ptr(), out[1].data_ptr(),
                                                    1 if clear else 0, self._stream()), "cda_episode_metrics_collect")
        return out

    # ------------------------------------------------------------------ the trade tape: every fill recorded on the device
    @property
    def tape_enabled(self):
        return int(lib().cda_tape_capacity(self._h)) > 0

    @property
    def tape_capacity(self):
        return int(lib().cda_tape_capacity(self._h))

    def enable_tape(self, capacity=1024):
        """From now on every fill of every market is appended to the market's ring of `capacity` records (a power of two) on the device - the reference's
        OrderBook.tape (include/cda.h cda_tape_enable; tape.py for the record layout).  Off by default; counters and rings start empty, the default
        drain cursor at 0.  Do not toggle it between the capture and the replay of a graph that holds this env's step launches (mlp.RolloutChains checks)."""
        capacity = int(capacity)
        if capacity < 1 or capacity & (capacity - 1):
            raise ValueError(f"tape capacity must be a power of two, got {capacity}")
        self.sync()
        check(lib().cda_tape_enable(self._h, capacity), "cda_tape_enable")
        self.tape_epoch += 1                                      # (captured graphs of this env's step launches are stale from here on)
        self._tape_cursor = torch.zeros(self.n_markets, dtype=torch.int64, device=self.device)

    def disable_tape(self):
        self.sync()
        check(lib().cda_tape_enable(self._h, 0), "cda_tape_enable")
        self.tape_epoch += 1
        self._tape_cursor = None

    def _need_tape(self, what):
        if not self.tape_enabled:
            raise RuntimeError(f"{what} needs the trade tape: call enable_tape() first (it is off by default)")

    def tape_counts(self):
        """{'n_total' i64[N]: fills since enable_tape, 'n_episode' i32[N]: fills since the market's last reset (the reference's len(LOB.tape)), 'episode' i32[N]:
        resets since enable_tape, 'partial' i32[N]: 1 = the episode's head is missing (the market was restored from a snapshot), 'n_previous' i32[N]: fills of the
        episode that ended at the market's last reset - records [n_total - n_episode - n_previous, n_total - n_episode)}, device tensors."""
        self._need_tape("tape_counts()")
        self.join()
        out = {"n_total": torch.empty(self.n_markets, dtype=torch.int64, device=self.device)}
        for k in ("n_episode", "episode", "partial", "n_previous"):
            out[k] = torch.empty(self.n_markets, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().cda_tape_counts_ex(self._h, out["n_total"].data_ptr(), out["n_episode"].data_ptr(), out["episode"].data_ptr(), out["partial"].data_ptr(),
                                           out["n_previous"].data_ptr(), self._stream()), "cda_tape_counts_ex")
        return out

    def drain_tape(self, cursor=None):
        """The streaming read: every market's records from its cursor on, oldest first, market after market -> (records i32 [K, 8] on the device, offsets i64 [N + 1]:
        market i owns rows offsets[i] : offsets[i + 1], dropped i64 [N]: records the ring had overwritten before they were read).  `cursor`: an i64 [N] device
        tensor of record numbers, advanced in place; None = the env's own, which starts at 0 with enable_tape."""
        self._need_tape("drain_tape()")
        cur = self._tape_cursor if cursor is None else cursor
        assert cur.dtype == torch.int64 and cur.is_contiguous() and cur.numel() == self.n_markets and cur.device == self.device
        self.join()
        n = self.n_markets
        with torch.cuda.device(self.device):
            off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
            dropped = torch.empty(n, dtype=torch.int64, device=self.device)
            check(lib().cda_tape_offsets(self._h, 0, n, cur.data_ptr(), off.data_ptr(), dropped.data_ptr(), self._stream()), "cda_tape_offsets")
            total = int(off[n].item())                  # the one 8-byte read
            rec = torch.empty((total, K.TAPE_WORDS), dtype=torch.int32, device=self.device)
            check(lib().cda_tape_pack(self._h, 0, n, cur.data_ptr(), off.data_ptr(), rec.data_ptr() if total else None, total, self._stream()), "cda_tape_pack")
        return rec, off, dropped

    def tape_last(self, k, first_market=0, n_markets=None, episode="current"):
        """The last k records of each market's CURRENT episode, oldest first (what state_helper.py walks with tape_display_length) ->
        (records i32 [n, k, 8], rows beyond the count zero; counts i32 [n]), device tensors.  episode="previous": of the episode that ended at the market's last reset."""
        self._need_tape("tape_last()")
        n = self.n_markets - int(first_market) if n_markets is None else int(n_markets)
        if not (0 <= int(first_market) and n >= 1 and int(first_market) + n <= self.n_markets and int(k) >= 1):
            raise ValueError(f"tape_last: range [{first_market}, {int(first_market) + n}) x {k} records is outside the env")
        which = self._tape_which(episode)
        return self._reader_call(lib().cda_tape_last_of, "cda_tape_last_of", int(first_market), n, (which, int(k)),
                                 (torch.empty((n, int(k), K.TAPE_WORDS), dtype=torch.int32, device=self.device), torch.empty(n, dtype=torch.int32, device=self.device)), info=False)

    @staticmethod
    def _tape_which(episode):
        if episode not in K.TAPE_EPISODES:
            raise ValueError(f"episode must be 'current' or 'previous', got {episode!r}")
        return K.TAPE_EPISODES[episode]

    def _market_range(self, what, first_market, n_markets):
        n = self.n_markets - int(first_market) if n_markets is None else int(n_markets)
        if not (0 <= int(first_market) and n >= 1 and int(first_market) + n <= self.n_markets):
            raise ValueError(f"{what}: range [{first_market}, {int(first_market) + n}) is outside the env's {self.n_markets} markets")
        return int(first_market), n

    def _top_max_step(self, first=0, n=None):
        """The largest max_step of the markets [first, first + n); by default of the whole env."""
        return int(self.market_rows(first, n)["max_step"].max()) if self.per_market else int(self.max_step)

    def _reader_call(self, fn, name, first, n, mid, outs, info=True):
        """One launch of a device reader (include/cda.h `name`, fn = lib().<name>) over the markets [first, first + n), on the caller's stream, ordered after every
        group's last step, no host synchronisation: fn(env, first, n, *mid, *outputs, stream).  mid: the plain arguments between the range and the outputs; outs:
        the tuple of the output tensors, allocated by the caller on self.device; info: the four-word info row [n, 4] behind them, allocated here.  -> the tuple of
        the outputs.  (Nothing else happens per call: these calls are launch-bound, and a microsecond of Python here is measurable.)"""
        self.join()
        if info:
            outs += (torch.empty((n, 4), dtype=torch.int32, device=self.device),)
        with torch.cuda.device(self.device):
            check(fn(self._h, first, n, *mid, *[t.data_ptr() for t in outs], self._stream()), name)
        return outs

    def tape_bars(self, bar_steps, n_bars=None, episode="current", first_market=0, n_markets=None):
        """Price / volume bars of one remembered episode, reduced on the device in one launch (include/cda.h cda_tape_bars): bar b of a market covers the episode's
        fills of env steps [b * bar_steps, (b + 1) * bar_steps) -> (bars i32 [n, n_bars, 12], info i32 [n, 4]), device tensors.  The twelve words of a bar are
        tape.BAR_DTYPE (tape.as_bars() gives the named view: open, high, low, close, n_trades, n_self, volume, buy_volume, notional); a bar without fills is
        all zeros.  info: records aggregated, records of the episode the ring had already overwritten, records beyond the last bar, partial flag.
        episode: "current", or "previous" = the episode that ended at the market's last reset.  n_bars defaults to ceil(max_step / bar_steps), largest max_step."""
        self._need_tape("tape_bars()")
        first, n = self._market_range("tape_bars", first_market, n_markets)
        which = self._tape_which(episode)
        if int(bar_steps) < 1:
            raise ValueError(f"tape_bars: bar_steps must be >= 1, got {bar_steps}")
        if n_bars is None:
            n_bars = -(-self._top_max_step() // int(bar_steps))
        if int(n_bars) < 1:
            raise ValueError(f"tape_bars: n_bars must be >= 1, got {n_bars}")
        return self._reader_call(lib().cda_tape_bars, "cda_tape_bars", first, n, (which, int(bar_steps), int(n_bars)),
                                 (torch.empty((n, int(n_bars), K.TAPE_BAR_WORDS), dtype=torch.int32, device=self.device),))

    def tape_flows(self, episode="current", first_market=0, n_markets=None):
        """Who trades with whom in one remembered episode (include/cda.h cda_tape_flows): (flows i64 [n, A, A, 3], info i32 [n, 4]), device tensors;
        flows[i, init_id, counter_id] = (quantity, notional = price x quantity, fills), the diagonal holds the self-trades.  info as tape_bars (its third word is 0)."""
        self._need_tape("tape_flows()")
        first, n = self._market_range("tape_flows", first_market, n_markets)
        which = self._tape_which(episode)
        return self._reader_call(lib().cda_tape_flows, "cda_tape_flows", first, n, (which,),
                                 (torch.empty((n, self.num_agents, self.num_agents, 3), dtype=torch.int64, device=self.device),))

    def tape_exec(self, horizons=(1, 5, 20), episode="current", first_market=0, n_markets=None):
        """The execution report of one remembered episode, per market and agent, reduced on the device in one launch (include/cda.h cda_tape_exec; tape.py
        exec_from_records is its specification, word for word): (stats i64 [n, A, 16], markouts i64 [n, A, H, 2, 4], info i32 [n, 4]), device tensors.
        stats: tape.STAT_FIELDS - bought / sold quantity and notional, quantity and fills as maker (counter_id) and as taker (init_id), self-trades, the running
        position's end, maximum and minimum, abs_pos_steps (the sum of |position| over the steps 0 .. S_last, S_last = the step of the last held record), first and
        last step of the agent's fills.  markouts[.., h, role 0 = maker / 1 = taker] = (sum of sign x (mark(s + horizons[h]) - price) x quantity, quantity, fills -
        over the fills whose s + horizons[h] <= S_last -, fills beyond that: open, counted and never marked); mark(t) = the last print at or before step t.
        horizons: 1 .. 8 step counts >= 0.  info as tape_flows; when it reports overwritten records or a partial episode the position words are relative to the
        first held record."""
        from .tape import _horizons
        self._need_tape("tape_exec()")
        first, n = self._market_range("tape_exec", first_market, n_markets)
        which = self._tape_which(episode)
        hz = _horizons(horizons)
        a = self.num_agents
        return self._reader_call(lib().cda_tape_exec, "cda_tape_exec", first, n, (which, (C.c_int32 * len(hz))(*hz), len(hz)),
                                 (torch.empty((n, a, K.TAPE_STAT_WORDS), dtype=torch.int64, device=self.device),
                                  torch.empty((n, a, len(hz), 2, 4), dtype=torch.int64, device=self.device)))

    def tape_episode(self, market=0):
        """The current episode's records of one market, oldest first, as a host array i32 [n, 8] (at most the ring's capacity of them)."""
        self._need_tape("tape_episode()")
        n_ep = int(self.tape_counts()["n_episode"][int(market)].item())
        k = max(1, min(n_ep, self.tape_capacity))
        rec, cnt = self.tape_last(k, int(market), 1)
        return rec[0, :int(cnt[0].item())].cpu().numpy()

    # ------------------------------------------------------------------ the quote tape: the top of the book per step, recorded on the device (quotes.py)
    @property
    def quotes_enabled(self):
        return int(lib().cda_quotes_capacity(self._h)) > 0

    @property
    def quote_capacity(self):
        return int(lib().cda_quotes_capacity(self._h))

    def enable_quotes(self, capacity=1024):
        """From now on every step entry point first records, per market whose episode is not over, the top of the book the step's orders will meet - best price,
        that level's volume and its order count per side (quotes.QUOTE_DTYPE) - into the market's ring of `capacity` records on the device (include/cda.h
        cda_quotes_enable), behind an attached order schedule's window and ahead of the step.  Off by default; rings start empty.  While it is on the one-launch
        policy step is off (rollout chains take their two-launch path) and run_random is refused.  Do not toggle it between the capture and the replay of a graph
        that holds this env's step launches (mlp.RolloutChains checks)."""
        capacity = int(capacity)
        if not 1 <= capacity <= (1 << 20):
            raise ValueError(f"quote capacity must be in 1 .. {1 << 20} steps, got {capacity}")
        self.sync()
        check(lib().cda_quotes_enable(self._h, capacity), "cda_quotes_enable")
        self.quote_epoch += 1                                     # (captured graphs of this env's step launches are stale from here on)

    def disable_quotes(self):
        self.sync()
        check(lib().cda_quotes_disable(self._h), "cda_quotes_disable")
        self.quote_epoch += 1

    def _need_quotes(self, what):
        if not self.quotes_enabled:
            raise RuntimeError(f"{what} needs the quote tape: call enable_quotes() first (it is off by default)")

    def quote_meta(self, first_market=0, n_markets=None):
        """Every market's meta row as the readers see it - rolled to the market's clock by the episode rule (quotes.roll) - i32 [n, 8], a device tensor;
        quotes.meta_from_words names the words, quotes.span says what the ring holds of either episode."""
        self._need_quotes("quote_meta()")
        first, n = self._market_range("quote_meta", first_market, n_markets)
        return self._reader_call(lib().cda_quote_meta, "cda_quote_meta", first, n, (), (torch.empty((n, 8), dtype=torch.int32, device=self.device),), info=False)[0]

    def quote_series(self, k=None, episode="current", first_market=0, n_markets=None):
        """The held quotes of one remembered episode, oldest first (include/cda.h cda_quote_series): (records i32 [n, k, 8] - quotes.QUOTE_DTYPE rows; rows beyond
        the count are zero -, counts i32 [n], info i32 [n, 4] = records returned, records of the episode's head the ring had overwritten, step of
        the first returned record, partial flag), device tensors.  An episode longer than k returns its LAST k records.  k defaults to the
        smaller of the ring's capacity and the largest max_step.  episode: "current", or "previous" = the episode that ended at the market's last reset."""
        self._need_quotes("quote_series()")
        first, n = self._market_range("quote_series", first_market, n_markets)
        which = self._tape_which(episode)
        if k is None:
            k = max(1, min(self.quote_capacity, self._top_max_step()))
        if int(k) < 1:
            raise ValueError(f"quote_series: k must be >= 1, got {k}")
        return self._reader_call(lib().cda_quote_series, "cda_quote_series", first, n, (which, int(k)),
                                 (torch.empty((n, int(k), K.QUOTE_WORDS), dtype=torch.int32, device=self.device), torch.empty(n, dtype=torch.int32, device=self.device)))

    def quote_stats(self, episode="current", first_market=0, n_markets=None):
        """The statistics of one remembered episode's held quotes, reduced on the device in one launch (include/cda.h cda_quote_stats; quotes.stats_from_quotes is
        its specification, word for word): (stats i64 [n, 16] - quotes.STAT_FIELDS -, info i32 [n, 4] = records aggregated, records lost to the ring, step of the
        first held record, partial flag), device tensors.  quotes.stats_summary turns a row into the ratios."""
        self._need_quotes("quote_stats()")
        first, n = self._market_range("quote_stats", first_market, n_markets)
        which = self._tape_which(episode)
        return self._reader_call(lib().cda_quote_stats, "cda_quote_stats", first, n, (which,),
                                 (torch.empty((n, K.QUOTE_STAT_WORDS), dtype=torch.int64, device=self.device),))

    def tape_spreads(self, horizons=(1, 5, 20), episode="current", first_market=0, n_markets=None):
        """The spread report of one remembered episode: the trade tape joined to the quotes by step, reduced on the device in one launch (include/cda.h
        cda_tape_spreads; quotes.spreads_from_records is its specification, word for word).  Needs the trade tape AND the quote tape.  -> (spreads i64
        [n, A, H, 2, 6], info i32 [n, 4]), device tensors: per agent, horizon and role (0 = maker, 1 = taker) quotes.SPREAD_FIELDS - cost_now = the sum of
        side x (2 price - m2(s)) x quantity, cost_later the same against m2(s + k), the scored quantity and fills, the fills whose s + k lies beyond the last held
        quote (open) and those whose quote at s or s + k is one-sided or no longer held (unquoted).  info: tape records aggregated, tape records lost, quote records
        lost, partial bits (1 tape, 2 quotes).  horizons: 1 .. 8 step counts >= 0.  quotes.spread_summary turns a row into the per-share ratios."""
        from .quotes import SPREAD_WORDS
        from .tape import _horizons
        self._need_tape("tape_spreads()")
        self._need_quotes("tape_spreads()")
        first, n = self._market_range("tape_spreads", first_market, n_markets)
        which = self._tape_which(episode)
        hz = _horizons(horizons)
        return self._reader_call(lib().cda_tape_spreads, "cda_tape_spreads", first, n, (which, (C.c_int32 * len(hz))(*hz), len(hz)),
                                 (torch.empty((n, self.num_agents, len(hz), 2, SPREAD_WORDS), dtype=torch.int64, device=self.device),))

    # ------------------------------------------------------------------ the stylised-facts report: return and order-flow statistics of an episode (stylised.py)
    def _stylised_points(self, what, first, n, bar_steps):
        """bar_steps, checked: the bar points of the longest episode of the range must fit a wave's LDS (include/cda.h CDA_STYL_MAX_BARS)"""
        from .stylised import MAX_BARS, _bar_steps, n_points
        bar = _bar_steps(bar_steps)
        top = self._top_max_step(first, n)
        if n_points(top, bar) > MAX_BARS:
            raise ValueError(f"{what}: an episode of {top} steps has {n_points(top, bar)} bar points at bar_steps = {bar}, more than {MAX_BARS}: raise bar_steps")
        return bar

    def quote_returns(self, lags=(1, 2, 5, 10), bar_steps=1, hist_half=16, episode="current", first_market=0, n_markets=None):
        """The return statistics of one remembered episode's held quotes, reduced on the device in one launch (include/cda.h cda_quote_returns;
        stylised.returns_from_quotes is its specification, word for word).  Needs the quote tape.  -> (base i64 [n, 8] - stylised.RETURN_FIELDS: bar points held,
        defined returns, missing ones, sum_r, sum_abs, sum_r2, up, down -, lagged i64 [n, L, 4] - RETURN_LAG_FIELDS per lag: n, rr, aa, ra -, hist i64
        [n, 2 hist_half + 1] - returns in ticks of the market's own row, the end bins hold the clipped mass -, info i32 [n, 4] as quote_stats), device tensors.
        The return at bar point p is m2((p + 1) bar_steps) - m2(p bar_steps), in half price units.  lags: 1 .. 8 values >= 1, in bars; every word is additive:
        stylised.pool sums over markets, stylised.summary turns pooled tables into autocorrelations, variance ratio, kurtosis."""
        from .stylised import MAX_HIST_HALF, RETURN_FIELDS, RETURN_LAG_FIELDS, _lags
        self._need_quotes("quote_returns()")
        first, n = self._market_range("quote_returns", first_market, n_markets)
        which = self._tape_which(episode)
        lg = _lags(lags, 1)
        if not 1 <= int(hist_half) <= MAX_HIST_HALF:
            raise ValueError(f"quote_returns: hist_half must be in 1 .. {MAX_HIST_HALF}, got {hist_half}")
        bar = self._stylised_points("quote_returns", first, n, bar_steps)
        return self._reader_call(lib().cda_quote_returns, "cda_quote_returns", first, n, (which, (C.c_int32 * len(lg))(*lg), len(lg), bar, int(hist_half)),
                                 (torch.empty((n, len(RETURN_FIELDS)), dtype=torch.int64, device=self.device),
                                  torch.empty((n, len(lg), len(RETURN_LAG_FIELDS)), dtype=torch.int64, device=self.device),
                                  torch.empty((n, 2 * int(hist_half) + 1), dtype=torch.int64, device=self.device)))

    def tape_signs(self, lags=(1, 2, 5, 10), episode="current", first_market=0, n_markets=None):
        """The order-flow sign statistics of one remembered episode's held fills, in tape order, reduced on the device in one launch (include/cda.h cda_tape_signs;
        stylised.signs_from_records is its specification, word for word).  Needs the trade tape.  -> (base i64 [n, 8] - stylised.SIGN_FIELDS: fills, buys, sells,
        buy_qty, sell_qty, self_fills, runs, steps_with_fills -, lagged i64 [n, L, 4] - SIGN_LAG_FIELDS per lag, in TRADE time: n, ss, qq, same_step -, info i32
        [n, 4] as tape_flows), device tensors.  lags: 1 .. 8 values >= 1, in fills."""
        from .stylised import SIGN_FIELDS, SIGN_LAG_FIELDS, _lags
        self._need_tape("tape_signs()")
        first, n = self._market_range("tape_signs", first_market, n_markets)
        which = self._tape_which(episode)
        lg = _lags(lags, 1)
        return self._reader_call(lib().cda_tape_signs, "cda_tape_signs", first, n, (which, (C.c_int32 * len(lg))(*lg), len(lg)),
                                 (torch.empty((n, len(SIGN_FIELDS)), dtype=torch.int64, device=self.device),
                                  torch.empty((n, len(lg), len(SIGN_LAG_FIELDS)), dtype=torch.int64, device=self.device)))

    def tape_flow_returns(self, lags=(0, 1, 5), bar_steps=1, episode="current", first_market=0, n_markets=None):
        """Signed volume joined to returns, bar by bar, of one remembered episode, reduced on the device in one launch (include/cda.h cda_tape_flow_returns;
        stylised.flow_returns_from_records is its specification, word for word).  Needs the trade tape AND the quote tape.  -> (lagged i64 [n, L, 6] -
        stylised.FLOW_LAG_FIELDS per lag l >= 0 over the kept bars b whose return r_(b + l) is defined: n, q = sum Q_b, r, qr, qq, rr; lag 0 is the impact
        regression -, base i64 [n, 4] - FLOW_FIELDS: fills and quantity of the kept bars, the kept bars with fills, bars_excluded (the bars up to the first held
        fill's where the tape ring has lost the episode's head) -, info i32 [n, 4] as tape_spreads), device tensors.  lags: 1 .. 8 values >= 0, in bars."""
        from .stylised import FLOW_FIELDS, FLOW_LAG_FIELDS, _lags
        self._need_tape("tape_flow_returns()")
        self._need_quotes("tape_flow_returns()")
        first, n = self._market_range("tape_flow_returns", first_market, n_markets)
        which = self._tape_which(episode)
        lg = _lags(lags, 0)
        bar = self._stylised_points("tape_flow_returns", first, n, bar_steps)
        return self._reader_call(lib().cda_tape_flow_returns, "cda_tape_flow_returns", first, n, (which, (C.c_int32 * len(lg))(*lg), len(lg), bar),
                                 (torch.empty((n, len(lg), len(FLOW_LAG_FIELDS)), dtype=torch.int64, device=self.device),
                                  torch.empty((n, len(FLOW_FIELDS)), dtype=torch.int64, device=self.device)))

    # ------------------------------------------------------------------ the P&L report: every agent's mark-to-mid equity curve of an episode (pnl.py)
    def tape_pnl(self, bar_steps=1, episode="current", series=False, first_market=0, n_markets=None):
        """What every agent's P&L did over one remembered episode: the trade tape joined to the quote tape on the bar points, reduced on the device in one launch
        (include/cda.h cda_tape_pnl; pnl.pnl_from_records is its specification, word for word).  Needs the trade tape AND the quote tape.  -> (stats i64 [n, A, 16]
        - pnl.PNL_FIELDS: marked / stale / unmarked points, bars, equity_first / _last, the inventory and trading parts of the P&L, sum_d2, up, down, under_water,
        max_drawdown, equity_max / _min, open_fills; money in half price units -, info i32 [n, 4] as tape_spreads) or, with series=True, (stats, equity i64
        [n, A, P], position i32 [n, A, P], marks i32 [n, P], info): E(p), pos(p) and the mark m(p) on the absolute grid of the P = ceil(largest max_step /
        bar_steps) points, zeros where a point is not marked (position: not held).  Device tensors; every word is written by the kernel.  pnl.fold /
        pnl.pnl_by_module fold rows, pnl.pnl_summary turns one into P&L, drawdown, Sharpe and hit ratio."""
        from .pnl import PNL_WORDS, n_points
        self._need_tape("tape_pnl()")
        self._need_quotes("tape_pnl()")
        first, n = self._market_range("tape_pnl", first_market, n_markets)
        which = self._tape_which(episode)
        bar = self._stylised_points("tape_pnl", first, n, bar_steps)
        pts = n_points(self._top_max_step(first, n), bar)
        a = self.num_agents
        stats = torch.empty((n, a, PNL_WORDS), dtype=torch.int64, device=self.device)
        equity = position = marks = None
        if series:
            equity = torch.empty((n, a, pts), dtype=torch.int64, device=self.device)
            position = torch.empty((n, a, pts), dtype=torch.int32, device=self.device)
            marks = torch.empty((n, pts), dtype=torch.int32, device=self.device)
        # (n_points stands between the curves and the info row, and the curves may be NULL: the tables travel among the plain arguments, the info row is the output)
        info, = self._reader_call(lib().cda_tape_pnl, "cda_tape_pnl", first, n, (which, bar, stats.data_ptr(), equity.data_ptr() if series else None,
                                  position.data_ptr() if series else None, marks.data_ptr() if series else None, pts), ())
        return (stats, equity, position, marks, info) if series else (stats, info)

    def quote_episode(self, market=0, episode="current"):
        """One market's held quotes of an episode, oldest first, as a structured host array (quotes.QUOTE_DTYPE)."""
        from .quotes import as_quotes
        rec, cnt, _ = self.quote_series(None, episode, int(market), 1)
        return as_quotes(rec[0, :int(cnt[0].item())].cpu().numpy()).copy()

    # ------------------------------------------------------------------ the depth tape: the Level-2 ladder per step, recorded on the device (depth.py)
    @property
    def depth_enabled(self):
        return int(lib().cda_depth_capacity(self._h)) > 0

    @property
    def depth_capacity(self):
        return int(lib().cda_depth_capacity(self._h))

    @property
    def depth_levels(self):
        return int(lib().cda_depth_levels(self._h))

    def enable_depth(self, capacity=1024, levels=10):
        """From now on every step entry point first records, per market whose episode is not over, the best `levels` price levels of both sides of the book the
        step's orders will meet - price and summed volume per level (depth.record_dtype(levels)) - into the market's ring of `capacity` records on the device
        (include/cda.h cda_depth_enable), behind an attached order schedule's window and the quote recorder and ahead of the step.  Off by default; rings start
        empty; it needs neither the quote tape nor the trade tape.  While it is on the one-launch policy step is off (rollout chains take their two-launch path) and
        run_random is refused.  Do not toggle it between the capture and the replay of a graph that holds this env's step launches (mlp.RolloutChains checks)."""
        from .depth import MAX_LEVELS
        capacity, levels = int(capacity), int(levels)
        if not 1 <= capacity <= (1 << 20) or not 1 <= levels <= MAX_LEVELS:
            raise ValueError(f"depth capacity must be in 1 .. {1 << 20} steps and levels in 1 .. {MAX_LEVELS}, got {capacity}, {levels}")
        self.sync()
        check(lib().cda_depth_enable(self._h, capacity, levels), "cda_depth_enable")
        self.depth_epoch += 1                                     # (captured graphs of this env's step launches are stale from here on)

    def disable_depth(self):
        self.sync()
        check(lib().cda_depth_disable(self._h), "cda_depth_disable")
        self.depth_epoch += 1

    def _need_depth(self, what):
        if not self.depth_enabled:
            raise RuntimeError(f"{what} needs the depth tape: call enable_depth() first (it is off by default)")

    def depth_meta(self, first_market=0, n_markets=None):
        """Every market's meta row of the depth tape as the readers see it - rolled to the market's clock by the episode rule (quotes.roll) - i32 [n, 8], a device
        tensor; quotes.meta_from_words names the words, quotes.span says what the ring holds of either episode."""
        self._need_depth("depth_meta()")
        first, n = self._market_range("depth_meta", first_market, n_markets)
        return self._reader_call(lib().cda_depth_meta, "cda_depth_meta", first, n, (), (torch.empty((n, 8), dtype=torch.int32, device=self.device),), info=False)[0]

    def depth_series(self, k=None, episode="current", first_market=0, n_markets=None):
        """The held ladders of one remembered episode, oldest first (include/cda.h cda_depth_series): (records i32 [n, k, (1 + levels) * 4] - depth.as_depth names
        the words; rows beyond the count are zero -, counts i32 [n], info i32 [n, 4] = records returned, records of the episode's head the ring had overwritten,
        step of the first returned record, partial flag), device tensors.  An episode longer than k returns its LAST k records.  k defaults to the smaller of the
        ring's capacity and the largest max_step."""
        self._need_depth("depth_series()")
        first, n = self._market_range("depth_series", first_market, n_markets)
        which = self._tape_which(episode)
        if k is None:
            k = max(1, min(self.depth_capacity, self._top_max_step()))
        if int(k) < 1:
            raise ValueError(f"depth_series: k must be >= 1, got {k}")
        return self._reader_call(lib().cda_depth_series, "cda_depth_series", first, n, (which, int(k)),
                                 (torch.empty((n, int(k), 4 * (1 + self.depth_levels)), dtype=torch.int32, device=self.device),
                                  torch.empty(n, dtype=torch.int32, device=self.device)))

    def depth_episode(self, market=0, episode="current"):
        """One market's held ladders of an episode, oldest first, as a structured host array (depth.record_dtype(levels))."""
        from .depth import as_depth
        rec, cnt, _ = self.depth_series(None, episode, int(market), 1)
        return as_depth(rec[0, :int(cnt[0].item())].cpu().numpy(), self.depth_levels).copy()

    def depth_profile(self, max_dist=32, episode="current", first_market=0, n_markets=None):
        """The average shape of the book over one remembered episode's held ladders, reduced on the device in one launch (include/cda.h cda_depth_profile;
        depth.profile_from_records is its specification, word for word).  -> (base i64 [n, 8] - depth.PROFILE_FIELDS -, levels i64 [n, 2, L, 3] - per side and
        level index steps, volume, distance in ticks from the side's best -, shape i64 [n, 2, max_dist + 1] - volume by distance, the last bin holds the clipped
        mass -, info i32 [n, 4] as quote_stats), device tensors.  Every word is additive: depth.pool sums over markets, depth.summary reads the ratios."""
        from .depth import MAX_DIST
        self._need_depth("depth_profile()")
        first, n = self._market_range("depth_profile", first_market, n_markets)
        which = self._tape_which(episode)
        if not 1 <= int(max_dist) <= MAX_DIST:
            raise ValueError(f"depth_profile: max_dist must be in 1 .. {MAX_DIST}, got {max_dist}")
        L = self.depth_levels
        return self._reader_call(lib().cda_depth_profile, "cda_depth_profile", first, n, (which, int(max_dist)),
                                 (torch.empty((n, 8), dtype=torch.int64, device=self.device), torch.empty((n, 2, L, 3), dtype=torch.int64, device=self.device),
                                  torch.empty((n, 2, int(max_dist) + 1), dtype=torch.int64, device=self.device)))

    def depth_imbalance(self, lags=(1, 2, 5, 10), k=None, half=8, episode="current", first_market=0, n_markets=None):
        """The future mid move given today's depth imbalance, over one remembered episode's held ladders, reduced on the device in one launch (include/cda.h
        cda_depth_imbalance; depth.imbalance_from_records is its specification, word for word).  -> (resp i64 [n, n_lags, 2 half, 5] - per lag and imbalance bin
        depth.RESPONSE_FIELDS: n, sum r, sum r^2, up, down -, base i64 [n, 4] - depth.IMBALANCE_FIELDS -, info i32 [n, 4] as quote_stats), device tensors.  The
        imbalance is taken over the first k levels (default: all recorded); lags: 1 .. 8 values >= 1, in steps."""
        from .depth import MAX_HIST_HALF, _lags
        self._need_depth("depth_imbalance()")
        first, n = self._market_range("depth_imbalance", first_market, n_markets)
        which = self._tape_which(episode)
        lg = _lags(lags, 1)
        k = self.depth_levels if k is None else int(k)
        if not 1 <= k <= self.depth_levels or not 1 <= int(half) <= MAX_HIST_HALF:
            raise ValueError(f"depth_imbalance: k must be in 1 .. {self.depth_levels} and half in 1 .. {MAX_HIST_HALF}, got {k}, {half}")
        return self._reader_call(lib().cda_depth_imbalance, "cda_depth_imbalance", first, n, (which, (C.c_int32 * len(lg))(*lg), len(lg), k, int(half)),
                                 (torch.empty((n, len(lg), 2 * int(half), 5), dtype=torch.int64, device=self.device),
                                  torch.empty((n, 4), dtype=torch.int64, device=self.device)))

    def depth_ofi(self, lags=(0, 1, 5), bar_steps=1, depths=(1,), episode="current", first_market=0, n_markets=None):
        """Multi-level order-flow imbalance joined to returns, bar by bar, of one remembered episode's held ladders, reduced on the device in one launch
        (include/cda.h cda_depth_ofi; depth.ofi_from_records is its specification, word for word).  -> (lagged i64 [n, n_depths, n_lags, 6] - depth.OFI_LAG_FIELDS
        per depth K and lag l >= 0 over the kept bars b whose return r_(b + l) is defined: n, q = sum OFI_b, r, qr, qq, rr -, base i64 [n, 4] - depth.OFI_FIELDS:
        pairs used, bars kept, bars excluded, saturated records -, info i32 [n, 4] as quote_stats), device tensors.  depths: 1 .. 4 values in 1 .. levels."""
        from .depth import MAX_DEPTHS, _lags
        self._need_depth("depth_ofi()")
        first, n = self._market_range("depth_ofi", first_market, n_markets)
        which = self._tape_which(episode)
        lg = _lags(lags, 0)
        dp = [int(x) for x in depths]
        if not 1 <= len(dp) <= MAX_DEPTHS or min(dp) < 1 or max(dp) > self.depth_levels:
            raise ValueError(f"depth_ofi: depths must be 1 .. {MAX_DEPTHS} values in 1 .. {self.depth_levels}, got {depths!r}")
        bar = self._stylised_points("depth_ofi", first, n, bar_steps)
        return self._reader_call(lib().cda_depth_ofi, "cda_depth_ofi", first, n, (which, (C.c_int32 * len(lg))(*lg), len(lg), bar, (C.c_int32 * len(dp))(*dp), len(dp)),
                                 (torch.empty((n, len(dp), len(lg), 6), dtype=torch.int64, device=self.device),
                                  torch.empty((n, 4), dtype=torch.int64, device=self.device)))

    # ------------------------------------------------------------------ the order tape: every decoded order of a step and its execution rank (order_tape.py)
    @property
    def order_tape_enabled(self):
        return int(lib().cda_order_tape_capacity(self._h)) > 0

    @property
    def order_tape_capacity(self):
        return int(lib().cda_order_tape_capacity(self._h))

    def enable_order_tape(self, capacity=1024):
        """From now on every step entry point first records, per market whose episode is not over, what the step's actions decode to - per agent type, side, size
        and price as the step's own `lob_actions` info words, and the rank the step's shuffle gives the order in the execution order (order_tape.record_dtype(A)) -
        into the market's ring of `capacity` records on the device (include/cda.h cda_order_tape_enable; a power of two), behind an attached order schedule's window
        and the quote and depth recorders and ahead of the step.  The recorder works on a copy of the market's generator: the step that follows is bit for bit the
        step an env without the tape takes.  Off by default; rings start empty; it needs no other tape (order_fills needs the trade tape too).  While it is on the
        one-launch policy step is off (rollout chains take their two-launch path) and run_random is refused.  Do not toggle it between the capture and the replay
        of a graph that holds this env's step launches (mlp.RolloutChains checks)."""
        capacity = int(capacity)
        if not 1 <= capacity <= (1 << 20) or capacity & (capacity - 1):
            raise ValueError(f"order tape capacity must be a power of two in 1 .. {1 << 20} steps, got {capacity}")
        self.sync()
        check(lib().cda_order_tape_enable(self._h, capacity), "cda_order_tape_enable")
        self.order_tape_epoch += 1                                # (captured graphs of this env's step launches are stale from here on)

    def disable_order_tape(self):
        self.sync()
        check(lib().cda_order_tape_disable(self._h), "cda_order_tape_disable")
        self.order_tape_epoch += 1

    def _need_order_tape(self, what):
        if not self.order_tape_enabled:
            raise RuntimeError(f"{what} needs the order tape: call enable_order_tape() first (it is off by default)")

    def order_tape_meta(self, first_market=0, n_markets=None):
        """Every market's meta row of the order tape as the readers see it - rolled to the market's clock by the episode rule (quotes.roll) - i32 [n, 8], a device
        tensor; quotes.meta_from_words names the words, quotes.span says what the ring holds of either episode."""
        self._need_order_tape("order_tape_meta()")
        first, n = self._market_range("order_tape_meta", first_market, n_markets)
        return self._reader_call(lib().cda_order_tape_meta, "cda_order_tape_meta", first, n, (), (torch.empty((n, 8), dtype=torch.int32, device=self.device),), info=False)[0]

    def order_tape_series(self, k=None, episode="current", first_market=0, n_markets=None):
        """The held order records of one remembered episode, oldest first (include/cda.h cda_order_tape_series): (records i32 [n, k, (1 + A) * 4] -
        order_tape.as_orders names the words; rows beyond the count are zero -, counts i32 [n], info i32 [n, 4] = records returned, records of the episode's head
        the ring had overwritten, step of the first returned record, partial flag), device tensors.  An episode longer than k returns its LAST k records.  k
        defaults to the smaller of the ring's capacity and the largest max_step."""
        self._need_order_tape("order_tape_series()")
        first, n = self._market_range("order_tape_series", first_market, n_markets)
        which = self._tape_which(episode)
        if k is None:
            k = max(1, min(self.order_tape_capacity, self._top_max_step()))
        if int(k) < 1:
            raise ValueError(f"order_tape_series: k must be >= 1, got {k}")
        return self._reader_call(lib().cda_order_tape_series, "cda_order_tape_series", first, n, (which, int(k)),
                                 (torch.empty((n, int(k), 4 * (1 + self.num_agents)), dtype=torch.int32, device=self.device),
                                  torch.empty(n, dtype=torch.int32, device=self.device)))

    def order_tape_episode(self, market=0, episode="current"):
        """One market's held order records of an episode, oldest first, as a structured host array (order_tape.record_dtype(A))."""
        from .order_tape import as_orders
        rec, cnt, _ = self.order_tape_series(None, episode, int(market), 1)
        return as_orders(rec[0, :int(cnt[0].item())].cpu().numpy(), self.num_agents).copy()

    def order_flow(self, episode="current", first_market=0, n_markets=None):
        """What every agent sent over one remembered episode's held order records, reduced on the device in one launch (include/cda.h cda_order_flow;
        order_tape.flow_from_records is its specification, word for word).  -> (flow i64 [n, A, 32] - order_tape.FLOW_FIELDS: steps present, passes, steps absent,
        per type x side orders and quantity, the placement classes of the limit orders against the touch -, info i32 [n, 4] as quote_stats), device tensors.
        Every word is additive: order_tape.pool sums over markets, order_tape.summary reads the ratios."""
        self._need_order_tape("order_flow()")
        first, n = self._market_range("order_flow", first_market, n_markets)
        which = self._tape_which(episode)
        return self._reader_call(lib().cda_order_flow, "cda_order_flow", first, n, (which,),
                                 (torch.empty((n, self.num_agents, 32), dtype=torch.int64, device=self.device),))

    def order_fills(self, episode="current", first_market=0, n_markets=None):
        """The trade tape of one remembered episode joined to its order records on the fill's step, reduced on the device in one launch (include/cda.h
        cda_order_fills; order_tape.fills_from_records is its specification, word for word).  Needs the trade tape as well.  -> (fills i64 [n, A, 24] -
        order_tape.FILL_FIELDS: per order type orders, submitted quantity, orders filled at once, quantity so filled; maker, self and unmatched fills -, info i32
        [n, 8] = order records held, lost, step of the first, partial, then fills held, lost, step of the first held fill (-1: none), partial), device tensors."""
        self._need_order_tape("order_fills()")
        self._need_tape("order_fills()")
        first, n = self._market_range("order_fills", first_market, n_markets)
        which = self._tape_which(episode)
        return self._reader_call(lib().cda_order_fills, "cda_order_fills", first, n, (which,),
                                 (torch.empty((n, self.num_agents, 24), dtype=torch.int64, device=self.device),
                                  torch.empty((n, 8), dtype=torch.int32, device=self.device)), info=False)

    # ------------------------------------------------------------------ the book report: reductions over the standing book, on the device
    def _book_call(self, name, first_market, n_markets, shape, dtype, *mid):
        first, n = self._market_range(name, first_market, n_markets)
        return self._reader_call(getattr(lib(), "cda_" + name), "cda_" + name, first, n, mid, (torch.empty((n,) + shape, dtype=dtype, device=self.device),), info=False)[0]

    def book_counts(self, first_market=0, n_markets=None):
        """Resting orders and distinct price levels of every side, tile and HBM ring together (include/cda.h cda_book_counts): i32 [n, 2, 2] =
        [market, side 0 bids / 1 asks, (orders, levels)], a device tensor.  Like every book_* reader: one launch on the caller's stream, ordered
        after every group's last step, no host synchronisation; book.py states the result in numpy (book.counts_from_orders)."""
        return self._book_call("book_counts", first_market, n_markets, (2, 2), torch.int32)

    def book_levels(self, max_levels, first_market=0, n_markets=None):
        """The Level-2 ladder of the WHOLE book, not only the observation's ten levels (cda_book_levels; book.levels_from_orders): i64 [n, 2, max_levels, 3]
        = (price, volume, orders) per level, best first; rows past a side's level count are zero.  1 <= max_levels <= 4096.  book.summary() reads spread,
        mid and imbalance off it."""
        from .book import _max_levels
        L = _max_levels(max_levels)
        return self._book_call("book_levels", first_market, n_markets, (2, L, 3), torch.int64, L)

    def book_impact(self, sizes, first_market=0, n_markets=None):
        """What a market order of each of `sizes` (1 .. 16 integers >= 1) would pay right now (cda_book_impact; book.impact_from_orders): i64 [n, 2, K, 3] =
        (filled, notional, last_price) for an order that consumes that side by price-time priority - side 0: the bids, hit by a sell; side 1: the asks, lifted
        by a buy; own resting orders included.  filled = min(size, the side's quantity), notional = sum of price x quantity over what is consumed, last_price =
        the price of the last order touched (0 on an empty side)."""
        from .book import _sizes
        q = _sizes(sizes)
        return self._book_call("book_impact", first_market, n_markets, (2, len(q), 3), torch.int64, (C.c_int64 * len(q))(*q), len(q))

    def book_agents(self, first_market=0, n_markets=None):
        """Every agent's resting orders (cda_book_agents; book.agents_from_orders): i64 [n, 2, A, 6] = (orders, quantity, notional, best_price, worst_price,
        ahead_qty) per side and agent; best / worst price = the prices of the agent's first / last own order in queue order, ahead_qty = the quantity resting
        strictly before its first own order; zeros for an agent with nothing on that side.  Bid + ask notional of an agent is its cash_on_hold."""
        return self._book_call("book_agents", first_market, n_markets, (2, self.num_agents, 6), torch.int64)

    def book_orders(self, first_market=0, n_markets=None):
        """The Level-3 dump of all markets in two launches (cda_book_offsets, cda_book_pack): (orders i32 [total, 5] - get_book()'s rows (price, qty, owner,
        order_id, timestamp), queue order -, offsets i64 [2 n + 1]): side s of market first_market + i owns rows offsets[2 i + s] : offsets[2 i + s + 1].
        Device tensors; the one host read is the 8-byte total.  book.split_orders() cuts them into per-market (bids, asks) pairs."""
        first, n = self._market_range("book_orders", first_market, n_markets)
        self.join()
        with torch.cuda.device(self.device):
            off = torch.empty(2 * n + 1, dtype=torch.int64, device=self.device)
            check(lib().cda_book_offsets(self._h, first, n, off.data_ptr(), self._stream()), "cda_book_offsets")
            total = int(off[2 * n].item())              # the one 8-byte read
            rows = torch.empty((total, 5), dtype=torch.int32, device=self.device)
            check(lib().cda_book_pack(self._h, first, n, off.data_ptr(), total, rows.data_ptr() if total else None, total, self._stream()), "cda_book_pack")
        return rows, off

    # ------------------------------------------------------------------ order streams: explicit orders into many markets in one launch (orders.py)
    def submit_orders(self, streams=None, *, offsets=None, msgs=None, first_market=0, n_markets=None, clear_step_counters=False, results=True, max_per_launch=65536,
                      max_len=None):
        """Play a list of explicit messages into every market of a range (include/cda.h cda_submit_orders): one asynchronous launch on the caller's stream, a wave
        per market, equivalent - bit for bit in the market's record - to place_order() / mark_to_mkt() once per valid message, in order.  No observation frame
        is pushed and t_step does not move: the next step() sees the book.  On a tape-enabled env the fills are recorded.
        streams: a list of n per-market sequences of (trader, type, side, size, price[, tag]) or ("mark",) (orders.pack) - or the packed form as tensors /
        arrays: offsets i64 [n + 1], msgs (orders.MSG_DTYPE, or uint8 / int32 rows of 16 bytes) with market first_market + i owning msgs[offsets[i] : offsets[i + 1]].
        A message outside the accepted domain (orders.valid) is skipped and reported; a market with an empty stream is not touched.
        clear_step_counters: clear every account's step counters behind a market's stream, so that seeded or exogenous flow does not reach the next step's reward terms.
        -> (results, summary): results int32 [total, 4] (orders.RESULT_DTYPE rows: status, n_fills, position_delta, resting_delta; None with results=False),
        summary int32 [n, 4] = (done, rejected, invalid, fills) per market, invalid = -1 for a market whose offsets are not a stream.  Device tensors.
        A stream longer than max_per_launch is played in successive launches of at most that many messages per market - the same final state and results -, so
        that no single launch runs unbounded.  max_len: the longest stream, when the caller knows it; for device offsets the default reads it back (8 bytes)."""
        from . import orders as OR
        first, n = self._market_range("submit_orders", first_market, n_markets)
        if int(max_per_launch) < 1:
            raise ValueError("max_per_launch must be >= 1")
        if streams is not None:
            if offsets is not None or msgs is not None:
                raise ValueError("submit_orders takes streams or (offsets, msgs), not both")
            if len(streams) != n:
                raise ValueError(f"{len(streams)} streams for {n} markets")
            offsets, msgs = OR.pack(streams)
        if offsets is None or msgs is None:
            raise ValueError("submit_orders needs streams or (offsets, msgs)")
        if isinstance(offsets, np.ndarray) or not isinstance(offsets, torch.Tensor):
            off_h = np.ascontiguousarray(np.asarray(offsets, np.int64))
            if max_len is None:
                max_len = int(np.diff(off_h).max()) if off_h.size > 1 else 0
            offsets = torch.from_numpy(off_h).to(self.device)
        if isinstance(msgs, np.ndarray):
            msgs = torch.from_numpy(np.ascontiguousarray(msgs).view(np.uint8).reshape(-1, 16)).to(self.device)
        if offsets.dtype != torch.int64 or offsets.numel() != n + 1 or offsets.device != self.device or not offsets.is_contiguous():
            raise ValueError(f"offsets must be a contiguous int64 [{n + 1}] tensor on {self.device}")
        if msgs.device != self.device or not msgs.is_contiguous() or (msgs.numel() * msgs.element_size()) % 16 != 0 or msgs.data_ptr() % 16 != 0:
            raise ValueError(f"msgs must be a contiguous, 16-byte aligned tensor of 16-byte messages on {self.device}")
        total = msgs.numel() * msgs.element_size() // 16
        if max_len is None:
            max_len = int((offsets[1:] - offsets[:-1]).max().item())
        self.host_epoch += 1
        self.join()
        flags = OR.CLEAR_STEP_COUNTERS if clear_step_counters else 0
        step = int(max_per_launch)
        with torch.cuda.device(self.device):
            res = torch.zeros((max(total, 1), 4), dtype=torch.int32, device=self.device)[:total] if results else None
            summary = None
            for skip in range(0, max(int(max_len), 1), step):
                part = torch.empty((n, 4), dtype=torch.int32, device=self.device)
                check(lib().cda_submit_orders_window(self._h, first, n, offsets.data_ptr(), msgs.data_ptr() if total else offsets.data_ptr(), total, skip, step,
                                                     res.data_ptr() if results and total else None, part.data_ptr(), flags, self._stream()), "cda_submit_orders")
                if summary is None:
                    summary = part
                else:                                          # (a market whose offsets are not a stream says -1 in every window)
                    summary = torch.where(summary[:, 2:3] < 0, summary, summary + part)
        return res, summary

    def seed_books(self, bids, asks, market=None, first_market=0, n_markets=None):
        """Start markets from a non-empty book: get_book() / book_orders() rows of ONE market (price, qty, owner, order_id, timestamp; queue order) rebuilt by limit
        orders (orders.from_book) in market `market`, or - market=None - in every market of [first_market, first_market + n_markets), in one launch, with the step
        counters cleared behind them.  Prices, quantities, owners and queue positions are the dump's; ids and timestamps are new; the escrow is taken from
        the target accounts, and an order its account cannot afford is rejected (see the returned summary).  Meant for freshly reset markets.  -> (results, summary)
        of submit_orders."""
        from . import orders as OR
        stream = OR.from_book(bids, asks)
        if market is not None:
            first_market, n_markets = int(market), 1
        first, n = self._market_range("seed_books", first_market, n_markets)
        _, one = OR.pack([stream])
        L = len(one)
        msgs = torch.from_numpy(one.view(np.uint8).reshape(-1, 16)).to(self.device).repeat(n, 1)
        offsets = torch.arange(n + 1, dtype=torch.int64, device=self.device) * L
        return self.submit_orders(offsets=offsets, msgs=msgs, first_market=first, n_markets=n, clear_step_counters=True, max_len=L)

    # ------------------------------------------------------------------ order schedules: per-step order flow played inside steps and rollouts (orders.py)
    @property
    def order_schedule(self):
        """whether an order schedule is attached"""
        return self._schedule is not None

    @property
    def schedule_epoch(self):
        """moved by every set_order_schedule / clear_order_schedule (cda_schedule_epoch): graphs captured on this env's step launches hold the schedule launch (or
        none) and the tables of the epoch they were captured under"""
        return int(lib().cda_schedule_epoch(self._h))

    def order_schedule_digest(self):
        """orders.schedule_digest of the attached schedule, None while nothing is attached (what a training checkpoint keeps)"""
        return self._schedule.digest if self._schedule is not None else None

    def set_order_schedule(self, schedule, market_schedule=None, loop=False, clear_step_counters=False):
        """Attach an order schedule (include/cda.h cda_schedule_attach): from now on every step - step(), run_scripted(), the rollout / evaluation / league chains -
        first plays, per market, the window of the market's current t_step into it, through the matching code of place_order(), then steps.  Window 0 is the
        seed book of every episode (the device-side auto reset included), windows 1 .. are background flow ahead of the step's own orders.
        schedule: rows[r][t] = the messages of step t of row r (orders.pack_schedule), or an orders.PackedSchedule.
        market_schedule: int [N], market i plays row market_schedule[i], -1 = none; None = market i plays row i % n_sched.
        loop: t_step wraps around the schedule's S windows; without it a step beyond them plays nothing.
        clear_step_counters: clear every account's step counters behind a played window (as submit_orders); off, a scheduled fill reaches the step's reward
        terms like any fill inside the step.
        A schedule replaces the one attached; the counters (order_schedule_counts) restart.  While attached run_random() raises and the one-launch policy
        step is off."""
        from . import orders as OR
        packed = schedule if isinstance(schedule, OR.PackedSchedule) else OR.pack_schedule(schedule)
        N = self.n_markets
        so = (np.arange(N) % packed.n_sched).astype(np.int32) if market_schedule is None else np.ascontiguousarray(np.asarray(
            market_schedule.detach().cpu().numpy() if hasattr(market_schedule, "detach") else market_schedule).astype(np.int64))
        if so.shape != (N,):
            raise ValueError(f"market_schedule must have shape {(N,)}, got {so.shape}")
        why = OR.schedule_check(packed, so, self.num_agents)
        if why is not None:
            raise ValueError(f"not an order schedule: {why}")
        so = so.astype(np.int32)
        so_t = torch.from_numpy(so).to(self.device)
        off_t = torch.from_numpy(packed.step_offsets).to(self.device)
        total = len(packed.msgs)
        msg_t = torch.from_numpy(np.ascontiguousarray(packed.msgs).view(np.uint8).reshape(-1, 16).copy()).to(self.device) if total else torch.zeros((1, 16), dtype=torch.uint8, device=self.device)
        flags = (OR.SCHEDULE_LOOP if loop else 0) | (OR.SCHEDULE_CLEAR_STEP_COUNTERS if clear_step_counters else 0)
        self.sync()
        with torch.cuda.device(self.device):
            check(lib().cda_schedule_attach(self._h, so_t.data_ptr(), off_t.data_ptr(), packed.n_sched, packed.n_steps, msg_t.data_ptr(), total, flags), "cda_schedule_attach")
        self._schedule = AttachedSchedule(so_t, off_t, msg_t, packed, so, bool(loop), bool(clear_step_counters), OR.schedule_digest(packed, so, loop, clear_step_counters))

    def load_order_schedule(self, path):
        """set_order_schedule from a file of orders.save_schedule (the command lines' --order-schedule): the file's row table - by default market i plays row
        i % n_sched - and flags"""
        from . import orders as OR
        packed, ms, loop, clear = OR.load_schedule(path)
        if ms is not None and len(ms) != self.n_markets:
            raise ValueError(f"{path}: market_schedule names rows for {len(ms)} markets, the env has {self.n_markets}")
        self.set_order_schedule(packed, market_schedule=ms, loop=loop, clear_step_counters=clear)

    def clear_order_schedule(self):
        self.sync()
        check(lib().cda_schedule_detach(self._h), "cda_schedule_detach")
        self._schedule = None

    def order_schedule_counts(self, first_market=0, n_markets=None):
        """i64 [n, 4] (device) = messages done, rejected, invalid, fills the attached schedule played into every market since it was attached (cda_schedule_counts)"""
        first, n = self._market_range("order_schedule_counts", first_market, n_markets)
        self.join()
        out = torch.empty((n, 4), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().cda_schedule_counts(self._h, first, n, out.data_ptr(), self._stream()), "cda_schedule_counts")
        return out

    def play_order_schedule(self, first_market=0, n_markets=None):
        """The launch every step issues first, on its own (cda_schedule_play): every market's window of its current t_step, on the caller's stream; nothing
        attached: nothing happens.  For tests and custom loops - a step() behind it plays the same window again."""
        first, n = self._market_range("play_order_schedule", first_market, n_markets)
        self.host_epoch += 1
        self.join()
        with torch.cuda.device(self.device):
            check(lib().cda_schedule_play(self._h, first, n, self._stream()), "cda_schedule_play")

    # ------------------------------------------------------------------ scripted opponents: rule-based agents on the device (scripted.py states the laws)
    @property
    def scripted(self):
        return self._script is not None

    def set_scripted(self, slot_script, profiles, seed=0, market_index_base=0):
        """Attach scripted opponents (include/cda.h cda_scripted_attach): slot_script int [N, A], 0 = the slot is not scripted, 1 + k = it plays profiles[k];
        profiles: 1 .. 16 scripted.Profile objects (or names / 'NAME:key=value' strings).  `seed` keys the taker's draws, market_index_base + market is the
        market's index in them.  The two tables become resident tensors the env keeps; rollout chains and run_scripted() then play the laws.  While attached
        the one-launch policy step is off (cda_policy_step_supported answers 0); ppo.train_fused trains on the env only when told the trained slots (trained_slots=k)
        and the league attaches its own (train_league_fused(scripted_opponents=...))."""
        from .scripted import MAX_PROFILES, parse_profile, profiles_array
        profs = [parse_profile(p) for p in profiles]
        if not 1 <= len(profs) <= MAX_PROFILES:
            raise ValueError(f"between 1 and {MAX_PROFILES} profiles, got {len(profs)}")
        slots = np.ascontiguousarray(np.asarray(slot_script.detach().cpu().numpy() if hasattr(slot_script, "detach") else slot_script).astype(np.int64))
        if slots.shape != (self.n_markets, self.num_agents):
            raise ValueError(f"slot_script must have shape {(self.n_markets, self.num_agents)}, got {slots.shape}")
        if slots.min() < 0 or slots.max() > len(profs):
            raise ValueError(f"slot_script values must lie in 0 .. {len(profs)} (0 = not scripted, 1 + k = profile k)")
        slot_t = torch.from_numpy(slots.astype(np.int32)).to(self.device)
        prof_t = torch.from_numpy(profiles_array(profs).view(np.uint8).reshape(len(profs), 64).copy()).to(self.device)
        self.sync()
        with torch.cuda.device(self.device):
            check(lib().cda_scripted_attach(self._h, slot_t.data_ptr(), prof_t.data_ptr(), len(profs), int(seed) & (2 ** 64 - 1), int(market_index_base) & (2 ** 64 - 1)),
                  "cda_scripted_attach")
        self._script = AttachedScripts(slot_t, prof_t, profs, int(seed) & (2 ** 64 - 1), int(market_index_base) & (2 ** 64 - 1), slots.astype(np.int32))
        self.script_epoch += 1

    def clear_scripted(self):
        self.sync()
        check(lib().cda_scripted_detach(self._h), "cda_scripted_detach")
        self._script = None
        self.script_epoch += 1

    def scripted_slots(self):
        """the attached slot table as a host array i32 [N, A] (zeros while nothing is attached)"""
        return self._script.slots_host if self._script is not None else np.zeros((self.n_markets, self.num_agents), np.int32)

    def scripted_slot_tensor(self):
        """the RESIDENT slot table i32 [N, A] on the device - the one k_script_actions reads at every step.  Rewriting it in place (values 0 .. the number of
        attached profiles; the league's per-episode assignment does, cda_league_assign_scripted) changes who plays the scripts from the next step on without a
        re-attach: the script epoch, and graphs captured on it, hold.  scripted_slots() stays the table as attached."""
        if self._script is None:
            raise RuntimeError("scripted_slot_tensor() needs scripted opponents: call set_scripted() first")
        return self._script.slot_script

    def scripted_profiles(self):
        return list(self._script.profiles) if self._script is not None else []

    def _action_buffers(self):
        N, A, dev = self.n_markets, self.num_agents, self.device
        return {"category": torch.zeros((N, A), dtype=torch.int32, device=dev), "size_mean": torch.zeros((N, A), dtype=torch.float32, device=dev),
                "size_sigma": torch.zeros((N, A), dtype=torch.float32, device=dev), "price": torch.zeros((N, A), dtype=torch.int32, device=dev),
                "price_offset": torch.ones((N, A), dtype=torch.int32, device=dev)}

    def scripted_actions(self, draw=0, counter=0, out=None, first_market=0, n_markets=None):
        """Every scripted slot's action of the markets' state NOW (include/cda.h cda_scripted_actions; scripted.actions_from_views is its specification): one
        launch on the caller's stream, ordered after every group's last step, no host synchronisation.  out: a dict of the five [N, A] action tensors (ACTION_KEYS;
        optionally 'a_cont' f32 [N, A, 2], 'logp' f32 [N, A], 'record' f32 [N, A, 8]) written in place where a slot is scripted and left alone elsewhere; None =
        fresh tensors holding a pass everywhere else.  counter: an int, or an i64 [1] device tensor read on the device.  Nothing attached: nothing is written."""
        return self._law_actions("cda_scripted_actions", "scripted_actions", draw, counter, out, first_market, n_markets)

    def _law_actions(self, entry, what, draw, counter, out, first_market, n_markets):
        """scripted_actions / stateful_actions: the shared argument checks and the one native call (`entry`: cda_scripted_actions or cda_stateful_actions)"""
        first, n = self._market_range(what, first_market, n_markets)
        if out is None:
            out = self._action_buffers()
        dts = {"category": torch.int32, "size_mean": torch.float32, "size_sigma": torch.float32, "price": torch.int32, "price_offset": torch.int32,
               "a_cont": torch.float32, "logp": torch.float32, "record": torch.float32}
        per = {"a_cont": 2, "record": 8}
        for k, t in out.items():
            if k in dts:
                assert t.dtype == dts[k] and t.is_contiguous() and t.device == self.device and t.numel() == self.n_markets * self.num_agents * per.get(k, 1), k
        if isinstance(counter, torch.Tensor):
            assert counter.dtype == torch.int64 and counter.device == self.device and counter.numel() >= 1
            ctr = counter
        elif int(counter) == 0:
            ctr = None
        else:
            ctr = torch.tensor([int(counter)], dtype=torch.int64, device=self.device)
        self.join()
        opt = lambda k: out[k].data_ptr() if k in out else None     # noqa: E731
        with torch.cuda.device(self.device):
            check(getattr(lib(), entry)(self._h, first, n, ctr.data_ptr() if ctr is not None else None, int(draw), *(out[k].data_ptr() for k in ACTION_KEYS),
                                        opt("a_cont"), opt("logp"), opt("record"), self._stream()), entry)
        if ctr is not None:
            ctr.record_stream(torch.cuda.current_stream(self.device))
        return out

    def run_scripted(self, n_steps, others="pass", action_seed=0, draw0=None):
        """Step the env n_steps times with every scripted slot playing its law: per step {the other slots' actions, cda_scripted_actions, step}, all on the
        device, no host synchronisation inside the loop.  others: what the slots that are not scripted play - 'pass', or 'random' = the uniform random stream
        (random_actions_device keyed action_seed and the draw number).  The taker's draw number of step k is draw0 + k; draw0 = None continues where the last
        run_scripted stopped.  Returns step()'s tuple of the last step."""
        if self._script is None and self._stateful is None:
            raise RuntimeError("run_scripted() needs scripted opponents: call set_scripted() (or set_stateful()) first")
        if others not in ("pass", "random"):
            raise ValueError(f"others must be 'pass' or 'random', got {others!r}")
        d = int(getattr(self, "_script_draw", 0) if draw0 is None else draw0)
        acts = self._action_buffers()
        base = (self._script if self._script is not None else self._stateful).market_index_base
        ret = None
        for k in range(int(n_steps)):
            if others == "random":
                with torch.cuda.device(self.device):
                    check(lib().cda_random_actions(int(action_seed) & (2 ** 64 - 1), base, d + k, 1, self.n_markets, self.num_agents,
                                                   *(acts[key].data_ptr() for key in ACTION_KEYS), self._stream()), "cda_random_actions")
            if self._script is not None:
                self.scripted_actions(draw=d + k, out=acts)
            if self._stateful is not None:                            # (behind the stateless family, as the rollout chains order them)
                self.stateful_actions(draw=d + k, out=acts)
            ret = self.step(acts)
        self._script_draw = d + int(n_steps)
        return ret

    # ------------------------------------------------------------------ the label tap: a law's answer for slots it does not play (DAgger; imitate.dagger)
    def _label_tables(self, slot_label, profiles):
        from .scripted import MAX_PROFILES, parse_profile, profiles_array
        profs = [parse_profile(p) for p in profiles]
        if not 1 <= len(profs) <= MAX_PROFILES:
            raise ValueError(f"between 1 and {MAX_PROFILES} profiles, got {len(profs)}")
        slots = np.ascontiguousarray(np.asarray(slot_label.detach().cpu().numpy() if hasattr(slot_label, "detach") else slot_label).astype(np.int64))
        if slots.shape != (self.n_markets, self.num_agents):
            raise ValueError(f"slot_label must have shape {(self.n_markets, self.num_agents)}, got {slots.shape}")
        if slots.min() < 0 or slots.max() > len(profs):
            raise ValueError(f"slot_label values must lie in 0 .. {len(profs)} (0 = not labelled, 1 + k = profile k)")
        slot_t = torch.from_numpy(slots.astype(np.int32)).to(self.device)
        prof_t = torch.from_numpy(profiles_array(profs).view(np.uint8).reshape(len(profs), 64).copy()).to(self.device)
        return profs, slots.astype(np.int32), slot_t, prof_t

    def set_label_tap(self, slot_label, profiles, rows, seed=0, market_index_base=0, mix=0.0):
        """Attach a label tap (include/cda.h cda_label_tap_attach): slot_label int [N, A], 0 = the slot is not labelled, 1 + k = profiles[k] (scripted.parse_profile's
        forms) is asked about it at every step of a rollout chain - about the slot's own position and resting orders, whoever plays it.  The answers land in row t of the
        tap's buffers, so chains of a horizon up to `rows` may run.  label_tap is then a dict of what the env owns: 'category', 'size_mean', 'size_sigma', 'price',
        'price_offset', 'played' [rows, N, A], 'mix_q32' (i64 [1]: the device word), the resident tables 'slot_label' i32 [N, A] and 'profiles' u8 [n, 64], and 'rows',
        'seed', 'market_index_base', 'profile_list' (the Profiles), 'slots_host'.  mix = beta in [0, 1]: a labelled slot that is not
        scripted plays its label with that probability (label_tap['played'] says where); set_label_mix changes it in place.  `seed` / market_index_base key the label
        law's draws and the mixing draw.  While attached the one-launch policy step is off.  Not saved by checkpoints or snapshots; single-process runs only."""
        from .scripted import mix_q32_of
        rows = int(rows)
        if rows < 1:
            raise ValueError("the tap needs at least one row")
        q = mix_q32_of(mix)
        profs, slots, slot_t, prof_t = self._label_tables(slot_label, profiles)
        N, A, dev = self.n_markets, self.num_agents, self.device
        tap = {k: torch.zeros((rows, N, A), dtype=torch.float32 if k in ("size_mean", "size_sigma") else torch.int32, device=dev) for k in ACTION_KEYS + ("played",)}
        tap["mix_q32"] = torch.tensor([q], dtype=torch.int64, device=dev)
        seed, base = int(seed) & (2 ** 64 - 1), int(market_index_base) & (2 ** 64 - 1)
        self.sync()
        with torch.cuda.device(dev):
            check(lib().cda_label_tap_attach(self._h, slot_t.data_ptr(), prof_t.data_ptr(), len(profs), seed, base, tap["mix_q32"].data_ptr(), rows,
                                             *(tap[k].data_ptr() for k in ACTION_KEYS), tap["played"].data_ptr()), "cda_label_tap_attach")
        tap.update(slot_label=slot_t, profiles=prof_t, rows=rows, seed=seed, market_index_base=base, profile_list=profs, slots_host=slots)
        self.label_tap = tap
        self.label_epoch += 1

    def set_label_mix(self, beta):
        """beta in [0, 1]: the probability with which a labelled, unscripted slot plays its label from the next launch on - an in-place write of the device word the
        kernel reads, so captured graphs follow it and label_epoch does not move"""
        from .scripted import mix_q32_of
        if self.label_tap is None:
            raise RuntimeError("set_label_mix() needs a label tap: call set_label_tap() first")
        self.label_tap["mix_q32"].fill_(mix_q32_of(beta))

    def clear_label_tap(self):
        self.sync()
        check(lib().cda_label_tap_detach(self._h), "cda_label_tap_detach")
        self.label_tap = None
        self.label_epoch += 1

    def label_actions(self, slot_label, profiles, seed=0, counter=0, draw=0, market_index_base=0, out=None, first_market=0, n_markets=None):
        """What profiles[slot_label - 1] would do in every labelled slot's place NOW (include/cda.h cda_label_actions; scripted.label_spec states it): one launch, no
        tap needed, no mixing, the env's actions untouched.  out: a dict of the five [N, A] action tensors, written only where slot_label names a profile; None = fresh
        tensors holding a pass elsewhere.  counter: an int, or an i64 [1] device tensor.  (seed, counter, market_index_base + market, draw, agent) key the law's draws."""
        first, n = self._market_range("label_actions", first_market, n_markets)
        profs, _slots, slot_t, prof_t = self._label_tables(slot_label, profiles)
        if out is None:
            out = self._action_buffers()
        dts = {"category": torch.int32, "size_mean": torch.float32, "size_sigma": torch.float32, "price": torch.int32, "price_offset": torch.int32}
        for k in ACTION_KEYS:
            t = out[k]
            assert t.dtype == dts[k] and t.is_contiguous() and t.device == self.device and t.numel() == self.n_markets * self.num_agents, k
        if isinstance(counter, torch.Tensor):
            assert counter.dtype == torch.int64 and counter.device == self.device and counter.numel() >= 1
            ctr = counter
        else:
            ctr = None if int(counter) == 0 else torch.tensor([int(counter)], dtype=torch.int64, device=self.device)
        self.join()
        with torch.cuda.device(self.device):
            check(lib().cda_label_actions(self._h, first, n, slot_t.data_ptr(), prof_t.data_ptr(), len(profs), int(seed) & (2 ** 64 - 1), int(market_index_base) & (2 ** 64 - 1),
                                          ctr.data_ptr() if ctr is not None else None, int(draw), *(out[k].data_ptr() for k in ACTION_KEYS), self._stream()), "cda_label_actions")
        cur = torch.cuda.current_stream(self.device)
        for t in (slot_t, prof_t) + ((ctr,) if ctr is not None else ()):
            t.record_stream(cur)
        return out

    # ------------------------------------------------------------------ scripted opponents with memory: trend, value, execution (stateful.py states the laws)
    @property
    def stateful(self):
        return self._stateful is not None

    def set_stateful(self, slot_table, profiles, seed=0, market_index_base=0):
        """Attach stateful opponents (include/cda.h cda_stateful_attach): slot_table int [N, A], 0 = the slot is not stateful, 1 + k = it plays profiles[k];
        profiles: 1 .. 16 stateful.Profile objects (or names / 'NAME:key=value' strings).  The two tables and a ZEROED state tensor i64 [N, A, 4] (stateful_state())
        become resident tensors the env keeps; rollout chains and run_scripted() then play the laws, behind the stateless family's launch.  `seed` keys the value law's
        draws, market_index_base + market is the market's index in them.  A slot that set_scripted names at this moment is refused (ValueError).  While attached the
        one-launch policy step is off.  A snapshot() does not carry the state: clone stateful_state() beside it and copy_ it back after restore()."""
        from .stateful import MAX_PROFILES, STATE_WORDS, parse_profile, profiles_array
        profs = [parse_profile(p) for p in profiles]
        if not 1 <= len(profs) <= MAX_PROFILES:
            raise ValueError(f"between 1 and {MAX_PROFILES} profiles, got {len(profs)}")
        slots = np.ascontiguousarray(np.asarray(slot_table.detach().cpu().numpy() if hasattr(slot_table, "detach") else slot_table).astype(np.int64))
        if slots.shape != (self.n_markets, self.num_agents):
            raise ValueError(f"slot_table must have shape {(self.n_markets, self.num_agents)}, got {slots.shape}")
        if slots.min() < 0 or slots.max() > len(profs):
            raise ValueError(f"slot_table values must lie in 0 .. {len(profs)} (0 = not stateful, 1 + k = profile k)")
        if self._script is not None and bool(((slots != 0) & (self._script.slots_host != 0)).any()):
            raise ValueError("a slot is named by set_scripted and by set_stateful: a slot plays one family (clear_scripted() or re-attach the scripts without it)")
        slot_t = torch.from_numpy(slots.astype(np.int32)).to(self.device)
        prof_t = torch.from_numpy(profiles_array(profs).view(np.uint8).reshape(len(profs), 64).copy()).to(self.device)
        state_t = torch.zeros((self.n_markets, self.num_agents, STATE_WORDS), dtype=torch.int64, device=self.device)
        self.sync()
        with torch.cuda.device(self.device):
            check(lib().cda_stateful_attach(self._h, slot_t.data_ptr(), prof_t.data_ptr(), len(profs), state_t.data_ptr(), int(seed) & (2 ** 64 - 1),
                                            int(market_index_base) & (2 ** 64 - 1)), "cda_stateful_attach")
        self._stateful = AttachedStateful(slot_t, prof_t, state_t, profs, int(seed) & (2 ** 64 - 1), int(market_index_base) & (2 ** 64 - 1), slots.astype(np.int32))
        self.stateful_epoch += 1

    def clear_stateful(self):
        self.sync()
        check(lib().cda_stateful_detach(self._h), "cda_stateful_detach")
        self._stateful = None
        self.stateful_epoch += 1

    def stateful_slots(self):
        """the attached stateful slot table as a host array i32 [N, A] (zeros while nothing is attached)"""
        return self._stateful.slots_host if self._stateful is not None else np.zeros((self.n_markets, self.num_agents), np.int32)

    def stateful_profiles(self):
        return list(self._stateful.profiles) if self._stateful is not None else []

    def stateful_state(self):
        """the RESIDENT state tensor i64 [N, A, 4] - the one k_stateful_actions reads and writes at every step (word 0: last t_step | tag << 32).  A caller clones it
        and copy_s the clone back to carry the slots' memory across snapshot() / restore(); zeroing it makes every slot start fresh at its next step."""
        if self._stateful is None:
            raise RuntimeError("stateful_state() needs stateful opponents: call set_stateful() first")
        return self._stateful.state

    def stateful_actions(self, draw=0, counter=0, out=None, first_market=0, n_markets=None):
        """Every stateful slot's state advanced on the markets' state NOW, and its action (include/cda.h cda_stateful_actions; stateful.play is its specification): one
        launch, scripted_actions' arguments and conventions.  A second call before the next step changes nothing and answers the same.  Nothing attached: nothing is
        written."""
        return self._law_actions("cda_stateful_actions", "stateful_actions", draw, counter, out, first_market, n_markets)

    # ------------------------------------------------------------------ snapshots, forks and resumable runs
    def snapshot(self, first=0, n=None):
        """A compact device image of markets [first, first + n) (include/cda.h cda_snapshot_*): their records, done bytes, episode-metric rows and the
        live windows of their HBM rings.  Returns a snapshot.Snapshot (uint8 device tensor + parsed header).  Ordered after every group's last step."""
        from .snapshot import Snapshot, parse_header
        n = self.n_markets - int(first) if n is None else int(n)
        if not (0 <= int(first) and n >= 1 and int(first) + n <= self.n_markets):
            raise ValueError(f"snapshot range [{first}, {int(first) + n}) is outside the env's {self.n_markets} markets")
        self.join()
        with torch.cuda.device(self.device):
            off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
            check(lib().cda_snapshot_offsets(self._h, int(first), n, off.data_ptr(), self._stream()), "cda_snapshot_offsets")
            total = int(off[n].item())                  # the one 8-byte read
            blob = torch.empty(total, dtype=torch.uint8, device=self.device)
            check(lib().cda_snapshot_pack(self._h, int(first), n, off.data_ptr(), blob.data_ptr(), total, self._stream()), "cda_snapshot_pack")
            header = parse_header(blob[:256].cpu())
        return Snapshot(blob, header, market_params=self.market_rows(int(first), n) if self.per_market else None)

    def restore(self, snap, first=0, src_first=0, n=None):
        """Markets [src_first, src_first + n) of `snap` -> markets [first, first + n) of this env (a Snapshot from this env or another with the same
        numeric config, tile, history depth, agents and episode-metrics setting; book_spill may differ).  The arena is written in place and the restored
        markets' observation rows of `obs` are re-emitted.  A mismatch raises ValueError naming the field; a blob the device check refuses raises
        CDAError - in both cases before any byte of the env is written."""
        from .snapshot import mismatch
        n = len(snap) - int(src_first) if n is None else int(n)
        if not (0 <= int(src_first) and n >= 1 and int(src_first) + n <= len(snap)):
            raise ValueError(f"source range [{src_first}, {int(src_first) + n}) is outside the snapshot's {len(snap)} markets")
        if not (0 <= int(first) and int(first) + n <= self.n_markets):
            raise ValueError(f"target range [{first}, {int(first) + n}) is outside the env's {self.n_markets} markets")
        why = mismatch(snap.header, self)
        if why is not None:
            raise ValueError(f"cannot restore this snapshot: {why}")
        # the restored markets' rows: the snapshot's (validated against this env first), else - for an env with rows of its own - the env's config
        rows = None
        if snap.market_params is not None:
            from .market_params import rows_from_numpy, validate_rows
            rows = rows_from_numpy(snap.market_params[int(src_first):int(src_first) + n])
            validate_rows(self.config, rows)
        elif self.per_market:
            from .market_params import rows_of
            rows = rows_of(self.config, [{}] * n)
        blob = snap.blob
        if blob.device != self.device or blob.data_ptr() % 256 != 0:
            blob = blob.to(self.device).clone()
        self.host_epoch += 1
        self.join()
        with torch.cuda.device(self.device):
            check(lib().cda_snapshot_restore(self._h, int(first), blob.data_ptr(), int(snap.nbytes), int(src_first), n, self.obs.data_ptr(), self._stream()),
                  "cda_snapshot_restore")
        blob.record_stream(torch.cuda.current_stream(self.device))     # (the allocator keeps it until the restore has run on this stream; nothing is held beyond)
        if rows is not None:
            self._write_rows(int(first), rows)          # (after the device's checks passed: a refused blob leaves the rows too as they were)
        if self.groups > 1:
            self.fork()                                 # the group streams see the restored markets
        return self.obs

    def state_bytes_per_market(self):
        return int(lib().cda_state_bytes_per_market(self._h))

    def nav_decimals(self):
        """info['nav'] as exact decimal.Decimal objects, [N][A] nested lists (host copy)."""
        raw = self.info["nav"].cpu().numpy().view(DEC_DTYPE).reshape(self.n_markets, self.num_agents)
        return [[K.dec_to_decimal(raw[i, a]) for a in range(self.num_agents)] for i in range(self.n_markets)]


def selftest_dec(op, a, b=None, device=0):
    """Device self-test of the ledger arithmetic: numpy DEC_DTYPE arrays in/out."""
    a = np.ascontiguousarray(a)
    out = np.zeros(len(a), DEC_DTYPE)
    bp = None if b is None else np.ascontiguousarray(b).ctypes.data
    check(lib().cda_selftest_dec(device, op, len(a), a.ctypes.data, bp, out.ctypes.data), "cda_selftest_dec")
    return out


def selftest_rng(seed, lo, hi, n_steps, n_normals, perm_n, device=0):
    first = np.zeros(2, np.int32)
    normals = np.zeros((n_steps, n_normals), np.float64)
    perms = np.zeros((n_steps, max(perm_n, 1)), np.int32)
    fs = np.zeros(8, np.uint64)
    perm_arg = perms[:, :perm_n].copy() if perm_n else perms
    check(lib().cda_selftest_rng(device, seed, lo, hi, n_steps, n_normals, perm_n, first.ctypes.data,
                                 normals.ctypes.data, perm_arg.ctypes.data, fs.ctypes.data), "cda_selftest_rng")
    return int(first[0]), normals, perm_arg[:, :perm_n], fs


def selftest_libm(op, x, device=0):
    """The restated libm function (op 0: log1p, 1: exp) on the DEVICE (device >= 0) or by the same source compiled for the
    host (device=None; needs no GPU): float64 numpy in / out."""
    x = np.ascontiguousarray(x, np.float64)
    y = np.zeros_like(x)
    if device is None:
        check(lib().cda_selftest_libm_host(op, len(x), x.ctypes.data, y.ctypes.data), "cda_selftest_libm_host")
    else:
        check(lib().cda_selftest_libm(device, op, len(x), x.ctypes.data, y.ctypes.data), "cda_selftest_libm")
    return y
