"""Behaviour cloning on the fused network (include/cda_imitate.h): demonstrations, their negative log-likelihood, pretraining.

A rollout records the five env action tensors of EVERY slot - the scripted opponents' (scripted.py) like the policy's - next to the one observation row per
market-step.  `Demonstrations` packs those actions into sample records (cda_bc_records: labels, raw Gaussian targets, a weight per sample); `BCUpdate` is
mlp.FusedUpdate's separate-kernel minibatch step with cda_bc_loss_records in the loss position - the network kernels (forward, backward, weight gradients, Adam)
are the PPO update's own, so every compiled variant (history depth, activation, vf_share_layers) trains; `pretrain` clones scripted experts (or distils a teacher
policy) into a policy that `ppo.train_fused(policy=...)`, the league and `evaluate` take as it is; `dagger` clones an expert from its LABELS of the learner's own states (the
env's label tap, csrc/cda_scripted_label.inc), aggregated in a `DaggerBuffer`.

`records_spec` and `bc_loss_spec` are the numpy / float64 statements of the two kernels (importable without a GPU): what the tests hold the kernels to.

    python -m gym_continuousdoubleauction_amd.imitate --expert maker --markets 1024 --agents 4 --iters 8 --horizon 64 --save maker.pt
    python -m gym_continuousdoubleauction_amd.imitate --dagger --label-expert maker --opponent taker --beta 0.5 --iters 8 --horizon 64 --save maker.pt
"""
import argparse
import contextlib
import json
import math

import numpy as np
import torch

from .mlp import FusedUpdate, NOUT, _check, _lib, _stream

N_CAT, N_PRICE, N_OFF = 9, 10, 3                      # include/cda_learner.h CDA_HEAD_*
SRC_NONE, SRC_ENV, SRC_POLICY = 0, 1, 2               # include/cda_imitate.h CDA_BC_SRC_*
SQUASH_BOUND = 1.0 - 2.0 ** -10                       # include/cda_imitate.h CDA_BC_SQUASH_BOUND
DEMO_FORMAT, DEMO_VERSION = "cda-demonstrations", 1
_LOG_2PI = math.log(2.0 * math.pi)


# ---- the two kernels, stated in numpy ----------------------------------------------------------------------------------------------------
def _slot_tables(slot_src, slot_weight, N, A):
    src = np.asarray(slot_src, dtype=np.int32).reshape(N, A)
    w = np.ones((N, A), np.float32) if slot_weight is None else np.asarray(slot_weight, dtype=np.float32).reshape(N, A)
    return src, w


def records_spec(category, price, price_offset, size_mean, size_sigma, a_cont, slot_src, slot_weight=None, rec=None):
    """cda_bc_records on the host: the five env action arrays [T, N, A] (+ a_cont [T, N, A, 2] or None) and the slot tables [N, A] -> (rec f32 [T, N, A, 8], stats
    f64[2] = the sum of the written weights, the samples with weight > 0).  rec (optional): the records before the launch - words 6, 7 are kept (zeros otherwise).
    The inverse squash is taken in float64 of the float32 action clamped to the bound, then rounded to float32."""
    cat = np.asarray(category, dtype=np.int32)
    T, N, A = cat.shape
    src, w = _slot_tables(slot_src, slot_weight, N, A)
    if a_cont is None and bool((src == SRC_POLICY).any()):
        raise ValueError("slot_src names policy samples (2) but there is no a_cont to copy them from")
    out = np.zeros((T, N, A, 8), np.float32) if rec is None else np.array(rec, dtype=np.float32, copy=True).reshape(T, N, A, 8)
    words = out.view(np.int32)
    words[..., 0], words[..., 1], words[..., 2] = cat, np.asarray(price, dtype=np.int32), np.asarray(price_offset, dtype=np.int32)
    M = np.float32(SQUASH_BOUND)
    m = np.clip(np.asarray(size_mean, dtype=np.float32), -M, M).astype(np.float64)
    s = np.clip(np.asarray(size_sigma, dtype=np.float32), np.float32(1.0) - M, M).astype(np.float64)
    x0, x1 = np.arctanh(m).astype(np.float32), (np.log(s) - np.log1p(-s)).astype(np.float32)
    if a_cont is not None:
        pol = np.broadcast_to(src == SRC_POLICY, (T, N, A))
        ac = np.asarray(a_cont, dtype=np.float32).reshape(T, N, A, 2)
        x0, x1 = np.where(pol, ac[..., 0], x0), np.where(pol, ac[..., 1], x1)
    weight = np.broadcast_to(np.where((src == SRC_ENV) | (src == SRC_POLICY), w, np.float32(0.0)).astype(np.float32), (T, N, A))
    out[..., 3], out[..., 4], out[..., 5] = x0, x1, weight
    return out, np.array([weight.astype(np.float64).sum(), float((weight > 0).sum())])


def _log_softmax(l):
    z = l - l.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def bc_loss_spec(outputs, log_std, rec, row_index=None, vf_coef=0.0, ent_coef=0.0, loss_scale=1.0, norm_rows=0):
    """cda_bc_loss_records in float64: outputs [R, stride] (24 policy columns | value | padding), log_std [2], rec f32 [*, A, 8] (cda_bc_records' layout: word 5 the
    weight, word 7 the return), row_index (optional) the record row of every output row.  Returns (d_out f64 [R, stride], sums5 f64[5], logp f64 [R, A], bc_stats
    f64[8]) as include/cda_imitate.h defines them: sums5[0..2] carry loss_scale (the finishing step divides by B = (norm_rows or R) * A: `out6_spec`), sums5[3..4]
    are dL / d log_std."""
    o = np.asarray(outputs, dtype=np.float64)
    R, stride = o.shape
    rec = np.ascontiguousarray(np.asarray(rec, dtype=np.float32))
    A = rec.shape[1]
    rr = np.ascontiguousarray(rec[np.arange(R) if row_index is None else np.asarray(row_index, dtype=np.int64)])
    lab = rr.view(np.int32)
    ls = np.asarray(log_std, dtype=np.float64).reshape(2)
    w, x, ret = rr[..., 5].astype(np.float64), rr[..., 3:5].astype(np.float64), rr[..., 7].astype(np.float64)
    B = (int(norm_rows) or R) * A
    k = float(loss_scale) / B
    g, W = -k * w, w.sum(1)
    d = np.zeros((R, stride))
    logp = np.full((R, A), -ls[0] - ls[1] - _LOG_2PI)
    H = np.full(R, 1.0 + _LOG_2PI + ls[0] + ls[1])
    stats = np.zeros(8)
    stats[0], stats[6] = w.sum(), float((w > 0).sum())
    for word, (lo, n) in enumerate(((0, N_CAT), (N_CAT, N_PRICE), (N_CAT + N_PRICE, N_OFF))):
        lp = _log_softmax(o[:, lo:lo + n])
        pr = np.exp(lp)
        h = -(pr * lp).sum(-1)
        c = np.clip(lab[..., word], 0, n - 1)                                   # pick<>'s clamp
        logp += np.take_along_axis(lp, c, axis=1)
        H += h
        onehot = c[..., None] == np.arange(n)
        d[:, lo:lo + n] = (g[..., None] * onehot).sum(1) - g.sum(1, keepdims=True) * pr + ent_coef * k * W[:, None] * pr * (lp + h[:, None])
        stats[1 + word] = (w * (c == o[:, lo:lo + n].argmax(-1)[:, None])).sum()
    err = x - o[:, None, 22:24]
    z = err * np.exp(-ls)
    logp -= 0.5 * (z ** 2).sum(-1)
    d[:, 22:24] = (g[..., None] * z * np.exp(-ls)).sum(1)
    dv = o[:, None, 24] - ret
    d[:, 24] = (2.0 * vf_coef * k * w * dv).sum(1)
    dls = (g[..., None] * (z ** 2 - 1.0)).sum((0, 1)) - ent_coef * k * w.sum()
    stats[4], stats[5] = (w * err[..., 0] ** 2).sum(), (w * err[..., 1] ** 2).sum()
    sums5 = np.array([loss_scale * (-w * logp).sum(), loss_scale * (w * dv ** 2).sum(), loss_scale * (w * H[:, None]).sum(), dls[0], dls[1]])
    return d, sums5, logp, stats


def out6_spec(sums5, samples, vf_coef=0.0, ent_coef=0.0):
    """what the finishing step makes of the sums: [nll, v_loss, entropy, loss, d log_std 0, d log_std 1]"""
    nll, vl, en = (float(sums5[q]) / samples for q in range(3))
    return np.array([nll, vl, en, nll + vf_coef * vl - ent_coef * en, sums5[3], sums5[4]])


# ---- demonstrations ------------------------------------------------------------------------------------------------------------------------
def pack_records(category, price, price_offset, size_mean, size_sigma, a_cont, slot_src, slot_weight=None, rec=None):
    """cda_bc_records on device tensors: the five action tensors [T, N, A] (i32, i32, i32, f32, f32), a_cont f32 [T, N, A, 2] or None, and the HOST tables slot_src i32 /
    slot_weight f32 [N, A] -> (rec f32 [T, N, A, 8], stats f64[2] on the device).  rec (optional): written in place, words 6, 7 untouched.  ValueError: a policy-sample
    slot (2) without a_cont."""
    T, N, A = category.shape
    dev = category.device
    src, w = _slot_tables(slot_src, slot_weight, N, A)
    if a_cont is None and bool((src == SRC_POLICY).any()):
        raise ValueError("slot_src names policy samples (2) but there is no a_cont to copy them from")
    for t, dt in ((category, torch.int32), (price, torch.int32), (price_offset, torch.int32), (size_mean, torch.float32), (size_sigma, torch.float32)):
        if t.dtype != dt or t.shape != (T, N, A) or not t.is_contiguous() or t.device != dev:
            raise ValueError("the action tensors are contiguous [T, N, A] on one device: category / price / price_offset int32, size_mean / size_sigma float32")
    if a_cont is not None and (a_cont.dtype != torch.float32 or a_cont.shape != (T, N, A, 2) or not a_cont.is_contiguous()):
        raise ValueError("a_cont is a contiguous float32 [T, N, A, 2]")
    if rec is None:
        rec = torch.zeros((T, N, A, 8), dtype=torch.float32, device=dev)
    elif rec.dtype != torch.float32 or rec.numel() != T * N * A * 8 or not rec.is_contiguous():
        raise ValueError("rec is a contiguous float32 [T, N, A, 8]")
    src_d, w_d = torch.from_numpy(np.ascontiguousarray(src)).to(dev), torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    stats = torch.zeros(2, dtype=torch.float64, device=dev)
    _check(_lib().cda_bc_records(category.data_ptr(), price.data_ptr(), price_offset.data_ptr(), size_mean.data_ptr(), size_sigma.data_ptr(),
                                 a_cont.data_ptr() if a_cont is not None else None, src_d.data_ptr(), w_d.data_ptr(), T, N, A, rec.data_ptr(), stats.data_ptr(),
                                 _stream(dev)), "cda_bc_records")
    return rec, stats


class Demonstrations:
    """obs f32 [R, OBS] (one row per market-step, step-major: row t * n_markets + m) and rec f32 [R, A, 8] (cda_bc_records' records), with the sum of the
    weights and the number of counted samples."""

    def __init__(self, obs, rec, n_markets, weight_sum=None, count=None):
        if obs.dim() != 2 or rec.dim() != 3 or rec.shape[0] != obs.shape[0] or rec.shape[2] != 8 or obs.shape[0] % int(n_markets):
            raise ValueError("demonstrations: obs [R, OBS], rec [R, A, 8], R a multiple of n_markets")
        self.obs, self.rec, self.n_markets = obs.contiguous(), rec.contiguous(), int(n_markets)
        if weight_sum is None or count is None:
            w = self.rec[..., 5].double()
            weight_sum, count = float(w.sum()), int((w > 0).sum())
        self.weight_sum, self.count = float(weight_sum), int(count)

    R = property(lambda self: self.obs.shape[0])
    A = property(lambda self: self.rec.shape[1])
    T = property(lambda self: self.obs.shape[0] // self.n_markets)

    @property
    def loss_scale(self):
        """1 / (the expected weight of a sample): what makes the loss of a shuffled minibatch the mean over its counted samples in expectation"""
        if self.weight_sum <= 0.0:
            raise ValueError("these demonstrations hold no counted sample (every weight is 0)")
        return self.R * self.A / self.weight_sum

    @classmethod
    def from_rollout(cls, chains, slot_src, slot_weight=None, with_returns=False):
        """the last run() of a mlp.RolloutChains as demonstrations: one cda_bc_records launch over its action buffers.  slot_src / slot_weight: host tables [N, A]
        (0 = not counted, 1 = an env action - a scripted slot's -, 2 = a sample of the rollout's policy, copied from a_cont).  with_returns: words ADV, RET are copied from
        the rollout's own records (after RolloutChains.gae), for a value term; zeros otherwise."""
        b, T, N, A = chains.buf, chains.T, chains.N, chains.A
        rec = torch.zeros((T, N, A, 8), dtype=torch.float32, device=chains.device)
        if with_returns:
            rec[..., 6:8] = b["record"][..., 6:8]
        rec, stats = pack_records(b["category"], b["price"], b["price_offset"], b["size_mean"], b["size_sigma"], b["a_cont"], slot_src, slot_weight, rec=rec)
        s = stats.cpu()
        return cls(b["obs"][:T].reshape(T * N, -1).clone(), rec.view(T * N, A, 8), N, float(s[0]), int(s[1]))

    @classmethod
    def from_labels(cls, chains, tap, slot_src, slot_weight=None):
        """the last run() of a mlp.RolloutChains on an env with a label tap (CDAVecEnv.label_tap) as demonstrations: the chain's observations with the tap's LABELS - what
        the label law would have done in each slot's place - in the position of the actions: one cda_bc_records launch over rows 0 .. T - 1 of the label buffers.
        slot_src / slot_weight: host tables [N, A], 1 (an env action: the label's five words) where a labelled slot counts, 0 elsewhere; a label is no policy sample, so
        2 is refused."""
        T, N, A = chains.T, chains.N, chains.A
        if T > int(tap["rows"]):
            raise ValueError(f"the tap holds {tap['rows']} rows, the rollout {T} steps")
        if bool((np.asarray(slot_src) == SRC_POLICY).any()):
            raise ValueError("labels are env actions (slot_src 1): there is no raw Gaussian sample to copy for slot_src 2")
        rec, stats = pack_records(tap["category"][:T], tap["price"][:T], tap["price_offset"][:T], tap["size_mean"][:T], tap["size_sigma"][:T], None, slot_src, slot_weight)
        s = stats.cpu()
        return cls(chains.buf["obs"][:T].reshape(T * N, -1).clone(), rec.view(T * N, A, 8), N, float(s[0]), int(s[1]))

    def save(self, path):
        with open(path, "wb") as fh:                                            # (a file object: numpy appends no suffix to the name)
            np.savez(fh, format=DEMO_FORMAT, version=DEMO_VERSION, obs=self.obs.cpu().numpy(), rec=self.rec.cpu().numpy(), n_markets=self.n_markets,
                     weight_sum=self.weight_sum, count=self.count)

    @classmethod
    def load(cls, path, device):
        with np.load(path) as z:
            if str(z["format"]) != DEMO_FORMAT or int(z["version"]) != DEMO_VERSION:
                raise ValueError(f"{path} is not a {DEMO_FORMAT} file of version {DEMO_VERSION}")
            return cls(torch.from_numpy(z["obs"]).to(device), torch.from_numpy(z["rec"]).to(device), int(z["n_markets"]), float(z["weight_sum"]), int(z["count"]))

    def split(self, frac, seed=0):
        """(train, held-out): round(frac * n_markets) markets (at least one, never all), drawn with `seed`, are held out with all their steps"""
        N = self.n_markets
        n_held = min(N - 1, max(1, int(round(float(frac) * N))))
        if N < 2:
            raise ValueError("a split needs at least two markets")
        order = np.random.default_rng(int(seed)).permutation(N)
        parts = []
        for idx in (np.sort(order[n_held:]), np.sort(order[:n_held])):
            ix = torch.from_numpy(idx).to(self.obs.device)
            obs = self.obs.view(self.T, N, -1)[:, ix].reshape(self.T * len(idx), -1)
            rec = self.rec.view(self.T, N, self.A, 8)[:, ix].reshape(self.T * len(idx), self.A, 8)
            parts.append(Demonstrations(obs, rec, len(idx)))
        return tuple(parts)


class DaggerBuffer:
    """DAgger's aggregate D <- D u D_i at a fixed size: `capacity_iters` blocks of `rows_per_iter` rows each, block j % capacity_iters holding the j-th set of
    demonstrations added (the oldest is overwritten once the buffer is full).  Rows not yet filled carry weight 0 - a loss skips them, and Demonstrations.loss_scale
    normalises by the weight sum - so a BCUpdate is built ONCE, at the full size, and `demos` is always the whole buffer.  weight_sum and count are those of the
    concatenation of the blocks it holds.  Plain tensors: device="cpu" needs no GPU."""

    def __init__(self, capacity_iters, rows_per_iter, num_agents, obs_dim, n_markets, device="cpu"):
        self.K, self.rows, self.A, self.n_markets = int(capacity_iters), int(rows_per_iter), int(num_agents), int(n_markets)
        if self.K < 1 or self.rows < 1 or self.rows % self.n_markets:
            raise ValueError("a DaggerBuffer holds capacity_iters >= 1 blocks of rows_per_iter rows, a multiple of n_markets")
        self.obs = torch.zeros((self.K * self.rows, int(obs_dim)), dtype=torch.float32, device=device)
        self.rec = torch.zeros((self.K * self.rows, self.A, 8), dtype=torch.float32, device=device)
        self.added = 0
        self._weight, self._count = [0.0] * self.K, [0] * self.K

    filled = property(lambda self: min(self.added, self.K))

    def add(self, demos):
        """copy one iteration's demonstrations into the next block (wrapping); returns the block's index"""
        if demos.R != self.rows or demos.A != self.A or demos.obs.shape[1] != self.obs.shape[1] or demos.n_markets != self.n_markets:
            raise ValueError(f"this buffer takes blocks of {self.rows} rows x {self.A} agents of {self.obs.shape[1]}-float observations over {self.n_markets} markets")
        j = self.added % self.K
        self.obs[j * self.rows:(j + 1) * self.rows].copy_(demos.obs)
        self.rec[j * self.rows:(j + 1) * self.rows].copy_(demos.rec)
        self._weight[j], self._count[j] = demos.weight_sum, demos.count
        self.added += 1
        return j

    @property
    def demos(self):
        """the whole buffer as Demonstrations (views, no copy): block-major, the unfilled blocks at weight 0"""
        return Demonstrations(self.obs, self.rec, self.n_markets, float(sum(self._weight)), int(sum(self._count)))


# ---- the update ---------------------------------------------------------------------------------------------------------------------------
def _figures(out6, bc_stats):
    """what run / step / evaluate report: nll, v_loss, entropy (out6), the three agreement rates, the two mean squared target errors, the weight and count (bc_stats)"""
    o, b = out6.detach().cpu().double(), bc_stats.detach().cpu()
    W = float(b[0]) or math.nan
    return {"nll": float(o[0]), "v_loss": float(o[1]), "entropy": float(o[2]), "agree_category": float(b[1]) / W, "agree_price": float(b[2]) / W,
            "agree_offset": float(b[3]) / W, "mse_mean": float(b[4]) / W, "mse_sigma": float(b[5]) / W, "weight": float(b[0]), "count": int(b[6])}


class BCUpdate(FusedUpdate):
    """mlp.FusedUpdate's separate-kernel minibatch step (fused=False: prep_rows per epoch, then forward, loss, backward, weight gradients, Adam) with
    cda_bc_loss_records in the loss position: its buffers, its permutation, its step - only the loss launch differs.  n_rows, rows_mb: multiples of 32; run() trains on
    the leading n_rows rows of the demonstrations it is given.  A policy with the state-dependent log-std head is refused: the separate kernels do not train it."""

    def __init__(self, policy, n_rows, rows_mb, num_agents, sub_batches=1, chunks=None):
        if bool(getattr(policy, "state_dependent_log_std", False)):
            raise ValueError("behaviour cloning runs the separate update kernels, which do not train the state-dependent log-std head: clone into a policy with a free log_std vector")
        super().__init__(policy, n_rows, rows_mb, num_agents, chunks=chunks, sub_batches=sub_batches, fused=False)
        self.bc_stats = torch.zeros(8, dtype=torch.float64, device=policy.device)
        self.loss_scale = 1.0

    def _loss_records(self, records, first, n_rows, norm_rows, clip, vf_coef, ent_coef, clear, finish, st):
        rec = records[0]
        _check(_lib().cda_bc_loss_records(self.out.data_ptr(), self.p.theta.data_ptr() + self.L.OFF_LS * 4, rec if isinstance(rec, int) else rec.data_ptr(),
                                          self.perm.data_ptr() + first * 8, n_rows, self.A, NOUT, float(vf_coef), float(ent_coef), float(self.loss_scale),
                                          self.d_out.data_ptr(), self.sums5.data_ptr(), self.out6.data_ptr(), norm_rows, clear, finish, None, self.bc_stats.data_ptr(), st),
               "cda_bc_loss_records")

    def _take(self, demos):
        if demos.R < self.R or demos.A != self.A or demos.obs.shape[1] != self.L.OBS:
            raise ValueError(f"this update was built for {self.R} rows x {self.A} agents of {self.L.OBS}-float observations")
        self.loss_scale = demos.loss_scale
        return demos.obs[:self.R], (demos.rec, None, 0)

    def step(self, demos, first=0, rows=None, lr=1e-3, vf_coef=0.0, ent_coef=0.0, betas=(0.9, 0.999), eps=1e-8, max_norm=math.inf, apply=True, perm=None):
        """ONE minibatch step on rows perm[first .. first + rows) of the demonstrations (perm: i64 [n_rows], default the identity).  apply=False: no optimiser step -
        the gradient is reduced into self.grad and the statistics into self.out6, theta and the Adam state stay as they are."""
        obs, records = self._take(demos)
        rows = self.rows_mb if rows is None else int(rows)
        dev = self.p.device
        self.perm.copy_(torch.arange(self.R, device=dev) if perm is None else perm)
        _check(self.L.fn("cda_mlp_prep_rows")(obs.data_ptr(), self.perm.data_ptr(), self.R, self.x_rm.data_ptr(), self.x_pk.data_ptr(), _stream(dev)), "cda_mlp_prep_rows")
        self.bc_stats.zero_()
        chunks, tiles = self.minibatch_step(first, rows, None, None, None, None, 0.0, vf_coef, ent_coef, lr, betas, eps, max_norm, apply=apply, records=records)
        if not apply:
            _check(self.L.fn("cda_mlp_reduce")(self.slab.data_ptr(), chunks, self.bias_slab.data_ptr(), tiles, self.sums5.data_ptr(), rows * self.A, float(vf_coef), float(ent_coef),
                                               0.0, self.out6.data_ptr(), self.p.adam_step.data_ptr(), self.grad.data_ptr(), self.norm2.data_ptr(), _stream(dev)), "cda_mlp_reduce")
        return _figures(self.out6, self.bc_stats)

    def run(self, demos, epochs=4, lr=1e-3, vf_coef=0.0, ent_coef=0.0, betas=(0.9, 0.999), eps=1e-8, max_norm=math.inf, perms=None):
        """`epochs` shuffled passes over the leading n_rows rows of `demos`, one optimiser step per minibatch.  Returns nll, entropy, v_loss, agree_category / agree_price /
        agree_offset, mse_mean / mse_sigma (+ weight, count): nll, v_loss and entropy are the LAST minibatch step's (as FusedUpdate.run reports its losses), the three agreement rates (the heads' modes against the labels) and the
        two mean squared target errors are over the last epoch."""
        obs, records = self._take(demos)
        for ep in range(int(epochs)):
            self.bc_stats.zero_()
            FusedUpdate.run(self, obs, epochs=1, clip=0.0, vf_coef=vf_coef, ent_coef=ent_coef, lr=lr, betas=betas, eps=eps, max_norm=max_norm,
                            perms=None if perms is None else perms[ep:ep + 1], records=records)
        return _figures(self.out6, self.bc_stats)

    def evaluate(self, demos, vf_coef=0.0, ent_coef=0.0):
        """the figures of run() for the policy as it is, over ALL rows of `demos`, plus `loglik` - the weighted mean log-likelihood of the demonstrations, taken from the
        kernel's per-sample log-probabilities: one forward pass and the loss kernel, no optimiser step."""
        if demos.A != self.A or demos.obs.shape[1] != self.L.OBS:
            raise ValueError(f"this update was built for {self.A} agents of {self.L.OBS}-float observations")
        dev, R = self.p.device, demos.R
        out = self.p.forward(demos.obs)
        d_out, logp = torch.empty_like(out), torch.empty((R, self.A), dtype=torch.float32, device=dev)
        sums, out6, stats = torch.zeros(5, dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.float32, device=dev), torch.zeros(8, dtype=torch.float64, device=dev)
        _check(_lib().cda_bc_loss_records(out.data_ptr(), self.p.theta.data_ptr() + self.L.OFF_LS * 4, demos.rec.data_ptr(), None, R, self.A, NOUT, float(vf_coef),
                                          float(ent_coef), float(demos.loss_scale), d_out.data_ptr(), sums.data_ptr(), out6.data_ptr(), 0, 1, 1, logp.data_ptr(),
                                          stats.data_ptr(), _stream(dev)), "cda_bc_loss_records")
        w = demos.rec[..., 5].double()
        fig = _figures(out6, stats)
        fig["loglik"] = float((w * logp.double()).sum() / w.sum())
        return fig


# ---- pretraining ---------------------------------------------------------------------------------------------------------------------------
def _rows_mb(n_rows, num_agents, minibatch):
    return max(32, min(n_rows, (max(1, int(minibatch) // num_agents) // 32) * 32))


def fit(policy, demos, iters=1, epochs=4, lr=1e-3, holdout=0.125, seed=0, minibatch=65536, vf_coef=0.0, ent_coef=0.0, log=print):
    """clone recorded demonstrations into `policy`: `iters` x `epochs` passes over the training markets, the held-out markets (Demonstrations.split) evaluated around
    every iteration.  Returns the history (a list of {"iter", "train", "held_before", "held"})."""
    train, held = demos.split(holdout, seed) if holdout else (demos, None)
    n_rows = train.R // 32 * 32
    if n_rows < 32:
        raise ValueError("behaviour cloning needs at least 32 market-steps of demonstrations")
    upd = BCUpdate(policy, n_rows, _rows_mb(n_rows, train.A, minibatch), train.A)
    history = []
    for it in range(int(iters)):
        before = upd.evaluate(held) if held is not None else None
        h = {"iter": it, "train": upd.run(train, epochs=epochs, lr=lr, vf_coef=vf_coef, ent_coef=ent_coef), "held_before": before,
             "held": upd.evaluate(held) if held is not None else None}
        history.append(h)
        log(json.dumps(h))
    return history


def pretrain(env, experts=None, learner_slots=1, iters=8, horizon=64, epochs=4, lr=1e-3, seed=0, policy=None, hidden=(256, 256), activation="tanh", vf_share_layers=False,
             holdout=0.125, log=print, teacher=None, minibatch=65536, vf_coef=0.0, ent_coef=0.0, chains=4, use_graph=True, keep=None):
    """Clone scripted experts - or distil a teacher policy - into a policy, on rollouts of `env` (a HIP CDAVecEnv with auto_reset; it is reset with `seed`).
    experts = [spec, ...] (scripted.parse_profile's forms): attached for the run as ppo.train_fused(opponents=...) attaches them - slot learner_slots + j of market m plays
    experts[(m + j) % P] - and detached on exit.  Per iteration: one rollout of `horizon` steps in which the LEARNER's current policy plays the leading learner_slots
    slots (so the states drift towards the ones it will meet), the scripted slots' actions packed as demonstrations (slot_src 1, weight 1), `epochs` passes of
    BCUpdate.run over the training markets, and an evaluation on the held-out markets (`holdout`: their share, Demonstrations.split with `seed` - the same markets
    every iteration).
    teacher (a FusedPolicy or a policy file): distillation - the teacher plays the leading slots in the learner's place (every slot when there are no experts) and its
    samples are the demonstrations there (slot_src 2: the raw Gaussian samples of a_cont).
    policy: the learner (default: a fresh FusedPolicy of `hidden` / `activation` / `vf_share_layers` at the env's history depth); one with the state-dependent log-std
    head is refused (ValueError, before anything runs).  Single process.  keep (a dict, optional): receives the last iteration's `train` / `held` demonstrations, the
    `update` and the `rollout`.  Returns (FusedPolicy, history): history[i] = {"iter", "train": BCUpdate.run's figures, "held_before" / "held": BCUpdate.evaluate's on the
    held-out markets before / after the iteration's update}."""
    from . import scripted as SC
    from .mlp import FusedPolicy, RolloutChains, load_policy
    if experts is None and teacher is None:
        raise ValueError("pretrain needs demonstrations: experts=[...] (scripted opponents), teacher=policy, or both")
    if getattr(env, "scripted", False):
        raise ValueError("pretrain attaches its own scripted experts for the run: it needs an env without scripts attached (clear_scripted() first)")
    dev, N, A, T = env.obs.device, env.n_markets, env.num_agents, int(horizon)
    if policy is None:
        policy = FusedPolicy(dev, seed=seed, n_hist=env.n_hist, hidden=hidden, activation=activation, vf_share_layers=vf_share_layers)
    if bool(getattr(policy, "state_dependent_log_std", False)):
        raise ValueError("behaviour cloning runs the separate update kernels, which do not train the state-dependent log-std head: clone into a policy with a free log_std vector")
    if isinstance(teacher, str):
        teacher = load_policy(teacher, dev)
    k = int(learner_slots)
    slot_src = np.zeros((N, A), np.int32)
    attach = contextlib.nullcontext()
    if experts is not None:
        profiles = [SC.parse_profile(e) for e in experts]
        if not profiles:
            raise ValueError("experts: None or a non-empty list of scripted opponents")
        attach = SC.attached(env, SC.opponent_slots(N, A, k, len(profiles)), profiles, seed=seed)
        slot_src[:, k:] = SRC_ENV
        if teacher is not None:
            slot_src[:, :k] = SRC_POLICY
    else:
        slot_src[:] = SRC_POLICY
    env.reset(seed=seed)
    history, upd = [], None
    with attach:
        roll = RolloutChains(env, teacher if teacher is not None else policy, T, groups=chains, seed=seed, use_graphs=use_graph, trained_slots=k if experts is not None else None)
        for it in range(int(iters)):
            roll.run()
            train, held = Demonstrations.from_rollout(roll, slot_src).split(holdout, seed)
            if upd is None:
                n_rows = train.R // 32 * 32
                if n_rows < 32:
                    raise ValueError("behaviour cloning needs at least 32 market-steps of training demonstrations per iteration")
                upd = BCUpdate(policy, n_rows, _rows_mb(n_rows, A, minibatch), A)
            before = upd.evaluate(held)
            h = {"iter": it, "train": upd.run(train, epochs=epochs, lr=lr, vf_coef=vf_coef, ent_coef=ent_coef), "held_before": before, "held": upd.evaluate(held)}
            history.append(h)
            log(json.dumps(h))
        if keep is not None:
            keep.update(train=train, held=held, update=upd, rollout=roll, slot_src=slot_src)
    return policy, history


def dagger(env, label_expert, opponents=None, learner_slots=1, iters=8, horizon=64, beta=1.0, beta_decay=0.5, aggregate=None, label_opponents=False, epochs=4, lr=1e-3,
           seed=0, policy=None, hidden=(256, 256), activation="tanh", vf_share_layers=False, holdout=0.125, log=print, minibatch=65536, chains=4, use_graph=True, keep=None):
    """DAgger (Ross, Gordon & Bagnell 2011) on the device: clone `label_expert` (a scripted.parse_profile spec) from labels of the LEARNER's own states.  pretrain()'s
    demonstrations are the expert's answers to the expert's situation; here a label tap (CDAVecEnv.set_label_tap) asks the law, inside every step of the captured
    rollout chains, what it would do in the learner's slot - with the learner's position, resting orders and place in the queue.
    The learner plays the leading learner_slots slots of every market.  The slots behind them play `opponents` ([spec, ...]), attached as pretrain attaches experts -
    slot learner_slots + j of market m plays opponents[(m + j) % P] -, or the league's uniform random module when opponents is None.  The tap labels the leading slots
    with label_expert and, with label_opponents, every opponent slot with its own profile (its label is then its action).  Iteration i: set_label_mix(beta *
    beta_decay ** i) - with that probability a learner slot plays the label instead of its sample (label_tap['played']) -, one rollout of `horizon` steps, the labels
    packed as demonstrations (Demonstrations.from_labels), the training markets' share added to a DaggerBuffer of `aggregate` iterations (None: all `iters`, the
    classic aggregate), `epochs` passes of ONE BCUpdate over the buffer, and the evaluation of this iteration's held-out markets (`holdout`) before and after.
    Scripts and tap are detached on exit.  Returns (FusedPolicy, history): history[i] = {"iter", "beta", "train", "held_before", "held", "on_policy_agreement"} - the
    last one the share of learner-slot samples with played == 0 whose executed category equals the label (reduced on the device; NaN when every sample was mixed in,
    as at beta = 1).  Out of scope: a tap on the league chains' update, in checkpoints and snapshots, on the dict facades, data-parallel runs; a policy with the
    state-dependent log-std head is refused."""
    from . import scripted as SC
    from .mlp import LEAGUE_RANDOM, FusedPolicy, PolicyBank, RolloutChains
    if getattr(env, "scripted", False) or getattr(env, "label_tap", None) is not None:
        raise ValueError("dagger attaches its own scripted opponents and label tap for the run: it needs an env without either (clear_scripted() / clear_label_tap() first)")
    dev, N, A, T, k = env.obs.device, env.n_markets, env.num_agents, int(horizon), int(learner_slots)
    if not 1 <= k <= A or (opponents is not None and k > A - 1):
        raise ValueError(f"learner_slots must lie in 1 .. num_agents{' - 1' if opponents is not None else ''}, got {k}")
    if not (0.0 <= float(beta) <= 1.0 and 0.0 <= float(beta_decay) <= 1.0):
        raise ValueError("beta and beta_decay lie in [0, 1]")
    if policy is None:
        policy = FusedPolicy(dev, seed=seed, n_hist=env.n_hist, hidden=hidden, activation=activation, vf_share_layers=vf_share_layers)
    if bool(getattr(policy, "state_dependent_log_std", False)):
        raise ValueError("behaviour cloning runs the separate update kernels, which do not train the state-dependent log-std head: clone into a policy with a free log_std vector")
    expert = SC.parse_profile(label_expert)
    tap_profiles, slot_label = [expert], np.zeros((N, A), np.int32)
    slot_label[:, :k] = 1
    attach, bank = contextlib.nullcontext(), None
    if opponents is not None:
        opp = [SC.parse_profile(o) for o in opponents]
        if not opp:
            raise ValueError("opponents: None (random modules) or a non-empty list of scripted opponents")
        opp_slots = SC.opponent_slots(N, A, k, len(opp))
        attach = SC.attached(env, opp_slots, opp, seed=seed)
        if label_opponents:
            if 1 + len(opp) > SC.MAX_PROFILES:
                raise ValueError(f"label_opponents: the tap's table holds the expert and the opponents, at most {SC.MAX_PROFILES} profiles")
            tap_profiles += opp
            slot_label[:, k:] = 1 + opp_slots[:, k:]
    elif label_opponents:
        raise ValueError("label_opponents needs scripted opponents: a random module has no law to label with")
    else:                                                                      # the league chain: bank row 0 = the learner (refreshed from `policy` ahead of every rollout)
        bank = PolicyBank(dev, N, A, 1, max_frozen=0, seed=seed, random_seed=seed, n_hist=policy.L.hist, activation=policy.activation, vf_share_layers=policy.vf_share_layers)
        slot_net = np.full((N, A), LEAGUE_RANDOM, np.int32)
        slot_net[:, :k] = 0
        bank.set_slots(torch.from_numpy(slot_net))
    slot_src = (slot_label != 0).astype(np.int32) * SRC_ENV
    K = int(iters) if aggregate is None else int(aggregate)
    if K < 1:
        raise ValueError("aggregate: None or the number of iterations the buffer holds, at least 1")
    env.reset(seed=seed)
    history, upd, buf = [], None, None
    with attach:
        env.set_label_tap(slot_label, tap_profiles, rows=T, seed=seed, mix=beta)
        try:
            tap = env.label_tap
            roll = RolloutChains(env, bank if bank is not None else policy, T, groups=chains, seed=seed, use_graphs=use_graph)
            for it in range(int(iters)):
                b = float(beta) * float(beta_decay) ** it
                env.set_label_mix(b)
                if bank is not None:
                    bank.theta[0].copy_(policy.theta); bank.wb[0].copy_(policy.wb)
                roll.run()
                on = tap["played"][:T, :, :k] == 0
                hit = (on & (roll.buf["category"][:, :, :k] == tap["category"][:T, :, :k])).sum().double() / on.sum().double()
                train, held = Demonstrations.from_labels(roll, tap, slot_src).split(holdout, seed)
                if upd is None:
                    buf = DaggerBuffer(K, train.R, A, train.obs.shape[1], train.n_markets, device=dev)
                    n_rows = buf.obs.shape[0] // 32 * 32
                    if n_rows < 32:
                        raise ValueError("DAgger needs at least 32 market-steps of training demonstrations in its buffer")
                    upd = BCUpdate(policy, n_rows, _rows_mb(n_rows, A, minibatch), A)
                buf.add(train)
                before = upd.evaluate(held)
                h = {"iter": it, "beta": b, "train": upd.run(buf.demos, epochs=epochs, lr=lr), "held_before": before, "held": upd.evaluate(held),
                     "on_policy_agreement": float(hit)}
                history.append(h)
                log(json.dumps(h))
            if keep is not None:
                keep.update(train=train, held=held, update=upd, rollout=roll, buffer=buf, slot_src=slot_src, slot_label=slot_label)
        finally:
            if env.label_tap is not None:
                env.clear_label_tap()
    return policy, history


def main(argv=None, parse_only=False):
    """parse_only: return the parsed arguments without touching a device (the flags' tests)"""
    p = argparse.ArgumentParser(description="clone scripted experts (or recorded demonstrations, or a teacher policy) into a policy file")
    p.add_argument("--expert", action="append", default=None, metavar="SPEC", help="a scripted expert ('pass', 'maker', 'taker', 'imbalance', 'NAME:key=value,...'); repeat for several "
                                                                                   "(slot K + j of market m plays expert (m + j) mod P)")
    p.add_argument("--teacher", default=None, metavar="FILE", help="distil this policy file: it plays the leading slots (every slot without --expert) and its samples are demonstrations")
    p.add_argument("--learner-slots", type=int, default=1, metavar="K", help="the leading slots per market that the learner (or the teacher) plays")
    p.add_argument("--markets", type=int, default=1024)
    p.add_argument("--agents", type=int, default=4)
    p.add_argument("--iters", type=int, default=8)
    p.add_argument("--horizon", type=int, default=64)
    p.add_argument("--epochs", type=int, default=4)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--max-step", type=int, default=4096)
    p.add_argument("--n-hist", type=int, default=4)
    p.add_argument("--holdout", type=float, default=0.125, help="share of the markets held out for evaluation")
    p.add_argument("--minibatch", type=int, default=65536, help="samples per optimiser step")
    p.add_argument("--fcnet-hiddens", type=int, nargs=2, default=(256, 256), metavar=("H1", "H2"))
    p.add_argument("--fcnet-activation", choices=("tanh", "relu", "elu", "linear"), default="tanh")
    p.add_argument("--vf-share-layers", action="store_true")
    p.add_argument("--init-policy", default=None, metavar="FILE", help="start from this policy file instead of a fresh network")
    p.add_argument("--save", default=None, metavar="FILE", help="write the cloned policy to this file (mlp.save_policy: evaluate --policy and ppo --init-policy read it)")
    p.add_argument("--demos-out", default=None, metavar="FILE.npz", help="save the last iteration's demonstrations (all markets)")
    p.add_argument("--demos", default=None, metavar="FILE.npz", help="clone these recorded demonstrations instead of rolling out (no env is created)")
    p.add_argument("--out", default=None, help="write a JSON summary to this file")
    p.add_argument("--dagger", action="store_true", help="DAgger: label the learner's own states with --label-expert through the env's label tap (needs --label-expert; "
                                                         "goes without --expert, --teacher and --demos)")
    p.add_argument("--label-expert", default=None, metavar="SPEC", help="--dagger: the scripted law whose answers in the learner's slots are the labels")
    p.add_argument("--opponent", action="append", default=None, metavar="SPEC", help="--dagger: a scripted opponent behind the learner's slots; repeat for several (default: random modules)")
    p.add_argument("--beta", type=float, default=1.0, metavar="B", help="--dagger: the probability with which the learner's slot plays the label in iteration 0")
    p.add_argument("--beta-decay", type=float, default=0.5, metavar="D", help="--dagger: iteration i mixes with beta * D ** i")
    p.add_argument("--aggregate", type=int, default=None, metavar="K", help="--dagger: the iterations the aggregated data set holds (default: all of them)")
    args = p.parse_args(argv)
    if args.dagger:
        if args.label_expert is None:
            raise SystemExit("--dagger needs --label-expert")
        if args.expert is not None or args.teacher is not None or args.demos is not None or args.demos_out is not None:
            raise SystemExit("--dagger makes its own demonstrations: it goes without --expert, --teacher, --demos and --demos-out")
    elif args.label_expert is not None or args.opponent is not None:
        raise SystemExit("--label-expert and --opponent belong to --dagger")
    elif args.demos is None and args.expert is None and args.teacher is None:
        raise SystemExit("one of --expert, --teacher or --demos is needed")
    if args.demos is not None and (args.expert is not None or args.teacher is not None or args.demos_out is not None):
        raise SystemExit("--demos replaces the rollouts: it goes without --expert, --teacher and --demos-out")
    if parse_only:
        return args
    from .mlp import FusedPolicy, load_policy, save_policy
    dev = torch.device("cuda:0")
    policy = load_policy(args.init_policy, dev) if args.init_policy else None
    net = dict(hidden=tuple(args.fcnet_hiddens), activation=args.fcnet_activation, vf_share_layers=args.vf_share_layers)
    if args.demos is not None:
        demos = Demonstrations.load(args.demos, dev)
        if policy is None:
            policy = FusedPolicy(dev, seed=args.seed, n_hist=demos.obs.shape[1] // 42, **net)
        hist = fit(policy, demos, iters=args.iters, epochs=args.epochs, lr=args.lr, holdout=args.holdout, seed=args.seed, minibatch=args.minibatch)
        checks = {}
    else:
        from .vec_env import CDAVecEnv
        env = CDAVecEnv({"num_of_agents": args.agents, "init_cash": 1000000, "max_step": args.max_step, "is_render": False, "auto_reset": True, "n_hist": args.n_hist},
                        n_markets=args.markets, device="cuda:0", with_info=False)
        keep = {}
        if args.dagger:
            policy, hist = dagger(env, args.label_expert, opponents=args.opponent, learner_slots=args.learner_slots, iters=args.iters, horizon=args.horizon, beta=args.beta,
                                  beta_decay=args.beta_decay, aggregate=args.aggregate, epochs=args.epochs, lr=args.lr, seed=args.seed, policy=policy, holdout=args.holdout,
                                  minibatch=args.minibatch, **net)
        else:
            policy, hist = pretrain(env, experts=args.expert, learner_slots=args.learner_slots, iters=args.iters, horizon=args.horizon, epochs=args.epochs, lr=args.lr,
                                    seed=args.seed, policy=policy, holdout=args.holdout, teacher=args.teacher, minibatch=args.minibatch, keep=keep, **net)
        if args.demos_out:
            Demonstrations.from_rollout(keep["rollout"], keep["slot_src"]).save(args.demos_out)
        checks = {"flagged_markets": int((env.flags() != 0).sum().item()), "invariant_violations": int((env.check_invariants() != 0).sum().item())}
        env.close()
    summary = {"experts": args.expert, "teacher": args.teacher, "demos": args.demos, "iterations": hist, **checks}
    if args.dagger:
        summary.update(dagger=True, label_expert=args.label_expert, opponents=args.opponent)
    if args.save:
        save_policy(args.save, policy)
        summary["saved"] = args.save
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    return summary


if __name__ == "__main__":
    main()
