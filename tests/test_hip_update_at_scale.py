"""GPU: the fused PPO update at the shapes train_fused / train_league_fused run, against plain references (tests/update_check_util.py).

At the toy sizes of tests/test_hip_mlp.py and tests/test_hip_league.py the reduction of the weight gradient's partial sums (k_grad_reduce) runs its 8-chunk dense
loop at most once and its 64-tile bias loop at most once per thread, and k_mlp_wgrad splits a few tiles over its chunks.  At a training minibatch of 65 536 rows
the update runs 51 chunks (36 at history depths 6 .. 8: FusedUpdate's min(255 // jobs, rows / 512)) and 1024 row tiles; a league update of 262 144 single-sample
rows runs 4096 tiles.  Every case asserts first that its shape takes those paths, so that it cannot shrink below them unnoticed.

Stages (update_check_util): (a) the loss gradient on the kernel's own outputs against float64 autograd; (b) the weight gradient alone - float64 products of the
kernel's own bfloat16 images against upd.grad, 1e-4 of each block's largest entry as at the toy size; (c) the whole gradient against float32 autograd through
ppo.ActorCritic; (d) loss statistics, squared norm and one clipped Adam step.  Each case prints the error ratios it measured (pytest -s)."""
import pytest
import torch

from update_check_util import make_problem, make_update, stage_loss_gradient, stage_rest, stage_weight_gradient, stage_whole_gradient, step

pytestmark = pytest.mark.gpu


def _assert_training_paths(upd, chunks, tiles, s, R):
    assert chunks > 8 and chunks % 8 != 0, chunks                  # the dense 8-chunk loop runs more than once, then a remainder
    assert tiles > 64, tiles                                        # the bias loop runs more than once per thread
    if R > upd.rows_mb:
        assert s > 0 and s % upd.rows_mb == 0                       # a later minibatch: the gather reads perm at an offset


def _report(name, **kw):
    print(f"\n[update at scale] {name}: " + ", ".join(f"{k} {v}" for k, v in kw.items()), flush=True)


def _fmt(d):
    return {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in d.items()}


@pytest.mark.parametrize("case", ["ppo_4096x4", "rllib_2048x8"])
def test_fused_update_at_the_training_shape(case):
    """train_fused at 4096 markets x 64 steps x 4 agents (262 144 rows, minibatches of 65 536, the LAST one checked) and at 2048 x 64 x 8 with RLlib's objective
    (KL penalty against an older network's distribution rows, value clamp): advantage sums handed over, normalised inside the loss"""
    if case == "ppo_4096x4":
        A, R, rows_mb, s, kl_coef, vf_clip = 4, 262144, 65536, 196608, 0.0, 0.0
    else:
        A, R, rows_mb, s, kl_coef, vf_clip = 8, 131072, 32768, 65536, 0.2, 10.0
    prob = make_problem(A, None, kl_coef, R=R, seed=21, adv_stats=True)
    upd = make_update(prob, rows_mb, vf_clip=vf_clip)
    chunks, tiles = step(prob, upd, s, rows_mb)
    _assert_training_paths(upd, chunks, tiles, s, R)
    a_ratio, off, n, terms = stage_loss_gradient(prob, upd, s, rows_mb, vf_clip)
    b_ratio, _ = stage_weight_gradient(prob, upd, s, rows_mb)
    cos, c_worst = stage_whole_gradient(prob, upd, s, rows_mb, vf_clip)
    d_ratios = stage_rest(prob, upd, chunks, tiles, terms)
    _report(case, chunks=chunks, tiles=tiles, d_out=f"{a_ratio:.3g} ({off} of {n} samples off)", wgrad=_fmt(b_ratio), cos=f"{cos:.6f}",
            whole_block=f"{c_worst:.3g}", rest=_fmt(d_ratios))


def test_league_update_at_the_training_shape():
    """train_league_fused from 4096 x 8 up: one sample per row (the record stride selects slot 5 of 8), 262 144 rows in ONE minibatch - 4096 tiles, 51 chunks"""
    R = 262144
    prob = make_problem(8, 5, 0.0, R=R, seed=33, adv_stats=True)
    upd = make_update(prob, R)
    chunks, tiles = step(prob, upd, 0, R)
    _assert_training_paths(upd, chunks, tiles, 0, R)
    assert tiles == 4096 and chunks == 51
    a_ratio, off, n, terms = stage_loss_gradient(prob, upd, 0, R, 0.0)
    b_ratio, _ = stage_weight_gradient(prob, upd, 0, R)
    d_ratios = stage_rest(prob, upd, chunks, tiles, terms)
    _report("league_262144x1", chunks=chunks, tiles=tiles, d_out=f"{a_ratio:.3g} ({off} of {n} samples off)", wgrad=_fmt(b_ratio), rest=_fmt(d_ratios))


@pytest.mark.parametrize("n_hist,want_chunks", [(1, 51), (7, 36), (8, 36)])
def test_other_history_depths_at_the_training_rows(n_hist, want_chunks):
    """history depths 1 and 7 (42 H inputs: k_grad_reduce's entry-by-entry path through W1's padding) and 8 (7 weight-gradient jobs: 36 chunks) at 65 536 rows"""
    R = 65536
    prob = make_problem(4, None, 0.0, R=R, seed=40 + n_hist, n_hist=n_hist, adv_stats=True)
    upd = make_update(prob, R)
    chunks, tiles = step(prob, upd, 0, R)
    _assert_training_paths(upd, chunks, tiles, 0, R)
    assert chunks == want_chunks, chunks
    a_ratio, off, n, _ = stage_loss_gradient(prob, upd, 0, R, 0.0)
    b_ratio, _ = stage_weight_gradient(prob, upd, 0, R)
    _report(f"n_hist {n_hist}", chunks=chunks, tiles=tiles, d_out=f"{a_ratio:.3g} ({off} of {n} samples off)", wgrad=_fmt(b_ratio))


def test_ragged_tail_after_a_full_minibatch():
    """A = 3: train_fused's minibatch is 87 360 rows (262 144 / 3, down to a multiple of 32), three of them leave a 64-row tail - 2 chunks, 1 tile.  After a full
    step has filled the slabs with its partial sums, the tail's gradient is its own: nothing of the larger step leaks into it."""
    R, A = 262144, 3
    rows_mb = max(32, min(R, (max(1, 262144 // A) // 32) * 32))
    assert rows_mb == 87360 and R - 3 * rows_mb == 64
    prob = make_problem(A, None, 0.0, R=R, seed=55, adv_stats=True)
    upd = make_update(prob, rows_mb)
    chunks, tiles = step(prob, upd, 0, rows_mb)
    _assert_training_paths(upd, chunks, tiles, 0, rows_mb)
    big = upd.grad.cpu().double()
    s = 3 * rows_mb
    chunks, tiles = step(prob, upd, s, R - s)
    assert (chunks, tiles) == (2, 1)
    a_ratio, off, n, terms = stage_loss_gradient(prob, upd, s, 64, 0.0)
    b_ratio, _ = stage_weight_gradient(prob, upd, s, 64)
    d_ratios = stage_rest(prob, upd, chunks, tiles, terms, check_adam=False)
    assert not torch.equal(upd.grad.cpu().double(), big)
    _report("ragged tail", d_out=f"{a_ratio:.3g} ({off} of {n} samples off)", wgrad=_fmt(b_ratio), rest=_fmt(d_ratios))


def test_separate_kernels_equal_the_fused_step_at_the_training_shape():
    """FusedUpdate(fused=False) - prep_rows, k_mlp_fwd8, the records' loss kernel, k_mlp_bwd8 - on the same 65 536-row minibatch of 262 144: observation image,
    activations and outputs bit for bit, gradients within the bounds of test_hip_mlp's test_fused_forward_loss_backward_equals_the_separate_kernels"""
    R, A, rows, s = 262144, 4, 65536, 131072
    res = []
    for fused in (True, False):
        prob = make_problem(A, None, 0.0, R=R, seed=61, adv_stats=True)
        upd = make_update(prob, rows, fused=fused)
        chunks, tiles = step(prob, upd, s, rows)
        _assert_training_paths(upd, chunks, tiles, s, R)
        xpk = (upd.x_pk_mb if fused else upd.x_pk[s * 192:])[:rows * 192].clone()
        res.append(dict(out=upd.out[:rows].clone(), d_out=upd.d_out[:rows].clone(), grad=upd.grad.clone(), out6=upd.out6.clone(), xpk=xpk,
                        h1=upd.h1p[:rows * 512].clone(), h2=upd.h2p[:rows * 512].clone(), dz2=upd.dz2p[:rows * 512].float().clone(), dz1=upd.dz1p[:rows * 512].float().clone()))
        if not fused:
            b_ratio, _ = stage_weight_gradient(prob, upd, s, rows)
        del upd
    a, b = res
    assert torch.equal(a["xpk"].view(torch.int16), b["xpk"].view(torch.int16))
    assert torch.equal(a["h1"].view(torch.int16), b["h1"].view(torch.int16)) and torch.equal(a["h2"].view(torch.int16), b["h2"].view(torch.int16))
    assert torch.equal(a["out"][:, :25], b["out"][:, :25])
    assert torch.allclose(a["d_out"], b["d_out"], rtol=2e-4, atol=2e-5 * float(a["d_out"].abs().max()))
    for k in ("dz2", "dz1"):
        assert (a[k] - b[k]).abs().max() <= 2e-2 * a[k].abs().max()
    assert torch.allclose(a["out6"], b["out6"], rtol=1e-4, atol=1e-7)
    g_err = float((a["grad"] - b["grad"]).abs().max() / a["grad"].abs().max())
    assert g_err <= 1e-3
    d_err = float((a["d_out"] - b["d_out"]).abs().max() / a["d_out"].abs().max())
    _report("separate kernels", grad=f"{g_err:.3g}", d_out=f"{d_err:.3g}", wgrad_separate=_fmt(b_ratio))
