"""Test helper: the fused PPO update (mlp.FusedUpdate, csrc/cda_mlp.hip k_mlp_fb + k_mlp_wgrad + k_grad_reduce + k_adam) against plain references, stage by stage.

(a) the loss gradient the kernel feeds its backward pass, against float64 autograd of the loss on the kernel's OWN float32 outputs (the clip / clamp decisions are
    taken on the same numbers); (b) the weight gradient alone: float64 products of the kernel's own bfloat16 activations and pre-activation gradients against
    upd.grad, block by block - isolates the weight-gradient products and the reduction of their partial sums; (c) the whole gradient against float32 autograd
    through ppo.ActorCritic; (d) the rest of the step: loss statistics, the squared gradient norm, one clipped Adam step against torch.

check_gradient() runs them on one minibatch [s, s + rows) of a whole batch of R rows; tests/test_hip_league.py, tests/test_hip_update_at_scale.py and
tools/gradient_soak.py drive it."""
import math

import torch

DEV = "cuda:0"


def _obs(n, seed=5, obs_dim=168):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, obs_dim, generator=g) * 1.5
    x[:, ::7] = 0.0
    return x


def _torch_objective(m, x, acts, lp_old, adv, ret, dist_old, ls_old, clip, vf_coef, ent_coef, kl_coef, vf_clip, agents_per_row):
    """the loss the fused kernel differentiates, stated with torch ops (RLlib's PPO torch learner: surrogate, clamped value error, entropy, KL(old || new))"""
    logp, ent, v = m.evaluate(x, acts, agents_per_row=agents_per_row)
    ratio = (logp - lp_old).exp()
    pg = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
    sq = (v - ret).pow(2)
    vl = (sq.clamp(max=vf_clip) if vf_clip > 0 else sq).mean()
    o, _ = m.trunk(x)
    o = o.float()
    kl = torch.zeros(x.shape[0])
    for lo, hi in ((0, 9), (9, 19), (19, 22)):
        ls_new = torch.log_softmax(o[:, lo:hi], -1)
        kl = kl + (dist_old[:, lo:hi].exp() * (dist_old[:, lo:hi] - ls_new)).sum(-1)
    mu_o, mu_n = dist_old[:, 22:24], o[:, 22:24]
    ls_new, ls_old = m.trunk_ls(x)[2], dist_old[:, 24:26]               # per row: the free vector (+ the state-dependent head's offsets); the rollout's ride in the row
    kl = kl + ((ls_new - ls_old) + (torch.exp(2 * ls_old) + (mu_o - mu_n) ** 2) / (2 * torch.exp(2 * ls_new)) - 0.5).sum(-1)
    return pg + vf_coef * vl - ent_coef * ent.mean() + kl_coef * kl.mean(), pg, vl, kl.mean()


def _grad_vector(m):
    from gym_continuousdoubleauction_amd import mlp
    gm = torch.zeros(mlp.PARAMS, dtype=torch.float64)
    H = 256
    gm[mlp.OFF_W1:mlp.OFF_B1] = m.l1.weight.grad.double().reshape(-1); gm[mlp.OFF_B1:mlp.OFF_W2] = m.l1.bias.grad.double()
    w2g = m.l2.weight.grad.double()
    gm[mlp.OFF_W2:mlp.OFF_B2] = torch.stack([w2g[:H, :H], w2g[H:, H:]]).reshape(-1); gm[mlp.OFF_B2:mlp.OFF_WO] = m.l2.bias.grad.double()
    wog = m.out.weight.grad.double(); blk = torch.zeros(32, H, dtype=torch.float64); blk[:24] = wog[:24, :H]; blk[24] = wog[24, H:]
    sd = m.state_dependent_log_std
    if sd:
        blk[25:27] = wog[25:27, :H]
    gm[mlp.OFF_WO:mlp.OFF_BO] = blk.reshape(-1)
    bog = m.out.bias.grad.double().clone(); bog[27 if sd else 25:] = 0
    gm[mlp.OFF_BO:mlp.OFF_LS] = bog; gm[mlp.OFF_LS:] = 0.0 if m.log_std.grad is None else m.log_std.grad.double()
    return gm


BLOCKS = lambda mlp: ((mlp.OFF_W1, mlp.OFF_B1, "W1"), (mlp.OFF_B1, mlp.OFF_W2, "b1"), (mlp.OFF_W2, mlp.OFF_B2, "W2"), (mlp.OFF_B2, mlp.OFF_WO, "b2"),   # noqa: E731
                      (mlp.OFF_WO, mlp.OFF_BO, "Wo"), (mlp.OFF_BO, mlp.OFF_LS, "bo"), (mlp.OFF_LS, mlp.PARAMS, "log_std"))


def _loss_gradient_on_outputs(out, log_std, sel, dist_old, ls_old, clip, vf_coef, ent_coef, kl_coef, vf_clip, sd=False, terms=False):
    """d loss / d outputs and d loss / d log_std by float64 autograd, starting from the kernel's OWN float32 outputs [R, 32] (so the clip / clamp decisions are taken
    on the same numbers): sel [R, agents, 8] the rows' sample records, dist_old [R, 24] - all in minibatch order.  terms: also the float64 per-sample loss terms
    {pg, vl, ent: [R * agents], kl: [R]} whose means the kernel reports in out6."""
    R, agents = sel.shape[0], sel.shape[1]
    o = out.double().clone().requires_grad_()
    ls_free = log_std.double().clone().requires_grad_()
    ls_row = ls_free + o[:, 25:27]                                  # [R, 2]: the free vector + the head's offsets (the kernel adds them whether or not the head trains)
    if not sd:
        ls_row = ls_free + o[:, 25:27].detach()
    O = o.repeat_interleave(agents, 0)
    ls = ls_row.repeat_interleave(agents, 0)
    flat = sel.reshape(R * agents, 8)
    acts = [flat[:, c].contiguous().view(torch.int32).long() for c in range(3)]
    a_cont, lp_old, adv, ret = flat[:, 3:5].double(), flat[:, 5].double(), flat[:, 6].double(), flat[:, 7].double()
    logp = ent = 0.0
    for (lo, hi), a in zip(((0, 9), (9, 19), (19, 22)), acts):
        l = torch.log_softmax(O[:, lo:hi], -1)
        logp = logp + l.gather(1, a.view(-1, 1)).squeeze(1)
        ent = ent - (l.exp() * l).sum(-1)
    z = (a_cont - O[:, 22:24]) * torch.exp(-ls)
    logp = logp + (-0.5 * z * z - ls - 0.5 * math.log(2 * math.pi)).sum(-1)
    ent = ent + (0.5 + 0.5 * math.log(2 * math.pi) + ls).sum(-1)
    ratio = (logp - lp_old).exp()
    pg_i = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv)
    pg = pg_i.mean()
    sq = (O[:, 24] - ret).pow(2)
    vl_i = sq.clamp(max=vf_clip) if vf_clip > 0 else sq
    vl = vl_i.mean()
    loss = pg + vf_coef * vl - ent_coef * ent.mean()
    kl = torch.zeros(R, dtype=torch.float64)
    if kl_coef:
        d = dist_old.double()
        lo_ = d[:, 24:26]                                           # the log-stds every row was sampled with
        kl = 0.0
        for lo, hi in ((0, 9), (9, 19), (19, 22)):
            kl = kl + (d[:, lo:hi].exp() * (d[:, lo:hi] - torch.log_softmax(o[:, lo:hi], -1))).sum(-1)
        kl = kl + ((ls_row - lo_) + (torch.exp(2 * lo_) + (d[:, 22:24] - o[:, 22:24]) ** 2) / (2 * torch.exp(2 * ls_row)) - 0.5).sum(-1)
        loss = loss + kl_coef * kl.mean()
    loss.backward()
    grads = o.grad, (torch.zeros(2, dtype=torch.float64) if sd else ls_free.grad)
    if terms:
        return grads + ({"pg": pg_i.detach(), "vl": vl_i.detach(), "ent": ent.detach(), "kl": kl.detach()},)
    return grads


def unpack_rows(packed, n_rows, n_feat, paired=False, first_row=0):
    """mlp.unpack_rows without its Python loops (rows [first_row, first_row + n_rows) of a packed bf16 image, first_row a multiple of 32): the same
    [n_rows/32][n_feat/32][2][64][8] -> [n_rows, n_feat] map as one scatter, for images of hundreds of thousands of rows"""
    per = 32 * n_feat
    p = packed.detach()[first_row * n_feat:first_row * n_feat + n_rows * n_feat].cpu().float().view(n_rows // 32, n_feat // 32, 2, 64, 8)
    assert first_row % 32 == 0 and p.numel() == (n_rows // 32) * per
    lane = torch.arange(64)
    j, h = lane & 31, lane >> 5
    r = 8 * torch.arange(2).view(2, 1, 1) + torch.arange(8).view(1, 1, 8)              # [2, 1, 8]
    row = ((r & 3) + 8 * (r >> 2) + 4 * h.view(1, 64, 1)).expand(2, 64, 8)           # [2, 64, 8]
    ft = torch.arange(n_feat // 32).view(-1, 1)
    col = (64 * (ft // 2) + 2 * j.view(1, 64) + (ft & 1)) if paired else ft * 32 + j.view(1, 64)          # [FT, 64]
    out = torch.zeros(n_rows // 32, 32, n_feat)
    out[:, row.unsqueeze(0).expand(n_feat // 32, 2, 64, 8), col.view(-1, 1, 64, 1).expand(n_feat // 32, 2, 64, 8)] = p
    return out.view(n_rows, n_feat)


def make_problem(A, slot, kl_coef, R=512, seed=6, sd=False, n_hist=4, adv_stats=False):
    """a policy, an older policy's distribution rows, R observation rows and their [R, A, 8] sample records.  adv_stats: also the two advantage sums and their
    count (what RolloutChains.gae hands the update), so the loss normalises the advantages on the fly; `rec_ref` then holds the normalised advantages as the
    kernel computes them (float32), the rows the references read."""
    from gym_continuousdoubleauction_amd import mlp
    g = torch.Generator().manual_seed(seed)
    L = mlp.layout(n_hist)
    th = mlp.init_theta(L.OBS, generator=torch.Generator().manual_seed(13), state_dependent_log_std=sd)
    p = mlp.FusedPolicy(DEV, theta=th)
    assert p.state_dependent_log_std == sd
    th_old = th.clone(); th_old[:L.OFF_LS] += 0.02 * torch.randn(L.OFF_LS, generator=g); th_old[L.OFF_LS:] = torch.tensor([-0.4, -0.65])
    x = _obs(R, seed=17, obs_dim=L.OBS) * 0.5
    rec = torch.zeros(R, A, 8)
    rec[..., 0] = torch.randint(0, 9, (R, A), generator=g).int().view(torch.float32)
    rec[..., 1] = torch.randint(0, 10, (R, A), generator=g).int().view(torch.float32)
    rec[..., 2] = torch.randint(0, 3, (R, A), generator=g).int().view(torch.float32)
    rec[..., 3:5] = torch.randn(R, A, 2, generator=g)
    rec[..., 5] = torch.randn(R, A, generator=g) * 0.1 - 7.0
    rec[..., 6] = torch.randn(R, A, generator=g)
    rec[..., 7] = torch.randn(R, A, generator=g)
    ls_old = th_old[L.OFF_LS:].clone()
    if kl_coef or R <= 4096:
        old_out = mlp.reference_outputs(th_old, x, emulate_bf16=False, dtype=torch.float32)
        dist_old = torch.cat([torch.log_softmax(old_out[:, :9], -1), torch.log_softmax(old_out[:, 9:19], -1), torch.log_softmax(old_out[:, 19:22], -1), old_out[:, 22:24],
                              ls_old + old_out[:, 25:27], torch.zeros(R, 2)], dim=1).contiguous()       # a rollout's row: ... | the log-stds it was sampled with | 2 zeros
        del old_out
    else:                                                        # (read only with the KL penalty)
        dist_old = torch.zeros(R, mlp.DIST_LD)
    prob = dict(p=p, L=L, x=x, rec=rec, rec_ref=rec, dist_old=dist_old, ls_old=ls_old, A=A, slot=slot, kl_coef=kl_coef, sd=sd, R=R, stats=None, count=0,
                agents=1 if slot is not None else A, g=g)
    if adv_stats:
        a = (rec[:, slot] if slot is not None else rec)[..., 6].double()
        stats = torch.tensor([float(a.sum()), float((a * a).sum())], dtype=torch.float64)
        n = a.numel()
        m = float(stats[0]) / n
        var = (float(stats[1]) - n * m * m) / (n - 1)
        mean32, rstd32 = torch.tensor(m, dtype=torch.float32), 1.0 / (torch.tensor(math.sqrt(var), dtype=torch.float32) + 1e-8)      # the kernel's float32 arithmetic
        ref = rec.clone()
        ref[..., 6] = (rec[..., 6] - mean32) * rstd32
        prob.update(stats=stats, count=n, rec_ref=ref)
    return prob


def make_update(prob, rows_mb, chunks=None, fused=True, vf_clip=0.0):
    """FusedUpdate over the problem's R rows with minibatches of rows_mb (chunks None: the default FusedUpdate picks), a random permutation and the problem's
    extra terms; device copies of the rows and records ride on the returned update (upd.dev)"""
    from gym_continuousdoubleauction_amd import mlp
    from gym_continuousdoubleauction_amd._lib import lib, check
    R, A, slot = prob["R"], prob["A"], prob["slot"]
    upd = mlp.FusedUpdate(prob["p"], R, rows_mb, prob["agents"], chunks=chunks, fused=fused)
    upd.perm.copy_(torch.randperm(R, generator=prob["g"]))
    recd, xd, dd, lsd = prob["rec"].to(DEV), prob["x"].to(DEV), prob["dist_old"].to(DEV), prob["ls_old"].to(DEV)
    statsd = prob["stats"].to(DEV) if prob["stats"] is not None else None
    if fused or slot is not None or prob["kl_coef"] or vf_clip:
        upd.set_extra(rec_stride=8 * A if slot is not None else 0, kl_coef=prob["kl_coef"], vf_clip=vf_clip, dist_old=dd, log_std_old=lsd)
    if not fused:
        check(lib().cda_mlp_prep_rows(xd.data_ptr(), upd.perm.data_ptr(), R, upd.x_rm.data_ptr(), upd.x_pk.data_ptr(), torch.cuda.current_stream().cuda_stream), "prep")
    upd.dev = dict(rec=recd, x=xd, dist=dd, ls=lsd, stats=statsd)
    return upd


def step(prob, upd, s, rows, clip=0.3, vf_coef=1.0, ent_coef=0.01):
    """one minibatch step with lr = 0 (the gradient and the loss statistics, parameters untouched); returns (chunks, tiles) the step ran with"""
    slot, d = prob["slot"], upd.dev
    base = d["rec"].data_ptr() + (32 * slot if slot is not None else 0)
    theta0 = prob["p"].theta.clone()
    ct = upd.minibatch_step(s, rows, None, None, None, None, clip, vf_coef, ent_coef, 0.0, (0.9, 0.999), 1e-8, math.inf, records=(base, d["stats"], prob["count"]),
                            obs_rows=d["x"] if upd.fused else None, debug_outputs=True)
    torch.cuda.synchronize()
    assert torch.equal(prob["p"].theta, theta0)                  # lr = 0
    return ct


def _sel(prob):
    rec = prob["rec_ref"]
    return rec[:, prob["slot"]:prob["slot"] + 1] if prob["slot"] is not None else rec


def stage_loss_gradient(prob, upd, s, rows, vf_clip, clip=0.3, vf_coef=1.0, ent_coef=0.01):
    """(a): d_out against float64 autograd on the kernel's own outputs; returns (worst row error / scale, off rows, samples, the float64 loss terms)"""
    p, sd = prob["p"], prob["sd"]
    pm = upd.perm.cpu()[s:s + rows]
    g_out, g_ls, terms = _loss_gradient_on_outputs(upd.out[:rows].cpu(), p.theta[p.L.OFF_LS:].cpu(), _sel(prob)[pm], prob["dist_old"][pm], prob["ls_old"], clip, vf_coef, ent_coef,
                                                   prob["kl_coef"], vf_clip, sd=sd, terms=True)
    d_out = upd.d_out[:rows].cpu().double()
    scale = float(g_out.abs().max())
    NC = 27 if sd else 25
    row_err = (d_out[:, :NC] - g_out[:, :NC]).abs().max(1).values
    off = int((row_err > 1e-4 * scale).sum())
    n = rows * prob["agents"]
    assert off <= n // 20000, ("d loss / d outputs", off, float(row_err.max()), scale)
    assert float(d_out[:, NC:].abs().max()) == 0.0
    grad_ls = upd.grad.cpu().double()[p.L.OFF_LS:]
    assert float((grad_ls - g_ls).abs().max()) <= 1e-4 * float(g_ls.abs().max()) + 1e-9, ("d loss / d log_std", grad_ls, g_ls)
    return float(row_err.sort().values[:rows - off].max()) / scale, off, n, terms


def stage_weight_gradient(prob, upd, s, rows, block=32768, bound=1e-4):
    """(b): the weight gradient alone.  The kernel's own bfloat16 images of the minibatch (x_pk_mb or the separate path's x_pk, h1p, h2p, dz1p, dz2p, doutp)
    multiplied and summed in float64, row block by row block, against upd.grad - block by block, each within `bound` of the block's largest entry.  Returns the
    worst ratio per block."""
    p, L = prob["p"], prob["p"].L
    XF = 32 * L.XT
    g = torch.zeros(L.PARAMS, dtype=torch.float64)
    W1, W2a, W2b, Wo = (g[L.OFF_W1:L.OFF_B1].view(512, L.OBS), g[L.OFF_W2:L.OFF_B2].view(2, 256, 256)[0], g[L.OFF_W2:L.OFF_B2].view(2, 256, 256)[1],
                        g[L.OFF_WO:L.OFF_BO].view(32, 256))
    b1, b2, bo = g[L.OFF_B1:L.OFF_W2], g[L.OFF_B2:L.OFF_WO], g[L.OFF_BO:L.OFF_LS]
    xsrc = upd.x_pk_mb if upd.fused else upd.x_pk[s * XF:]                 # (the separate kernels' image holds the whole shuffled batch)
    pol = [r for r in range(32) if r < 24 or r in (25, 26)]
    for r0 in range(0, rows, block):
        n = min(block, rows - r0)
        n32 = (n + 31) // 32 * 32
        xb = unpack_rows(xsrc, n32, XF, first_row=r0)[:n, :L.OBS].double()
        h1, h2, k1, k2 = (unpack_rows(t, n32, 512, paired=True, first_row=r0)[:n].double() for t in (upd.h1p, upd.h2p, upd.dz1p, upd.dz2p))
        do = unpack_rows(upd.doutp, n32, 32, first_row=r0)[:n].double()
        W1 += k1.t() @ xb; b1 += k1.sum(0)
        W2a += k2[:, :256].t() @ h1[:, :256]; W2b += k2[:, 256:].t() @ h1[:, 256:]; b2 += k2.sum(0)
        Wo[pol] += do[:, pol].t() @ h2[:, :256]; Wo[24] += do[:, 24] @ h2[:, 256:]
        bo[:27] += upd.d_out[r0:r0 + n, :27].cpu().double().sum(0)
        del xb, h1, h2, k1, k2, do
    grad = upd.grad.cpu().double()
    worst = {}
    for lo, hi, name in BLOCKS(L)[:-1]:
        err = float((grad[lo:hi] - g[lo:hi]).abs().max())
        mx = float(g[lo:hi].abs().max())
        assert mx > 0 and err <= bound * mx, ("weight gradient", name, err, mx)
        worst[name] = err / mx
    return worst, g


def stage_whole_gradient(prob, upd, s, rows, vf_clip, d_out=None, clip=0.3, vf_coef=1.0, ent_coef=0.01):
    """(c): the backward pass alone (the kernel's loss gradient through the float32 PyTorch network) within 3 % per block, and the whole gradient against float32
    autograd of the whole objective: cosine > 0.999, 3 % per block.  Returns (cosine, worst block ratio)."""
    from gym_continuousdoubleauction_amd import mlp
    p, sd, agents = prob["p"], prob["sd"], prob["agents"]
    pm = upd.perm.cpu()[s:s + rows]
    grad = upd.grad.cpu().double()
    sel = _sel(prob)[pm]
    xs = prob["x"][pm]
    m = mlp.actor_critic_from_theta(p.theta).float()
    acts = (sel[..., 0].contiguous().view(torch.int32).long().reshape(-1), sel[..., 1].contiguous().view(torch.int32).long().reshape(-1),
            sel[..., 2].contiguous().view(torch.int32).long().reshape(-1), sel[..., 3:5].reshape(-1, 2))
    loss, pg, vl, kl = _torch_objective(m, xs, acts, sel[..., 5].reshape(-1), sel[..., 6].reshape(-1), sel[..., 7].reshape(-1), prob["dist_old"][pm], prob["ls_old"],
                                        clip, vf_coef, ent_coef, prob["kl_coef"], vf_clip, agents)
    loss.backward()
    gm = _grad_vector(m)
    NC = 27 if sd else 25
    d_out = upd.d_out[:rows].cpu().double() if d_out is None else d_out
    m2 = mlp.actor_critic_from_theta(p.theta).float()
    o2 = m2.trunk_packed(xs)
    torch.autograd.backward([o2], [torch.cat([d_out[:, :NC], torch.zeros(rows, 32 - NC, dtype=torch.float64)], 1).float()])
    m2.log_std.grad = torch.zeros(2)
    g2 = _grad_vector(m2)
    worst = 0.0
    for lo, hi, name in BLOCKS(mlp)[:-1]:
        a, b = grad[lo:hi], g2[lo:hi]
        assert (a - b).norm() <= 3e-2 * b.norm() + 1e-9, ("backward pass alone", name, float((a - b).norm() / b.norm()))
    cos = float((grad * gm).sum() / (grad.norm() * gm.norm()))
    assert cos > 0.999, cos
    for lo, hi, name in BLOCKS(mlp):
        a, b = grad[lo:hi], gm[lo:hi]
        assert (a - b).norm() <= (4e-2 if sd else 3e-2) * b.norm() + 1e-9, (name, float((a - b).norm() / b.norm()))
        worst = max(worst, float((a - b).norm() / b.norm()))
    return cos, worst


def stage_rest(prob, upd, chunks, tiles, terms, vf_coef=1.0, ent_coef=0.01, check_adam=True):
    """(d): out6 against the float64 loss terms (each mean within 1e-5 of the mean absolute term: float32 per-sample arithmetic summed in float64), norm2[2]
    against the float64 sum of squares of upd.grad, and one clipped Adam step (max_norm 0.5, lr 5e-5) from the device gradient against clip_grad_norm_ +
    torch.optim.Adam.  Returns the worst ratios."""
    from gym_continuousdoubleauction_amd._lib import check
    p, kl_coef = prob["p"], prob["kl_coef"]
    out6 = upd.out6.cpu().double()
    ratios = {}
    ref = {0: terms["pg"], 1: terms["vl"], 2: terms["ent"], 6: terms["kl"]}
    for w, t in ref.items():
        if w == 6 and not kl_coef:
            assert float(out6[6]) == 0.0
            continue
        err, scale = abs(float(out6[w]) - float(t.mean())), float(t.abs().mean())
        assert err <= 1e-5 * scale + 1e-12, ("out6", w, float(out6[w]), float(t.mean()))
        ratios[f"out6[{w}]"] = err / scale
    total = terms["pg"].mean() + vf_coef * terms["vl"].mean() - ent_coef * terms["ent"].mean() + kl_coef * terms["kl"].mean()
    scale = float(terms["pg"].abs().mean() + vf_coef * terms["vl"].abs().mean() + ent_coef * terms["ent"].abs().mean() + kl_coef * terms["kl"].abs().mean())
    err = abs(float(out6[3]) - float(total))
    assert err <= 1e-5 * scale, ("out6 loss", float(out6[3]), float(total))
    ratios["out6[3]"] = err / scale
    grad = upd.grad.cpu().double()
    n2, want = float(upd.norm2[2].cpu()), float((grad * grad).sum())
    assert abs(n2 - want) <= 1e-6 * want, ("norm2", n2, want)
    ratios["norm2"] = abs(n2 - want) / want
    if check_adam:
        # the partial sums of the step are still in the slabs: the same reduce once more (without the loss sums: log_std's entries 0), now with lr and clipping
        p.adam_m.zero_(); p.adam_v.zero_(); p.adam_step.zero_()
        theta_before = p.theta.clone()
        st = torch.cuda.current_stream().cuda_stream
        check(p.L.fn("cda_mlp_adam")(p.theta.data_ptr(), p.adam_m.data_ptr(), p.adam_v.data_ptr(), p.adam_step.data_ptr(), p.wb.data_ptr(), upd.slab.data_ptr(), chunks,
                                     upd.bias_slab.data_ptr(), tiles, None, 0, 0.0, 0.0, 0.0, None, 5e-5, 0.9, 0.999, 1e-8, 0.5, upd.grad.data_ptr(), upd.norm2.data_ptr(), st),
              "cda_mlp_adam")
        torch.cuda.synchronize()
        g2 = upd.grad.cpu().double()
        assert torch.equal(g2[:p.L.OFF_LS], grad[:p.L.OFF_LS]) and (g2[p.L.OFF_LS:] == 0).all()      # the reduce is deterministic
        th = torch.nn.Parameter(theta_before)
        opt = torch.optim.Adam([th], lr=5e-5)
        th.grad = upd.grad.clone()
        torch.nn.utils.clip_grad_norm_([th], 0.5)
        opt.step()
        err = float((p.theta - th.detach()).abs().max())
        assert err <= 5e-8, ("adam", err)                       # float32 update of magnitude ~lr = 5e-5: agreement to 1e-3 of a step
        ratios["adam"] = err / 5e-5
    return ratios


def check_gradient(A, slot, kl_coef, vf_clip, R=512, seed=6, chunks=4, check_clip_share=True, soak=False, sd=False, rows=None, s=0, adv_stats=False):
    """(also driven over random shapes by tools/gradient_soak.py, soak=True: there the TIGHT check is the loss gradient on the kernel's own outputs; the whole
    gradient against float32 autograd is held to wider bands - a sample whose ratio / value error sits within bfloat16 noise of a clip / clamp boundary takes the
    other branch in float32, a discrete change of that sample's whole contribution, and random shapes with few samples per minibatch meet that)
    R: rows of the whole batch; the checked minibatch is [s, s + rows) of its permutation (rows None: all R).  chunks None: FusedUpdate's default.
    adv_stats: the loss normalises the advantages with sums handed over as train_fused does.  Returns the cosine and a dict of the measured error ratios."""
    from gym_continuousdoubleauction_amd import mlp
    rows = R if rows is None else rows
    prob = make_problem(A, slot, kl_coef, R=R, seed=seed, sd=sd, adv_stats=adv_stats)
    p, x, dist_old, ls_old, agents = prob["p"], prob["x"], prob["dist_old"], prob["ls_old"], prob["agents"]
    upd = make_update(prob, rows, chunks=chunks, vf_clip=vf_clip)
    step(prob, upd, s, rows)
    grad, out6 = upd.grad.cpu().double(), upd.out6.cpu()
    perm = upd.perm.cpu()
    m = mlp.actor_critic_from_theta(p.theta).float()
    pm = perm[s:s + rows]
    sel = _sel(prob)[pm]                                         # [rows, agents, 8]
    xs, ds = x[pm], dist_old[pm]
    acts = (sel[..., 0].contiguous().view(torch.int32).long().reshape(-1), sel[..., 1].contiguous().view(torch.int32).long().reshape(-1),
            sel[..., 2].contiguous().view(torch.int32).long().reshape(-1), sel[..., 3:5].reshape(-1, 2))
    loss, pg, vl, kl = _torch_objective(m, xs, acts, sel[..., 5].reshape(-1), sel[..., 6].reshape(-1), sel[..., 7].reshape(-1), ds, ls_old,
                                        0.3, 1.0, 0.01, kl_coef, vf_clip, agents)
    loss.backward()
    gm = _grad_vector(m)
    # (1) tight: the loss gradient the kernel fed its backward pass, against float64 autograd on the kernel's own outputs (same decisions at the clip / clamp
    #     boundaries): every shape-dependent piece - record stride, agents per row, the KL rows, the clamp - is in this step
    g_out, g_ls = _loss_gradient_on_outputs(upd.out[:rows].cpu(), p.theta[mlp.OFF_LS:].cpu(), sel, ds, ls_old, 0.3, 1.0, 0.01, kl_coef, vf_clip, sd=sd)
    d_out = upd.d_out[:rows].cpu().double()
    scale = float(g_out.abs().max())
    NC = 27 if sd else 25                                        # the columns that carry a gradient: 24 policy outputs, the value, (the head's two log-std offsets)
    row_err = (d_out[:, :NC] - g_out[:, :NC]).abs().max(1).values
    if sd:
        assert float(d_out[:, 25:27].abs().max()) > 1e-3 * scale and float(upd.out[:rows, 25:27].abs().max()) > 0.05
    off = int((row_err > 1e-4 * scale).sum())
    # (a sample EXACTLY on a clip / clamp boundary - within float32 rounding of it - may take the other branch in float64: at most one row per 20 000 samples)
    assert off <= (rows * agents) // 20000, ("d loss / d outputs", off, float(row_err.max()), scale)
    assert float(d_out[:, NC:].abs().max()) == 0.0
    assert float((grad[mlp.OFF_LS:] - g_ls).abs().max()) <= 1e-4 * float(g_ls.abs().max()) + 1e-9, ("d loss / d log_std", grad[mlp.OFF_LS:], g_ls)
    ratios = {"d_out": float(row_err.sort().values[:rows - off].max()) / scale, "d_out_off_rows": off,
              "log_std": float((grad[mlp.OFF_LS:] - g_ls).abs().max()) / max(float(g_ls.abs().max()), 1e-300)}
    # (2) the network's backward pass alone: the kernel's loss gradient pushed through the float32 PyTorch network by autograd - no decision is taken in this
    #     comparison, what is left is bfloat16 operands against float32
    m2 = mlp.actor_critic_from_theta(p.theta).float()
    o2 = m2.trunk_packed(xs)
    torch.autograd.backward([o2], [torch.cat([d_out[:, :NC], torch.zeros(rows, 32 - NC, dtype=torch.float64)], 1).float()])
    m2.log_std.grad = torch.zeros(2)
    g2 = _grad_vector(m2)
    for lo, hi, name in BLOCKS(mlp)[:-1]:
        a, b = grad[lo:hi], g2[lo:hi]
        assert (a - b).norm() <= 3e-2 * b.norm() + 1e-9, ("backward pass alone", name, float((a - b).norm() / b.norm()))
        ratios[f"backward {name}"] = float((a - b).norm() / b.norm())
    # (3) the whole gradient against float32 autograd through the PyTorch network
    cos = float((grad * gm).sum() / (grad.norm() * gm.norm()))
    assert cos > (0.9 if soak else 0.999), cos                   # bfloat16 operands against float32: direction within 1e-3, every block's magnitude within 3 %
    # (with the state-dependent head every row's log-stds are bfloat16-operand products too - they scale the Gaussian heads' whole gradient: 4 %, measured 3.1 % on W1)
    for lo, hi, name in BLOCKS(mlp):
        a, b = grad[lo:hi], gm[lo:hi]
        assert (a - b).norm() <= (0.5 if soak else (4e-2 if sd else 3e-2)) * b.norm() + 1e-9, (name, float((a - b).norm() / b.norm()))
        ratios[f"whole {name}"] = float((a - b).norm() / b.norm())
    assert abs(float(out6[3]) - float(loss.detach())) <= 2e-2 * abs(float(loss.detach())) + 1e-3
    assert abs(float(out6[1]) - float(vl.detach())) <= 2e-2 * float(vl.detach()) + 1e-4
    if kl_coef:
        assert float(kl.detach()) > 1e-4 and abs(float(out6[6]) - float(kl.detach())) <= 3e-2 * float(kl.detach()) + 1e-5, (float(out6[6]), float(kl.detach()))
    else:
        assert float(out6[6]) == 0.0
    if vf_clip and check_clip_share:                               # the clamp is active on a real share of the samples
        frac = float(((m.evaluate(xs, acts, agents_per_row=agents)[2] - sel[..., 7].reshape(-1)).pow(2) > vf_clip).float().mean())
        assert 0.2 < frac < 0.95, frac
    ratios["cos"] = cos
    del perm
    return cos, ratios
