"""GPU: EVERY compiled object of the network kernels (tests/mlp_variants.py: 7 history depths x 4 hidden activations x separate / shared trunk = 56, each with its own
k-steps of layer 1, W1 operand layout, LDS tiles, dW1 slab and activation epilogue) against the float64 statement of its network (mlp.reference_outputs /
reference_gradients) and the relations the suite holds at the default variant.  tests/test_hip_hist.py, test_hip_activation.py and test_hip_vf_share.py walk the
AXES of the table (every depth at tanh, every activation and the shared trunk at depths 1, 4, 8); this file walks the cross product - 31 of the 56 objects
(tests/test_mlp_variants_host.py prints them) had never been launched by a numeric test: depths 2, 3, 6, 7 - the only ones whose padded observation is a whole
number of 32-wide operand tiles, or (7) ends in a half tile like 1, 4, 8 - with anything but tanh on a separate trunk, and linear on a shared one.

Per variant: (a) forward and stored activations, (b) the pad columns of the observation images, (c) backward / weight gradients / reduce, (d) the one-launch update
against the separate kernels on a real rollout, (e) the sampling and the greedy launch, (f) the league launches, (g) the entry points with no relation of their
own above, and that every entry point of include/cda_mlp.h was launched for this variant.  Every bound is the one the suite applies to the same quantity at depths
1, 4, 8 (quoted at each assert); the state-dependent log-std head is on for every other variant (mlp_variants.head_on).  The conditions the dispatch checks rest
on - a non-tanh network's outputs differ from the tanh network's, a shared trunk's value column from the separate network's, a relu network stores zeros - are
confirmed on the float64 statement alone in tests/test_mlp_variants_host.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mlp_variants as V      # noqa: E402
import sampler_ref as R       # noqa: E402

pytestmark = pytest.mark.gpu

DEV = V.DEV
H = V.H
CALLED = {}          # variant -> the entry points of include/cda_mlp.h launched for it (through Layout.fn)
RAN = {}             # variant -> the checks of this file that ran for it
CHECKS = ("a", "b", "c", "d", "e", "f")


@pytest.fixture(scope="module", autouse=True)
def _record_entry_points():
    """every entry point handed out by Layout.fn is wrapped for the time of this module: a call notes (variant, name) - check (g) reads the notes"""
    from gym_continuousdoubleauction_amd import _lib, mlp
    orig = mlp.Layout.fn

    def fn(self, name):
        f = orig(self, name)
        if name not in _lib.MLP_SYMBOLS:
            return f
        key = (self.hist, self.activation, self.vf_share_layers)

        def call(*args):
            CALLED.setdefault(key, set()).add(name)
            return f(*args)
        return call
    mlp.Layout.fn = fn
    yield
    mlp.Layout.fn = orig


def _policy(h, act, vfs, sd=None, **kw):
    p = V.policy(h, act, vfs, kw.pop("seed", V.seed_of(h)), kw.pop("scale", 2.0), V.head_on(h, act, vfs) if sd is None else sd, **kw)
    assert p.L.suffix == V.object_name(h, act, vfs)[len("cda_mlp"):] and (p.L.hist, p.activation, p.vf_share_layers) == (h, act, vfs)
    return p


def _half(t, vfs):
    """what a shared trunk's images are compared on: the trunk's (policy half's) columns"""
    return t[:, :H] if vfs else t


# ---- a ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,act,vfs", V.PARAMS)
def test_a_forward_and_stored_activations_equal_the_rounded_reference(h, act, vfs):
    """p.forward on 200 rows (no multiple of the 128-row tile) and prep_rows + forward_train on their first 160 against the float64 statement; bounds:
    tests/test_hip_activation.py (separate trunk: 3e-3 max(1, max |ref|) hmax) and tests/test_hip_vf_share.py (shared: 2e-2 max(1, max |h2|)); the stored images
    within one bfloat16 ulp (h1) / two (h2: it inherits h1's flips) of max(1, max |h|), at most 2 % / 5 % of the entries flipped"""
    from gym_continuousdoubleauction_amd import mlp
    RAN.setdefault((h, act, vfs), set()).add("a")
    sd = V.head_on(h, act, vfs)
    live = 27 if sd else 25
    p = _policy(h, act, vfs)
    n = V.N_TRAIN
    x = V.obs(V.N_FWD, h)
    ref, xb, h1, h2 = mlp.reference_outputs(p.theta, x, keep=True, activation=act, vf_share_layers=vfs)
    xd = x.to(DEV)
    out_dev = p.forward(xd).clone()
    out = out_dev.cpu().double()
    hmax = max(1.0, float(h1.abs().max()), float(h2.abs().max()))
    tol = 2e-2 * max(1.0, float(h2.abs().max())) if vfs else 3e-3 * max(1.0, float(ref.abs().max())) * hmax
    err = float((out[:, :27] - ref[:, :27]).abs().max())
    print(f"\n[mlp variants] {V.variant_id((h, act, vfs))} forward: error {err:.3g} (bound {tol:.3g}), max |h| {hmax:.3g}")
    assert err <= tol, (err, tol)
    assert bool((out[:, live:] == 0).all()) and (not sd or float(out[:, 25:27].abs().max()) > 0)          # columns 25 .. 31: exact zeros without the head
    ws = V.train_forward(p, x[:n])
    g1, g2 = V.images(ws, n)
    a1, a2, r1, r2 = _half(g1, vfs), _half(g2, vfs), _half(h1[:n], vfs), _half(h2[:n], vfs)
    e1, e2, f1, f2 = float((a1 - r1).abs().max()), float((a2 - r2).abs().max()), float((a1 != r1).double().mean()), float((a2 != r2).double().mean())
    print(f"[mlp variants] {V.variant_id((h, act, vfs))} images: h1 {e1:.3g} flipped {f1:.4f}, h2 {e2:.3g} flipped {f2:.4f}")
    assert e1 <= 2 ** -7 * max(1.0, float(r1.abs().max())) and f1 < 0.02
    assert e2 <= 2 ** -6 * max(1.0, float(r2.abs().max())) and f2 < 0.05
    assert torch.equal(ws["out"][:n], out_dev[:n])               # the training forward and the rollout's forward: the same outputs bit for bit
    if act == "relu":
        assert bool((a1 >= 0).all()) and float((a1 == 0).double().mean()) > 0.2
    if act != "tanh":                                            # dispatch: the activation is applied - the tanh object gives other outputs for the same parameters
        tanh = mlp.FusedPolicy(DEV, theta=p.theta.cpu(), vf_share_layers=vfs).forward(xd).cpu().double()
        assert float((tanh[:, :25] - out[:, :25]).abs().max()) > 1e-2
    if vfs:                                                      # dispatch: the value column is the trunk's, and the value half of theta is not read
        sep = mlp.reference_outputs(p.theta, x, activation=act)
        assert float((sep[:, 24] - out[:, 24]).abs().max()) > 1e-2
        V.perturb_value_half(p)
        ws2 = V.train_forward(p, x[:n])
        out2 = p.forward(xd)
        torch.cuda.synchronize()
        assert torch.equal(out_dev.view(torch.int32), out2.view(torch.int32)) and torch.equal(ws2["out"][:n].view(torch.int32), ws["out"][:n].view(torch.int32))
        assert torch.equal(V.trunk_tiles(ws["h1p"], n).view(torch.int16), V.trunk_tiles(ws2["h1p"], n).view(torch.int16))
        assert torch.equal(V.trunk_tiles(ws["h2p"], n).view(torch.int16), V.trunk_tiles(ws2["h2p"], n).view(torch.int16))


# ---- b ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,act,vfs", V.PARAMS)
def test_b_pad_columns_of_the_observation_images_are_written_and_never_data(h, act, vfs):
    """include/cda_mlp.h gives cda_mlp_prep_rows no strided source (obs is f32[*, 42 n_hist], rows back to back), so the slack of a wider row cannot hold NaN.  It does
    say what the kernel writes: x_rm bf16 [n_rows][KX] "row-major, zero padded" and x_pk, the packed image of the same rows in XT whole feature tiles - both are
    outputs of n_rows whole rows, pad columns included.  So: both buffers start as NaN; after prep_rows every entry is finite, the 42 n_hist data columns are the
    bfloat16 observation and the pad columns (6, 12, 2, 8, 4, 10, 0 of them in x_rm at depths 1, 2, 3, 4, 6, 7, 8; up to the tile in x_pk) exact zeros; and the
    forward, backward and weight gradients on those buffers give bit for bit what they give on buffers that started as zeros."""
    from gym_continuousdoubleauction_amd import mlp
    RAN.setdefault((h, act, vfs), set()).add("b")
    p = _policy(h, act, vfs)
    L, n = p.L, V.N_TRAIN
    x = V.obs(n, h, seed=11)
    d_out = V.d_out_of(n)
    ws = V.full_backward(p, x, d_out, 3, fill=float("nan"))
    xr = ws["x_rm"].float().cpu().view(n, L.KX)
    xp = mlp.unpack_rows(ws["x_pk"], n, 32 * L.XT)
    want = x.to(torch.bfloat16).float()
    assert bool(torch.isfinite(xr).all()) and bool(torch.isfinite(xp).all())
    assert torch.equal(xr[:, :L.OBS], want) and bool((xr[:, L.OBS:] == 0).all()) and xr.shape[1] - L.OBS == (6, 12, 2, 8, None, 4, 10, 0)[h - 1]
    assert torch.equal(xp[:, :L.OBS], want) and bool((xp[:, L.OBS:] == 0).all())
    z = V.full_backward(p, x, d_out, 3, fill=0.0)
    for k, m in (("x_rm", n * L.KX), ("x_pk", n * 32 * L.XT), ("h1p", n * 512), ("h2p", n * 512), ("dz1p", n * 512), ("dz2p", n * 512)):          # (rows past n: scratch)
        assert torch.equal(ws[k][:m].view(torch.int16), z[k][:m].view(torch.int16)), k
    assert torch.equal(ws["out"][:n].view(torch.int32), z["out"][:n].view(torch.int32)) and torch.equal(ws["grad"].view(torch.int32), z["grad"].view(torch.int32))
    assert bool(torch.isfinite(ws["grad"]).all()) and float(ws["grad"][L.OFF_W1:L.OFF_B1].abs().max()) > 0


# ---- c ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,act,vfs", V.PARAMS)
def test_c_backward_and_weight_gradients_equal_the_rounded_reference(h, act, vfs):
    """backward, the weight-gradient jobs of this depth (three row chunks, NaN slabs) and the reduction against mlp.reference_gradients on the kernel's own stored
    images: dz2 / dz1 within one / two bfloat16 ulps of the largest entry, every parameter block within 1e-4 of the float64 contraction of the kernel's own packed
    operands and within 2e-2 of the reference's (tests/test_hip_activation.py's bounds)"""
    from gym_continuousdoubleauction_amd import mlp
    RAN.setdefault((h, act, vfs), set()).add("c")
    n, chunks = V.N_TRAIN, 3
    p = _policy(h, act, vfs)
    L = p.L
    x = V.obs(n, h, seed=11)
    d_out = V.d_out_of(n)
    ws = V.full_backward(p, x, d_out, chunks)
    h1, h2 = V.images(ws, n)
    xb = mlp.unpack_rows(ws["x_pk"], n, 32 * L.XT)[:, :L.OBS].double()
    gref, dz1, dz2 = mlp.reference_gradients(p.theta, xb, h1, h2, d_out, activation=act, vf_share_layers=vfs)
    k2, k1 = mlp.unpack_rows(ws["dz2p"][:n * 512], n, 512, paired=True).double(), mlp.unpack_rows(ws["dz1p"][:n * 512], n, 512, paired=True).double()
    if vfs:                                                       # (the value half of a shared trunk's images is not the kernels' to write)
        k1[:, H:] = 0; k2[:, H:] = 0
    e2, e1 = float((k2 - dz2).abs().max()), float((k1 - dz1).abs().max())
    print(f"\n[mlp variants] {V.variant_id((h, act, vfs))} backward: dz2 {e2 / float(dz2.abs().max()):.3g} dz1 {e1 / float(dz1.abs().max()):.3g} of the largest entry")
    assert e2 <= 2 ** -7 * float(dz2.abs().max()) and e1 <= 2 ** -6 * float(dz1.abs().max())
    if act == "relu":                                             # relu'(z) = 0 where the stored h is 0: those dz are exact zeros
        assert bool((k2[h2 == 0] == 0).all()) and bool((k1[h1 == 0] == 0).all())
    g_mine = torch.zeros(L.PARAMS, dtype=torch.float64)
    g_mine[L.OFF_W1:L.OFF_B1] = (k1.t() @ xb).reshape(-1); g_mine[L.OFF_B1:L.OFF_W2] = k1.sum(0)
    g_mine[L.OFF_W2:L.OFF_B2] = torch.stack([k2[:, :256].t() @ h1[:, :256], k2[:, 256:].t() @ h1[:, 256:]]).reshape(-1); g_mine[L.OFF_B2:L.OFF_WO] = k2.sum(0)
    g_mine[L.OFF_WO:L.OFF_LS] = gref[L.OFF_WO:L.OFF_LS]
    grad = ws["grad"].cpu().double()
    assert bool(torch.isfinite(grad).all())
    if vfs:
        for a, b in mlp.value_half(L):
            assert bool((grad[a:b] == 0).all())
        wo = grad[L.OFF_WO:L.OFF_BO].view(32, H)
        assert float(wo[24].abs().max()) > 0 and bool((wo[27:] == 0).all())
    for lo, hi, name in V.blocks_of(L):
        err = float((grad[lo:hi] - g_mine[lo:hi]).abs().max())
        assert err <= 1e-4 * float(g_mine[lo:hi].abs().max()) + 1e-12, (name, err, float(g_mine[lo:hi].abs().max()))
        err = float((grad[lo:hi] - gref[lo:hi]).abs().max())
        assert err <= 2e-2 * float(gref[lo:hi].abs().max()), (name, err, float(gref[lo:hi].abs().max()))


# ---- d ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,act,vfs", V.PARAMS)
def test_d_fused_forward_loss_backward_equals_the_separate_kernels(h, act, vfs):
    """tests/test_hip_activation.py's test of the same name at the smallest shape that still has a ragged last tile and episode ends: 40 markets x 8 steps = 320
    rows (2.5 tiles of the separate kernels' 128 rows), five agents dealt round the sampler's four lanes, max_step 4.  The policy carries no log-std head: the
    head trains on the fused kernel only, it has no separate-kernel twin"""
    from gym_continuousdoubleauction_amd import CDAVecEnv, mlp
    from gym_continuousdoubleauction_amd._lib import check
    RAN.setdefault((h, act, vfs), set()).add("d")
    N, T, A = 40, 8, 5
    env = CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 4, "is_render": False, "auto_reset": True, "n_hist": h}, n_markets=N, with_info=False)
    p = _policy(h, act, vfs, sd=False, seed=37, scale=1.0)
    env.reset(seed=11)
    roll = mlp.RolloutChains(env, p, T, groups=2, seed=6)
    buf = roll.run()
    records = roll.gae(gamma=0.99, lam=0.95, reward_scale=1e-3)
    torch.cuda.synchronize()
    assert int((buf["terminated"] | buf["truncated"]).sum()) >= N           # episode ends inside the rollout
    R_ = T * N
    obs = buf["obs"][:T].view(R_, -1)
    perm = torch.randperm(R_, generator=torch.Generator().manual_seed(3))
    img = (lambda t: V.trunk_tiles(t, R_)) if vfs else (lambda t: t[:R_ * 512])
    res = []
    for fused in (False, True):
        upd = mlp.FusedUpdate(p, R_, R_, A, chunks=3, fused=fused)
        upd.perm.copy_(perm)
        if not fused:
            check(p.L.fn("cda_mlp_prep_rows")(obs.data_ptr(), upd.perm.data_ptr(), R_, upd.x_rm.data_ptr(), upd.x_pk.data_ptr(), torch.cuda.current_stream().cuda_stream), "prep")
        upd.minibatch_step(0, R_, None, None, None, None, 0.2, 0.5, 0.01, 0.0, (0.9, 0.999), 1e-8, 0.5, records=records, obs_rows=obs if fused else None, debug_outputs=True)
        torch.cuda.synchronize()
        res.append(dict(out=upd.out[:R_].clone(), d_out=upd.d_out[:R_].clone(), grad=upd.grad.clone(), out6=upd.out6.clone(),
                        h1=img(upd.h1p).clone(), h2=img(upd.h2p).clone(), dz2=img(upd.dz2p).float().clone(), dz1=img(upd.dz1p).float().clone()))
    a, b = res
    assert torch.equal(a["h1"].view(torch.int16), b["h1"].view(torch.int16)) and torch.equal(a["h2"].view(torch.int16), b["h2"].view(torch.int16))
    assert torch.equal(a["out"][:, :25], b["out"][:, :25])
    assert float(a["d_out"][:, 24].abs().max()) > 0
    assert torch.allclose(a["d_out"], b["d_out"], rtol=2e-4, atol=2e-5 * float(a["d_out"].abs().max()))
    for k in ("dz2", "dz1"):
        assert (a[k] - b[k]).abs().max() <= 2e-2 * a[k].abs().max()
    assert torch.allclose(a["out6"], b["out6"], rtol=1e-4, atol=1e-7) and float(a["out6"][1]) > 0
    assert (a["grad"] - b["grad"]).abs().max() <= 1e-3 * a["grad"].abs().max() and bool(torch.isfinite(a["grad"]).all()) and float(a["grad"].abs().max()) > 0
    if vfs:
        for g in (a["grad"], b["grad"]):
            for lo, hi in mlp.value_half(p.L):
                assert bool((g[lo:hi] == 0).all())
    assert (env.flags() == 0).all()
    env.close()


# ---- e ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,act,vfs", V.PARAMS)
def test_e_sampling_and_greedy_launches_follow_the_restated_law(h, act, vfs):
    """policy_step on 200 rows x 5 agents at draw 7, counter 2^40, seed 2^64 - 1 against tests/sampler_ref.py sample by sample (tests/test_hip_sampler.py's _compare,
    its caps unchanged); its value is the forward's column 24; p.act is the argmax / the means of the same forward (tests/test_hip_evaluate.py's relation).

    The Gaussian deviation is held to GAUSS_BOUND plus each sample's own read-back term (mlp_variants.compare, a_cont_rounding).  Without the term the seven linear
    variants with the head on miss GAUSS_BOUND = 7.6e-6 on an MI355X - h1-linear 4.51e-5, h2-linear-vfs 1.86e-4, h3-linear 1.15e-4, h4-linear-vfs 1.57e-5,
    h6-linear-vfs 4.12e-5, h7-linear 3.08e-5, h8-linear-vfs 6.40e-5: a linear network's head moves log_std to -6 .. -7.4 at rows whose mean is of order 1 - and
    the float32 statement of a_cont = mu + exp(log_std) n on the host, read back the same way, misses it by the same figures to three digits (4.51e-5, 1.86e-4,
    1.15e-4, 1.57e-5, 4.12e-5, 3.00e-5, 6.40e-5): the stored sample's rounding, not the sampler.  With the term no sample of any variant exceeds 1.4e-6 + it."""
    RAN.setdefault((h, act, vfs), set()).add("e")
    N, A, draw, counter, seed = V.N_FWD, 5, 7, 2 ** 40, 2 ** 64 - 1
    sd = V.head_on(h, act, vfs)
    p = _policy(h, act, vfs)
    x = V.obs(N, h, seed=31).to(DEV)
    ctr = torch.full((1,), counter, dtype=torch.int64, device=DEV)
    outs = p.policy_step(x, A, seed=seed, counter=ctr, draw=draw)
    fwd = p.forward(x)
    greedy = p.act(x, A)
    torch.cuda.synchronize()
    out = fwd.cpu().numpy()
    i = np.arange(N * A)
    V.compare(f"variants {V.variant_id((h, act, vfs))} sd{int(sd)}", V.flat(outs), R.rollout_key(seed, counter, draw), i, np.repeat(out, A, axis=0),
              np.repeat(V.log_std_rows(p, out), A, axis=0), a_cont_rounding=True)
    assert torch.equal(outs["value"], fwd[:, 24])
    V.check_mode(greedy, fwd, p.log_std, sd)
    assert torch.equal(greedy["value"], fwd[:, 24])


# ---- f ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,act,vfs", V.PARAMS)
def test_f_league_launches_route_every_slot_to_its_net_of_this_object(h, act, vfs):
    """a PolicyBank of this variant, two trainable nets of different parameters, 64 markets x 4 slots: every slot's sample of cda_mlp_league_step is bit for bit
    what cda_mlp_policy_step of the net that plays it draws at the same key (tests/test_hip_league.py's relation at the default variant), each net's value row is
    its own; the greedy launch (cda_mlp_league_act) gives every slot the mode of its net's forward"""
    from gym_continuousdoubleauction_amd import mlp
    RAN.setdefault((h, act, vfs), set()).add("f")
    N, A, k = 64, 4, 2
    sd = V.head_on(h, act, vfs)
    bank = mlp.PolicyBank(DEV, N, A, k, max_frozen=1, seed=3, random_seed=4242, n_hist=h, state_dependent_log_std=sd, activation=act, vf_share_layers=vfs)
    assert bank.L.suffix == V.object_name(h, act, vfs)[len("cda_mlp"):]
    for q in range(k):
        bank.policies[q].theta.copy_(V.theta(h, vfs, V.seed_of(h) + 100 * q, 2.0, sd)); bank.policies[q].pack()
    sn = torch.randint(0, k, (N, A), generator=torch.Generator().manual_seed(9), dtype=torch.int32)
    sn[:, 0], sn[:, 1] = 0, 1
    bank.set_slots(sn)
    x = V.obs(N, h, seed=31).to(DEV)
    ctr = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    o = {kk: v.clone() for kk, v in bank.act(x, 77, ctr, 3, greedy=False).items()}
    g = {kk: v.clone() for kk, v in bank.act(x, 77, ctr, 3, greedy=True).items()}
    torch.cuda.synchronize()
    assert not torch.equal(bank.theta[0], bank.theta[1])
    pols = [mlp.FusedPolicy(DEV, theta=bank.theta[net].cpu(), activation=act, vf_share_layers=vfs) for net in range(k)]
    refs = [{kk: v.clone() for kk, v in pol.policy_step(x, A, seed=77, counter=ctr, draw=3).items()} for pol in pols]
    torch.cuda.synchronize()
    for net, (pol, ref) in enumerate(zip(pols, refs)):
        assert torch.equal(pol.wb, bank.wb[net]) and pol.state_dependent_log_std == sd
        fwd = pol.forward(x)
        torch.cuda.synchronize()
        mask = (sn == net).to(DEV)
        assert int(mask.sum()) > 50
        for key in ("category", "size_mean", "size_sigma", "price", "price_offset", "logp", "a_cont"):
            assert torch.equal(o[key][mask], ref[key][mask]), (net, key)
        assert not torch.equal(o["logp"][mask], refs[1 - net]["logp"][mask])          # (... and not what the other net draws there)
        assert torch.equal(o["value"][net], ref["value"]) and torch.equal(g["value"][net], fwd[:, 24])
        for a in range(A):
            rows = torch.nonzero(sn[:, a] == net).view(-1).to(DEV)
            if len(rows):
                V.check_mode({kk: v[rows][:, a:a + 1] for kk, v in g.items() if kk != "value"}, fwd[rows], pol.log_std, sd)


# ---- g ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _chain_env(h, N, A):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    return CDAVecEnv({"num_of_agents": A, "init_cash": 1000000, "max_step": 4, "is_render": False, "auto_reset": True, "n_hist": h}, n_markets=N, with_info=False)


STEP_KEYS = ("category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp")


@pytest.mark.parametrize("h,act,vfs", V.PARAMS)
def test_g_every_entry_point_is_launched_for_this_variant(h, act, vfs):
    """the entry points of include/cda_mlp.h with no relation of their own in (a) .. (f), each held to the cheapest relation its own test holds at the default
    variant - the MFMA self-test (tests/test_hip_mlp.py); cda_mlp_values / _values_counted = the forward's column 24 bit for bit (tests/test_hip_league.py);
    reduce + apply = the one-call Adam step to tests/test_hip_dp.py's bounds; the league's sampled chain, the greedy chain and the league's greedy chain record
    at every step what one launch on that step's observation gives (tests/test_hip_league.py, tests/test_hip_evaluate.py) - and then: every name of
    _lib.MLP_SYMBOLS was launched for this variant by this file."""
    from gym_continuousdoubleauction_amd import _lib, mlp
    from gym_continuousdoubleauction_amd._lib import check
    key = (h, act, vfs)
    sd = V.head_on(h, act, vfs)
    p = _policy(h, act, vfs)
    L = p.L
    st = torch.cuda.current_stream().cuda_stream
    # the operand / accumulator conventions of this object's copy of the MFMA self-test
    gen = torch.Generator().manual_seed(1)
    a, b, d = torch.randn(32, 16, generator=gen).numpy().astype(np.float32), torch.randn(16, 32, generator=gen).numpy().astype(np.float32), np.zeros((32, 32), np.float32)
    check(L.fn("cda_mlp_selftest_mfma")(0, a.ctypes.data, b.ctypes.data, d.ctypes.data), "cda_mlp_selftest_mfma")
    want = torch.from_numpy(a).to(torch.bfloat16).double().numpy() @ torch.from_numpy(b).to(torch.bfloat16).double().numpy()
    assert np.abs(d - want).max() <= 1e-5 * np.abs(want).max() + 1e-6
    # the value launches: all rows, and the first *count rows of a device-side count
    n, count = V.N_FWD, 70
    x = V.obs(n, h, seed=41).to(DEV)
    col = p.forward(x)[:, 24].clone()
    v_all, v_cnt = torch.full((n,), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)
    cnt_dev = torch.full((1,), count, dtype=torch.int32, device=DEV)
    check(L.fn("cda_mlp_values")(p.wb.data_ptr(), p.theta.data_ptr(), 1, x.data_ptr(), n, v_all.data_ptr(), n, st), "cda_mlp_values")
    check(L.fn("cda_mlp_values_counted")(p.wb.data_ptr(), p.theta.data_ptr(), 1, x.data_ptr(), n, cnt_dev.data_ptr(), v_cnt.data_ptr(), n, st), "cda_mlp_values_counted")
    torch.cuda.synchronize()
    assert torch.equal(v_all, col) and torch.equal(v_cnt[:count], col[:count])
    # reduce + apply (a data-parallel learner's two halves, the collective between them the identity) against the one-call step
    Rr, A, lr = 64, 4, 1e-3
    xr, rec = V.obs(Rr, h, seed=17).to(DEV) * 0.5, V.records(Rr, A).to(DEV)
    th0 = p.theta.cpu().clone()
    steps = []
    for allreduce in (None, lambda t: t):
        q = mlp.FusedPolicy(DEV, theta=th0, activation=act, vf_share_layers=vfs)
        upd = mlp.FusedUpdate(q, Rr, Rr, A, chunks=2, allreduce=allreduce, world=1)
        upd.perm.copy_(torch.arange(Rr))
        upd.minibatch_step(0, Rr, None, None, None, None, 0.2, 0.5, 0.01, lr, (0.9, 0.999), 1e-8, 0.5, records=(rec, None, 0), obs_rows=xr)
        torch.cuda.synchronize()
        steps.append((q.theta.cpu().double(), upd.grad.cpu().double(), float(upd.norm2[2]), float(q.adam_step.item())))
    (tw, gw, nw, sw), (tg, gg, ng, sg) = steps
    moved = (tw - th0.double()).norm()
    assert sw == sg == 1.0 and float(gw.norm()) > 0 and (gg - gw).norm() <= 2e-4 * gw.norm() and abs(ng - nw) <= 1e-3 * nw
    assert float((tw - th0.double()).abs().max()) > 0.5 * lr and (tg - tw).norm() <= 0.02 * moved
    # the three chains that (d) does not run, two steps each on one small env
    N, T, seed = 32, 2, 99
    env = _chain_env(h, N, A)
    bank = mlp.PolicyBank(DEV, N, A, 1, max_frozen=1, seed=3, random_seed=77, n_hist=h, state_dependent_log_std=sd, activation=act, vf_share_layers=vfs)
    bank.policies[0].theta.copy_(p.theta); bank.policies[0].pack()
    slots = torch.full((N, A), mlp.LEAGUE_RANDOM, dtype=torch.int32)
    slots[:, 0] = 0
    slots[::2, 2] = 0
    bank.set_slots(slots)
    for pol, greedy in ((bank, False), (p, True), (bank, True)):
        env.reset(seed=700)
        roll = mlp.RolloutChains(env, pol, T, groups=1, seed=seed, use_graphs=False, greedy=greedy)
        buf = roll.run()
        torch.cuda.synchronize()
        cnt = roll.counter.clone()
        for t in range(T):
            if pol is bank:
                o = bank.act(buf["obs"][t], seed, cnt, t, greedy=greedy)
                value = buf["value"][0, t]
            else:
                o = p.act(buf["obs"][t], A)
                value = buf["value"][t]
            torch.cuda.synchronize()
            for kk in STEP_KEYS:
                assert torch.equal(o[kk].view(torch.int32), buf[kk][t].view(torch.int32)), (greedy, pol is bank, kk, t)
            assert torch.equal(value, p.forward(buf["obs"][t])[:, 24])
        assert torch.equal(buf["value"][0, T] if pol is bank else buf["value"][T], p.forward(buf["obs"][T])[:, 24])          # the bootstrap value
    assert (env.flags() == 0).all()
    env.close()
    own = {"cda_mlp_selftest_mfma", "cda_mlp_values", "cda_mlp_values_counted", "cda_mlp_reduce", "cda_mlp_apply", "cda_mlp_league_rollout_chain", "cda_mlp_eval_chain",
           "cda_mlp_league_eval_chain"}
    called = CALLED.get(key, set())
    assert own <= called, sorted(own - called)
    if RAN.get(key, set()) >= set(CHECKS):                        # (a) .. (f) ran for this variant in this process (the whole file): every entry point was launched
        missing = set(_lib.MLP_SYMBOLS) - called
        assert not missing, (V.variant_id(key), sorted(missing))


def test_g_the_walk_covered_every_variant_it_ran():
    """at the end of the module: no variant for which all seven checks ran misses an entry point, and the notes name no variant outside the table"""
    from gym_continuousdoubleauction_amd import _lib
    assert set(CALLED) <= set(V.VARIANTS)
    for key, ran in RAN.items():
        if ran >= set(CHECKS) and "cda_mlp_selftest_mfma" in CALLED.get(key, set()):
            assert set(_lib.MLP_SYMBOLS) <= CALLED[key], (V.variant_id(key), sorted(set(_lib.MLP_SYMBOLS) - CALLED[key]))
