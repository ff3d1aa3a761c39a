"""CPU: the shared-trunk network (RLlib's `vf_share_layers = True`: one encoder, the pi heads and the value head both read its last layer) on the host side -
the PyTorch statement against a plain RLlib-shaped module and the float64 reference the GPU tests hold the kernels to, the parameter-vector conventions
(the value half is exact zeros, output row 24 reads the policy half), policy files, checkpoint arguments, and the shared-trunk objects of the built library
(entry points <name>[_h<H>][_<act>]_vfs, include/cda_mlp.h CDA_MLP_VFS_VARIANTS)."""
import ctypes as C
import os
import re
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ("tanh", "relu", "elu", "linear")
H = 256


def _obs(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 168, generator=g) * 1.5
    x[:, ::7] = 0.0
    return x


def _rllib_module(m, act):
    """the RLlib shape of a shared-trunk PPO module (torch framework): an encoder nn.Sequential of fcnet_hiddens / fcnet_activation, a linear pi head and a linear
    value head on its output - with the weights of ActorCritic `m` copied in"""
    a = {"tanh": nn.Tanh(), "relu": nn.ReLU(), "elu": nn.ELU(), "linear": nn.Identity()}[act]
    enc = nn.Sequential(nn.Linear(168, H), a, nn.Linear(H, H), a).double()
    n_pi = 24 + (2 if m.state_dependent_log_std else 0)
    pi, vf = nn.Linear(H, n_pi).double(), nn.Linear(H, 1).double()
    rows = list(range(24)) + ([25, 26] if m.state_dependent_log_std else [])
    with torch.no_grad():
        enc[0].weight.copy_(m.l1.weight[:H]); enc[0].bias.copy_(m.l1.bias[:H])
        enc[2].weight.copy_(m.l2.weight[:H, :H]); enc[2].bias.copy_(m.l2.bias[:H])
        pi.weight.copy_(m.out.weight[rows, :H]); pi.bias.copy_(m.out.bias[rows])
        vf.weight.copy_(m.out.weight[24:25, :H]); vf.bias.copy_(m.out.bias[24:25])
    return enc, pi, vf, rows


@pytest.mark.parametrize("sd", (False, True))
@pytest.mark.parametrize("act", ACTS)
def test_actor_critic_equals_the_rllib_shaped_module(act, sd):
    """ppo.ActorCritic(vf_share_layers=True) in float64 equals nn.Sequential trunk + two nn.Linear heads: outputs, and the autograd gradient of every trunk and head
    parameter for a loss on all outputs (the value's part reaches the trunk); the value half of the block matrices gets an exact-zero gradient"""
    from gym_continuousdoubleauction_amd import ppo
    torch.manual_seed(1)
    m = ppo.ActorCritic(168, activation=act, state_dependent_log_std=sd, vf_share_layers=True).double()
    assert m.vf_share_layers and bool((m.l1.weight[H:] == 0).all()) and bool((m.l1.bias[H:] == 0).all())
    assert bool((m.l2.weight[H:] == 0).all()) and bool((m.l2.weight[:, H:] == 0).all()) and bool((m.l2.bias[H:] == 0).all())
    assert bool((m.out.weight[24, H:] == 0).all()) and bool((m.out.weight[24, :H] != 0).any())
    enc, pi, vf, rows = _rllib_module(m, act)
    x = _obs(48).double()
    g = torch.Generator().manual_seed(2)
    w_pi, w_v = torch.randn(48, len(rows), generator=g, dtype=torch.float64), torch.randn(48, generator=g, dtype=torch.float64)
    o = m.trunk_packed(x)
    z = enc(x)
    p_ref, v_ref = pi(z), vf(z)[:, 0]
    assert torch.allclose(o[:, rows], p_ref, rtol=1e-12, atol=1e-12) and torch.allclose(o[:, 24], v_ref, rtol=1e-12, atol=1e-12)
    ((o[:, rows] * w_pi).sum() + (o[:, 24] * w_v).sum()).backward()
    ((p_ref * w_pi).sum() + (v_ref * w_v).sum()).backward()
    pairs = ((m.l1.weight.grad[:H], enc[0].weight.grad), (m.l1.bias.grad[:H], enc[0].bias.grad), (m.l2.weight.grad[:H, :H], enc[2].weight.grad),
             (m.l2.bias.grad[:H], enc[2].bias.grad), (m.out.weight.grad[rows, :H], pi.weight.grad), (m.out.bias.grad[rows], pi.bias.grad),
             (m.out.weight.grad[24:25, :H], vf.weight.grad), (m.out.bias.grad[24:25], vf.bias.grad))
    for a, b in pairs:
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-12), float((a - b).abs().max())
    for dead in (m.l1.weight.grad[H:], m.l1.bias.grad[H:], m.l2.weight.grad[H:], m.l2.weight.grad[:, H:], m.l2.bias.grad[H:], m.out.weight.grad[:, H:]):
        assert bool((dead == 0).all())


def test_value_half_stays_zero_under_the_optimiser():
    from gym_continuousdoubleauction_amd import ppo
    torch.manual_seed(3)
    m = ppo.ActorCritic(168, vf_share_layers=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    x = _obs(64)
    for _ in range(5):
        opt.zero_grad()
        o = m.trunk_packed(x)
        (o[:, :24].square().mean() + (o[:, 24] - 1).square().mean()).backward()
        opt.step()
    assert bool((m.l1.weight[H:] == 0).all()) and bool((m.l1.bias[H:] == 0).all()) and bool((m.l2.bias[H:] == 0).all())
    assert bool((m.l2.weight[H:] == 0).all()) and bool((m.l2.weight[:, H:] == 0).all()) and bool((m.out.weight[24, H:] == 0).all())


@pytest.mark.parametrize("act", ACTS)
def test_reference_math_equals_float64_autograd(act):
    """reference_outputs / reference_gradients(vf_share_layers=True) against float64 autograd through ActorCritic(vf_share_layers=True); the value column depends
    on the trunk (it differs from the separate network's on the same theta) and the value half's gradient is exact zeros"""
    from gym_continuousdoubleauction_amd import mlp
    th = mlp.init_theta(generator=torch.Generator().manual_seed(7), vf_share_layers=True)
    th[:mlp.OFF_LS] *= 2.0
    th = mlp._r(th.double())
    x = mlp._r(_obs(96, seed=8).double())
    m = mlp.actor_critic_from_theta(th, dtype=torch.float64, activation=act, vf_share_layers=True)
    out = m.trunk_packed(x)
    want_out = mlp.reference_outputs(th, x, emulate_bf16=False, activation=act, vf_share_layers=True)
    assert torch.allclose(out.detach(), want_out, rtol=1e-12, atol=1e-12)
    sep = mlp.reference_outputs(th, x, emulate_bf16=False, activation=act)
    assert float((sep[:, 24] - want_out[:, 24]).abs().max()) > 1e-3 and torch.equal(sep[:, :24], want_out[:, :24])
    d_out = torch.zeros(96, 32, dtype=torch.float64)
    d_out[:, :25] = mlp._r(torch.randn(96, 25, generator=torch.Generator().manual_seed(9), dtype=torch.float64))
    (out * d_out).sum().backward()
    want = torch.zeros(mlp.PARAMS, dtype=torch.float64)
    want[mlp.OFF_W1:mlp.OFF_B1] = m.l1.weight.grad.reshape(-1); want[mlp.OFF_B1:mlp.OFF_W2] = m.l1.bias.grad
    w2g = m.l2.weight.grad
    want[mlp.OFF_W2:mlp.OFF_B2] = torch.stack([w2g[:H, :H], w2g[H:, H:]]).reshape(-1); want[mlp.OFF_B2:mlp.OFF_WO] = m.l2.bias.grad
    blk = torch.zeros(32, H, dtype=torch.float64); blk[:25] = m.out.weight.grad[:25, :H]
    want[mlp.OFF_WO:mlp.OFF_BO] = blk.reshape(-1); want[mlp.OFF_BO:mlp.OFF_LS] = m.out.bias.grad
    _, xb, h1, h2 = mlp.reference_outputs(th, x, emulate_bf16=False, keep=True, activation=act, vf_share_layers=True)
    got, dz1, dz2 = mlp.reference_gradients(th, xb, h1, h2, d_out, activation=act, vf_share_layers=True)
    L = mlp.layout(4)
    for lo, hi, name in ((L.OFF_W1, L.OFF_B1, "W1"), (L.OFF_B1, L.OFF_W2, "b1"), (L.OFF_W2, L.OFF_B2, "W2"), (L.OFF_B2, L.OFF_WO, "b2"),
                         (L.OFF_WO, L.OFF_BO, "Wo"), (L.OFF_BO, L.OFF_LS, "bo")):
        a, b = got[lo:hi], want[lo:hi]
        assert (a - b).norm() <= 1e-2 * b.norm() + 1e-12, (act, name, float((a - b).norm() / b.norm()))
    for a, b in mlp.value_half(L):
        assert bool((got[a:b] == 0).all()) and bool((want[a:b] == 0).all())
    assert bool((dz1[:, H:] == 0).all()) and bool((dz2[:, H:] == 0).all())
    # the value loss reaches the trunk: a d_out on column 24 alone moves W1's policy rows
    d_v = torch.zeros_like(d_out); d_v[:, 24] = 1.0
    g_v, _, _ = mlp.reference_gradients(th, xb, h1, h2, d_v, activation=act, vf_share_layers=True)
    assert float(g_v[L.OFF_W1:L.OFF_W1 + H * L.OBS].abs().max()) > 0


@pytest.mark.parametrize("sd", (False, True))
def test_theta_round_trips_and_init_zeroes_the_value_half(sd):
    from gym_continuousdoubleauction_amd import mlp, ppo
    for h in (4, 6):
        L = mlp.layout(h)
        th = mlp.init_theta(42 * h, generator=torch.Generator().manual_seed(h), state_dependent_log_std=sd, vf_share_layers=True)
        assert th.numel() == L.PARAMS and mlp.value_half_is_zero(th)
        for a, b in mlp.value_half(L):
            assert bool((th[a:b] == 0).all()) and b > a
        wo = th[L.OFF_WO:L.OFF_BO].view(32, H)
        assert bool((wo[24] != 0).any()) and float(th[L.OFF_BO + 24]) != 0.0 and mlp.has_log_std_head(th) == sd
        assert mlp.hidden_widths(th) == (256, 256)
        m = mlp.actor_critic_from_theta(th, vf_share_layers=True)
        assert m.vf_share_layers and torch.equal(mlp.theta_from_actor_critic(m), th)
    # a fresh torch module round-trips too, and narrow widths are dead units inside the trunk
    torch.manual_seed(4)
    m = ppo.ActorCritic(168, vf_share_layers=True, state_dependent_log_std=sd)
    th = mlp.theta_from_actor_critic(m)
    assert mlp.value_half_is_zero(th)
    assert torch.equal(mlp.theta_from_actor_critic(mlp.actor_critic_from_theta(th, vf_share_layers=True)), th)
    narrow = mlp.init_theta(generator=torch.Generator().manual_seed(5), hidden=(64, 128), vf_share_layers=True)
    assert mlp.hidden_widths(narrow) == (64, 128) and mlp.value_half_is_zero(narrow)
    with pytest.raises(ValueError, match="value half"):
        mlp.actor_critic_from_theta(mlp.init_theta(generator=torch.Generator().manual_seed(6)), vf_share_layers=True)


def test_layout_suffixes():
    from gym_continuousdoubleauction_amd import mlp
    assert mlp.layout(4).suffix == "" and mlp.layout(4, vf_share_layers=True).suffix == "_vfs"
    assert mlp.layout(6, "elu", True).suffix == "_h6_elu_vfs" and mlp.layout(8, "tanh", True).suffix == "_h8_vfs" and mlp.layout(4, "relu", True).suffix == "_relu_vfs"
    assert mlp.layout(4, vf_share_layers=True).PARAMS == mlp.PARAMS and mlp.layout(4, vf_share_layers=True).vf_share_layers
    assert mlp.layout(4) is not mlp.layout(4, vf_share_layers=True) and not mlp.layout(4).vf_share_layers


def test_policy_files_carry_the_flag_and_refuse_a_live_value_half(tmp_path):
    from gym_continuousdoubleauction_amd import mlp
    th = mlp.init_theta(generator=torch.Generator().manual_seed(2), vf_share_layers=True)
    rec = mlp.policy_record(th, vf_share_layers=True)
    assert rec["vf_share_layers"] is True and rec["hidden"] == [256, 256]
    path = str(tmp_path / "shared.pt")
    torch.save(rec, path)
    got, act, vfs = mlp.read_policy(path, with_activation=True, with_vf_share_layers=True)
    assert torch.equal(got, th) and act == "tanh" and vfs is True
    assert mlp.read_policy(path, with_vf_share_layers=True)[1] is True and torch.equal(mlp.read_policy(path), th)
    # a file of separate networks carries no key: its dict is what it was
    sep = mlp.init_theta(generator=torch.Generator().manual_seed(3))
    r0 = mlp.policy_record(sep)
    assert set(r0) == {"format", "version", "theta", "n_hist", "hidden", "state_dependent_log_std"}
    torch.save(r0, str(tmp_path / "sep.pt"))
    assert mlp.read_policy(str(tmp_path / "sep.pt"), with_vf_share_layers=True)[1] is False
    # claiming a shared trunk with a non-zero value half is refused, on reading and on writing; the flag must be a bool
    bad = dict(r0, vf_share_layers=True)
    torch.save(bad, str(tmp_path / "bad.pt"))
    with pytest.raises(ValueError, match="value half"):
        mlp.read_policy(str(tmp_path / "bad.pt"))
    with pytest.raises(ValueError, match="value half"):
        mlp.policy_record(sep, vf_share_layers=True)
    one = th.clone(); one[mlp.OFF_B2 + 300] = 1e-6
    with pytest.raises(ValueError):
        mlp.check_policy_record(dict(rec, theta=one))
    torch.save(dict(rec, vf_share_layers=1), str(tmp_path / "int.pt"))
    with pytest.raises(ValueError, match="bool"):
        mlp.read_policy(str(tmp_path / "int.pt"))


def test_checkpoint_arguments_add_the_key_for_shared_trunks_only():
    from gym_continuousdoubleauction_amd import checkpoint as CK
    old = {"markets": 64, "agents": 4, "horizon": 32, "hidden": [256, 256], "seed": 0}
    assert CK.with_vf_share_layers(old, False) == old
    shared = CK.with_vf_share_layers(old, True)
    assert shared == dict(old, vf_share_layers=True)
    with pytest.raises(ValueError, match="vf_share_layers"):
        CK.check_args(old, shared)
    with pytest.raises(ValueError, match="vf_share_layers"):
        CK.check_args(shared, old)
    CK.check_args(shared, CK.with_vf_share_layers(old, True))
    both = CK.with_vf_share_layers(CK.with_activation(old, "elu"), True)
    assert both == dict(old, activation="elu", vf_share_layers=True)


@pytest.fixture(scope="module")
def hip_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_hip()
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib(), _lib


def _suffixes(_lib):
    return [d + a + "_vfs" for d in [""] + [f"_h{h}" for h in _lib.MLP_HIST_VARIANTS] for a in [""] + ["_" + x for x in _lib.MLP_ACT_VARIANTS]]


def test_every_entry_point_exists_as_a_shared_trunk(hip_lib):
    """include/cda_mlp.h CDA_MLP_VFS_VARIANTS; the library exports <name>[_h<H>][_<act>]_vfs for every declared name, every compiled depth and activation, and
    mlp.layout(h, a, vf_share_layers=True) resolves to them"""
    from gym_continuousdoubleauction_amd import mlp
    L, _lib = hip_lib
    hdr = open(os.path.join(ROOT, "include", "cda_mlp.h")).read()
    assert re.search(r'#define CDA_MLP_VFS_VARIANTS "vfs"', hdr)
    declared = set(re.findall(r"^(?:int|int32_t)\s+(cda_[a-z0-9_]+)\s*\(", hdr, flags=re.M))
    assert len(_suffixes(_lib)) == 28 and set(_suffixes(_lib)) <= set(_lib.mlp_variant_suffixes())
    so = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        for sfx in _suffixes(_lib):
            getattr(so, name + sfx)
    for h in mlp.HIST_VARIANTS:
        for a in mlp.ACTIVATIONS:
            name = "cda_mlp_forward" + ("" if h == 4 else f"_h{h}") + ("" if a == "tanh" else "_" + a) + "_vfs"
            assert mlp.layout(h, a, True).fn("cda_mlp_forward") is getattr(L, name)


def test_shared_trunk_entry_points_refuse_null_arguments_without_a_device(hip_lib):
    """every _vfs entry point has the base signature and returns CDA_ERR_INVALID on NULL arguments (no device touched); the weight-gradient job count is the
    trunk's own (no dW2 block 1, no value panels of dW1): two fewer halves' jobs than the separate network's"""
    L, _lib = hip_lib
    INVALID = -1

    def zero(t):
        if t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer)):
            return None
        return 0.0 if t in (C.c_float, C.c_double) else 0
    for name in _lib.MLP_SYMBOLS:
        for sfx in _suffixes(_lib):
            fn = getattr(L, name + sfx)
            assert fn.argtypes == getattr(L, name).argtypes
            if not fn.argtypes:
                base = getattr(L, name + sfx[:-4])()
                if name == "cda_mlp_wgrad_jobs":
                    assert fn() == (base - 1) // 2 + 1 and fn() < base, (sfx, fn(), base)
                else:
                    assert fn() == base
                continue
            assert fn(*[zero(t) for t in fn.argtypes]) == INVALID, name + sfx
