"""CPU: behaviour cloning's C-ABI (include/cda_imitate.h) is declared, bound once and validates before it launches; the numpy statements of its two kernels
(imitate.records_spec, imitate.bc_loss_spec) hold what they claim - the inverse squash round-trips, the loss gradient equals float64 autograd of the same loss
written with torch.distributions; the command lines parse."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "include", "cda_imitate.h")
INVALID = -1


@pytest.fixture(scope="module")
def hip_lib():
    import __graft_entry__ as g
    g.build_hip()
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib(), _lib


def test_the_header_s_symbols_are_bound_once_and_have_no_variants(hip_lib):
    L, _lib = hip_lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cda_[a-z_0-9]+)\s*\(", txt)))
    assert declared == sorted(_lib.IMITATE_SYMBOLS) and len(declared) == 2
    assert '#include "cda_learner.h"' in txt
    for other in (_lib.SYMBOLS, _lib.MLP_SYMBOLS, _lib.LEARNER_SYMBOLS):
        assert not set(_lib.IMITATE_SYMBOLS) & set(other)
    for hdr in ("cda_learner.h", "cda_mlp.h", "cda.h"):                         # declared in their own header only
        other = open(os.path.join(ROOT, "include", hdr)).read()
        assert not any(re.search(r"\b%s\s*\(" % name, other) for name in declared), hdr
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines()
    exported = [ln.split()[-1] for ln in syms if ln.strip()]
    from gym_continuousdoubleauction_amd import mlp
    for name in declared:
        assert exported.count(name) == 1 and getattr(L, name).argtypes
        assert [e for e in exported if e.startswith(name)] == [name]             # no _h<H> / _<act> / _vfs copy
        assert mlp.layout(2, "relu", True).fn(name) is getattr(L, name) and mlp.layout(4).fn(name) is getattr(L, name)


def test_both_entry_points_refuse_bad_arguments_before_touching_the_device(hip_lib):
    L, _lib = hip_lib

    def zero(t):
        return None if t is C.c_void_p else (0.0 if t in (C.c_float, C.c_double) else 0)
    for name in _lib.IMITATE_SYMBOLS:
        fn = getattr(L, name)
        assert fn(*[zero(t) for t in fn.argtypes]) == INVALID, name
    one, odd = C.c_void_p(64), C.c_void_p(72)                                   # non-NULL, never dereferenced: validation fails first (72: not 16-byte aligned)

    def records(T=4, N=8, A=4, rec=one, cat=one, stats=one, src=one):
        return L.cda_bc_records(cat, one, one, one, one, None, src, one, T, N, A, rec, stats, None)
    assert records(T=0) == INVALID and records(N=0) == INVALID and records(A=0) == INVALID and records(A=17) == INVALID
    assert records(rec=odd) == INVALID and records(rec=None) == INVALID and records(cat=None) == INVALID and records(stats=None) == INVALID and records(src=None) == INVALID

    def loss(rows=64, A=4, stride=32, rec=one, out=one, d_out=one, sums=one, out6=one, norm_rows=0):
        return L.cda_bc_loss_records(out, one, rec, None, rows, A, stride, 0.5, 0.01, 1.0, d_out, sums, out6, norm_rows, 1, 1, None, None, None)
    assert loss(rows=0) == INVALID and loss(A=0) == INVALID and loss(A=17) == INVALID
    assert loss(stride=24) == INVALID and loss(stride=30) == INVALID and loss(stride=20) == INVALID
    assert loss(rec=odd) == INVALID and loss(rec=None) == INVALID and loss(out=None) == INVALID and loss(d_out=None) == INVALID
    assert loss(sums=None) == INVALID and loss(out6=None) == INVALID and loss(norm_rows=-1) == INVALID


def _actions(T, N, A, seed):
    g = np.random.default_rng(seed)
    cat, price, off = g.integers(0, 9, (T, N, A)), g.integers(0, 10, (T, N, A)), g.integers(0, 3, (T, N, A))
    mean, sigma = g.uniform(-1, 1, (T, N, A)).astype(np.float32), g.uniform(0, 1, (T, N, A)).astype(np.float32)
    mean.reshape(-1)[:4] = (0.0, 1.0, -1.0, 0.5)                                # a pass, the Box bounds
    sigma.reshape(-1)[:4] = (0.0, 1.0, 0.0, 1.0)
    cat.reshape(-1)[0] = price.reshape(-1)[0] = 0
    off.reshape(-1)[0] = 1                                                      # the scripted pass (0, 0.0, 0.0, 0, 1)
    return cat.astype(np.int32), price.astype(np.int32), off.astype(np.int32), mean, sigma, g.normal(size=(T, N, A, 2)).astype(np.float32)


def test_records_spec_inverts_the_squash_and_keeps_what_it_must():
    from gym_continuousdoubleauction_amd import imitate as IM
    T, N, A = 3, 5, 4
    cat, price, off, mean, sigma, a_cont = _actions(T, N, A, 1)
    src = np.ones((N, A), np.int32)
    src[:, 0], src[1, 2] = 0, 2
    w = np.random.default_rng(2).choice([0.25, 0.5, 1.0, 2.0], (N, A)).astype(np.float32)
    before = np.full((T, N, A, 8), 7.25, np.float32)
    rec, stats = IM.records_spec(cat, price, off, mean, sigma, a_cont, src, w, rec=before)
    words = rec.view(np.int32)
    assert np.array_equal(words[..., 0], cat) and np.array_equal(words[..., 1], price) and np.array_equal(words[..., 2], off)
    assert np.array_equal(rec[..., 6:], before[..., 6:])                         # words 6, 7 untouched
    assert np.isfinite(rec).all()
    env = np.broadcast_to(src != 2, (T, N, A))
    M = np.float32(IM.SQUASH_BOUND)
    # the forward squash of the targets gives the clamped action back, within the bound tests/test_hip_mlp.py holds the forward squash to
    assert np.allclose(np.tanh(rec[..., 3].astype(np.float64))[env], np.clip(mean, -M, M)[env], rtol=0, atol=1e-6)
    assert np.allclose((1.0 / (1.0 + np.exp(-rec[..., 4].astype(np.float64))))[env], np.clip(sigma, 1 - M, M)[env], rtol=0, atol=1e-6)
    assert np.array_equal(rec[:, 1, 2, 3:5], a_cont[:, 1, 2])                    # a policy sample is copied
    assert (rec[:, :, 0, 5] == 0).all() and np.array_equal(rec[0, :, 1:, 5], w[:, 1:])
    assert stats[0] == w[:, 1:].astype(np.float64).sum() * T and stats[1] == T * N * (A - 1)
    # the edge values alone: a pass, size_mean = +-1, size_sigma in {0, 1}
    e = np.zeros((1, 1, 4), np.int32)
    rec2, _ = IM.records_spec(e, e, e, np.float32([[[0.0, 1.0, -1.0, 0.0]]]), np.float32([[[0.0, 1.0, 0.0, 1.0]]]), None, np.ones((1, 4), np.int32))
    assert np.isfinite(rec2).all() and rec2[0, 0, 0, 3] == 0.0 and rec2[0, 0, 1, 3] == -rec2[0, 0, 2, 3] and rec2[0, 0, 0, 4] == -rec2[0, 0, 1, 4]
    with pytest.raises(ValueError):
        IM.records_spec(cat, price, off, mean, sigma, None, src, w)              # a policy-sample slot without a_cont


def _loss_case(R, A, seed, stride=32):
    g = np.random.default_rng(seed)
    out = np.zeros((R, stride), np.float32)
    out[:, :25] = g.normal(size=(R, 25)).astype(np.float32) * 1.5
    rec = np.zeros((R, A, 8), np.float32)
    words = rec.view(np.int32)
    words[..., 0], words[..., 1], words[..., 2] = g.integers(0, 9, (R, A)), g.integers(0, 10, (R, A)), g.integers(0, 3, (R, A))
    rec[..., 3:5] = g.normal(size=(R, A, 2))
    rec[..., 5] = g.choice([0.0, 0.5, 1.0, 2.0], (R, A))
    rec[..., 6:8] = g.normal(size=(R, A, 2))
    rec[::3, :, 5] = 0.0                                                        # whole rows that do not count
    return out, np.float32([-0.5, 0.3]), rec


def _torch_loss(out, log_std, rec, vf_coef, ent_coef, loss_scale):
    """the same loss with torch.distributions in float64: (L, outputs leaf, log_std leaf)"""
    D = torch.distributions
    o = torch.tensor(out, dtype=torch.float64, requires_grad=True)
    ls = torch.tensor(log_std, dtype=torch.float64, requires_grad=True)
    lab = torch.tensor(np.ascontiguousarray(rec).view(np.int32)[..., :3].astype(np.int64))
    r = torch.tensor(rec, dtype=torch.float64)
    cats = [D.Categorical(logits=o[:, None, 0:9]), D.Categorical(logits=o[:, None, 9:19]), D.Categorical(logits=o[:, None, 19:22])]
    normal = D.Normal(o[:, None, 22:24], ls.exp())
    logp = sum(c.log_prob(lab[..., q]) for q, c in enumerate(cats)) + normal.log_prob(r[..., 3:5]).sum(-1)
    H = sum(c.entropy() for c in cats) + normal.entropy().sum(-1)
    w = r[..., 5]
    R, A = w.shape
    L = loss_scale / (R * A) * (w * (-logp + vf_coef * (o[:, None, 24] - r[..., 7]) ** 2 - ent_coef * H)).sum()
    return L, o, ls, logp


@pytest.mark.parametrize("A,vf_coef,ent_coef", [(1, 0.0, 0.0), (4, 0.5, 0.01), (16, 0.5, 0.0)])
def test_bc_loss_spec_equals_float64_autograd_of_the_same_loss(A, vf_coef, ent_coef):
    from gym_continuousdoubleauction_amd import imitate as IM
    out, log_std, rec = _loss_case(40, A, 3 + A)
    scale = 1.75
    d, sums5, logp, stats = IM.bc_loss_spec(out, log_std, rec, vf_coef=vf_coef, ent_coef=ent_coef, loss_scale=scale)
    L, o, ls, logp_t = _torch_loss(out, log_std, rec, vf_coef, ent_coef, scale)
    L.backward()
    assert np.allclose(d, o.grad.numpy(), rtol=1e-10, atol=1e-15)
    assert np.allclose(sums5[3:], ls.grad.numpy(), rtol=1e-10, atol=1e-15)
    assert np.allclose(logp, logp_t.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert (d[:, 25:] == 0).all()
    o6 = IM.out6_spec(sums5, 40 * A, vf_coef, ent_coef)
    assert np.isclose(o6[3], float(L.detach()), rtol=1e-10)
    # zero-weight samples contribute nothing: other labels, targets and returns there change no output but their own log-probability
    rec2 = rec.copy()
    dead = rec[..., 5] == 0
    rec2.view(np.int32)[..., 0][dead] = 8 - rec.view(np.int32)[..., 0][dead]
    rec2[..., 3][dead] += 3.0
    rec2[..., 7][dead] -= 2.0
    d2, s2, logp2, st2 = IM.bc_loss_spec(out, log_std, rec2, vf_coef=vf_coef, ent_coef=ent_coef, loss_scale=scale)
    assert np.array_equal(d2, d) and np.array_equal(s2, sums5) and np.array_equal(st2, stats) and np.array_equal(logp2[~dead], logp[~dead])
    assert (d[::3] == 0).all()                                                  # rows whose every sample has weight 0
    # loss_scale scales linearly (3 = a power of two short of exact: round-off only)
    d3, s3, _, st3 = IM.bc_loss_spec(out, log_std, rec, vf_coef=vf_coef, ent_coef=ent_coef, loss_scale=2.0 * scale)
    assert np.allclose(d3, 2.0 * d, rtol=1e-14, atol=0) and np.allclose(s3, 2.0 * sums5, rtol=1e-14, atol=0) and np.array_equal(st3, stats)
    # norm_rows and row_index: a gather from a larger record array, normalised over more rows
    big = np.concatenate([rec[::-1], rec])
    d4, s4, logp4, _ = IM.bc_loss_spec(out, log_std, big, row_index=np.arange(40) + 40, vf_coef=vf_coef, ent_coef=ent_coef, loss_scale=scale, norm_rows=80)
    assert np.allclose(d4, d / 2, rtol=1e-14, atol=0) and np.allclose(s4[:3], sums5[:3], rtol=1e-14) and np.array_equal(logp4, logp)


def test_bc_loss_spec_clamps_labels_as_pick_does_and_counts_agreement():
    from gym_continuousdoubleauction_amd import imitate as IM
    out, log_std, rec = _loss_case(8, 2, 11)
    rec[..., 5] = 1.0
    hi, lo = rec.copy(), rec.copy()
    hi.view(np.int32)[..., 0], hi.view(np.int32)[..., 1], hi.view(np.int32)[..., 2] = 8, 9, 2
    lo.view(np.int32)[..., :3] = 0
    far, neg = hi.copy(), lo.copy()
    far.view(np.int32)[..., :3] = 1000
    neg.view(np.int32)[..., :3] = -5
    for a, b in ((hi, far), (lo, neg)):
        ra, rb = IM.bc_loss_spec(out, log_std, a, ent_coef=0.01), IM.bc_loss_spec(out, log_std, b, ent_coef=0.01)
        assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
    best = rec.copy()
    best.view(np.int32)[..., 0] = out[:, None, 0:9].argmax(-1)
    best.view(np.int32)[..., 1] = out[:, None, 9:19].argmax(-1)
    best.view(np.int32)[..., 2] = out[:, None, 19:22].argmax(-1)
    best[..., 3:5] = out[:, None, 22:24]
    st = IM.bc_loss_spec(out, log_std, best)[3]
    assert st.tolist() == [16.0, 16.0, 16.0, 16.0, 0.0, 0.0, 16.0, 0.0]


def test_the_command_lines_parse():
    from gym_continuousdoubleauction_amd import imitate as IM, ppo
    a = IM.main(["--expert", "maker", "--expert", "taker:max_position=100", "--markets", "64", "--agents", "4", "--iters", "2", "--horizon", "8", "--save", "p.pt",
                 "--demos-out", "d.npz"], parse_only=True)
    assert a.expert == ["maker", "taker:max_position=100"] and (a.markets, a.agents, a.iters, a.horizon, a.save, a.demos_out, a.demos) == (64, 4, 2, 8, "p.pt", "d.npz", None)
    b = IM.main(["--demos", "d.npz", "--save", "p.pt"], parse_only=True)
    assert b.demos == "d.npz" and b.expert is None
    with pytest.raises(SystemExit):
        IM.main([], parse_only=True)                                            # nothing to clone
    with pytest.raises(SystemExit):
        IM.main(["--demos", "d.npz", "--expert", "maker"], parse_only=True)
    assert ppo.main(["--init-policy", "p.pt"], parse_only=True).init_policy == "p.pt"
    assert ppo.main([], parse_only=True).init_policy is None
