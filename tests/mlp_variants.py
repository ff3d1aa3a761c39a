"""The network kernels' instance table: csrc/cda_mlp.hip is compiled once per (history depth, hidden activation, separate / shared trunk) - mlp.HIST_VARIANTS x
mlp.ACTIVATIONS x vf_share_layers, 56 objects, each exporting its own copy of include/cda_mlp.h's entry points under <name>[_h<H>][_<act>][_vfs] - and the helpers
the per-variant tests share (tests/test_mlp_variants_host.py: the table, the symbols, the layout constants; tests/test_hip_mlp_variants.py: every object against
the float64 statement of its network; tests/test_hip_activation.py, test_hip_vf_share.py and test_hip_sampler.py import their helpers from here).

Importing this module needs no GPU: the table is derived from mlp.py, the helpers touch the device when they are called."""
import numpy as np
import pytest
import torch

from gym_continuousdoubleauction_amd import mlp

DEV = "cuda:0"
H = mlp.HID

#: every compiled object as (n_hist, activation, vf_share_layers): derived, so that a new depth or activation is walked without anyone remembering this file
VARIANTS = [(h, act, vfs) for h in mlp.HIST_VARIANTS for act in mlp.ACTIVATIONS for vfs in (False, True)]


def variant_id(v):
    h, act, vfs = v
    return f"h{h}-{act}" + ("-vfs" if vfs else "")


IDS = [variant_id(v) for v in VARIANTS]
PARAMS = [pytest.param(*v, id=variant_id(v)) for v in VARIANTS]

#: rows of the training-path checks (whole 32-row tiles: the update's row images) and of forward / policy_step (no multiple of the forward's 128-row tile)
N_TRAIN, N_FWD = 160, 200


def object_name(h, act, vfs):
    """the object file __graft_entry__.build_hip compiles for a variant, and (behind "cda_mlp") the suffix of its entry points"""
    return "cda_mlp" + ("" if h == 4 else f"_h{h}") + ("" if act == "tanh" else f"_{act}") + ("_vfs" if vfs else "")


def head_on(h, act, vfs):
    """the state-dependent log-std head is on for every other variant, so that both head settings meet every value of every axis"""
    return (h + mlp.ACTIVATIONS.index(act) + int(vfs)) % 2 == 0


def seed_of(h):
    return 3 + h


# ---- parameters, observations ------------------------------------------------------------------------------------------------------------------------------------
def theta(n_hist=4, vfs=False, seed=3, scale=1.0, sd=False, hidden=(256, 256)):
    th = mlp.init_theta(42 * n_hist, generator=torch.Generator().manual_seed(seed), state_dependent_log_std=sd, hidden=hidden, vf_share_layers=vfs)
    th[:mlp.layout(n_hist).OFF_LS] *= scale
    return th


def policy(n_hist=4, act="tanh", vfs=False, seed=3, scale=1.0, sd=False, hidden=(256, 256)):
    return mlp.FusedPolicy(DEV, theta=theta(n_hist, vfs, seed, scale, sd, hidden), state_dependent_log_std=sd, activation=act, vf_share_layers=vfs)


def obs(n, n_hist=4, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 42 * n_hist, generator=g) * 1.5
    x[:, ::7] = 0.0                                     # observations hold exact zeros (empty book levels)
    return x


def d_out_of(n, seed=4):
    """the output gradient of the backward checks: 25 live columns at 1e-3"""
    d = torch.zeros(n, 32)
    d[:, :25] = torch.randn(n, 25, generator=torch.Generator().manual_seed(seed)) * 1e-3
    return d


def perturb_value_half(p, seed=99):
    """non-zero entries in theta's value half (behind the policy object's back), re-packed: a shared-trunk kernel must not read them"""
    g = torch.Generator().manual_seed(seed)
    th = p.theta.cpu()
    for a, b in mlp.value_half(p.L):
        th[a:b] = torch.randn(b - a, generator=g) * 0.3
    p.theta.copy_(th.to(DEV))
    p.pack()


# ---- the separate update kernels, launched one by one ------------------------------------------------------------------------------------------------------------
def train_forward(p, x, fill=0.0):
    """prep_rows + forward_train of this policy's variant: the packed images of the observation rows and of h1 / h2, the outputs.  fill: what x_rm / x_pk hold
    before prep_rows writes them"""
    from gym_continuousdoubleauction_amd._lib import check
    L = p.L
    n = x.shape[0]
    bf = torch.bfloat16
    tile = int(L.fn("cda_mlp_tile_rows")())
    pad = (n + tile - 1) // tile * tile
    ws = {"x_rm": torch.full((n * L.KX,), fill, dtype=bf, device=DEV), "x_pk": torch.full((n * 32 * L.XT,), fill, dtype=bf, device=DEV),
          "h1p": torch.zeros(pad * 512, dtype=bf, device=DEV), "h2p": torch.zeros(pad * 512, dtype=bf, device=DEV),
          "out": torch.zeros((pad, 32), dtype=torch.float32, device=DEV), "pad": pad, "tiles": pad // tile}
    xd = x.to(DEV).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    check(L.fn("cda_mlp_prep_rows")(xd.data_ptr(), None, n, ws["x_rm"].data_ptr(), ws["x_pk"].data_ptr(), st), "prep")
    check(L.fn("cda_mlp_forward_train")(p.wb.data_ptr(), p.theta.data_ptr(), ws["x_rm"].data_ptr(), n, ws["h1p"].data_ptr(), ws["h2p"].data_ptr(), ws["out"].data_ptr(), st), "fwd")
    torch.cuda.synchronize()
    return ws


def images(ws, n):
    return (mlp.unpack_rows(ws["h1p"][:n * 512], n, 512, paired=True).double(), mlp.unpack_rows(ws["h2p"][:n * 512], n, 512, paired=True).double())


def trunk_tiles(packed, n):
    """the trunk's (half 0's) feature tiles of a packed hidden image [n / 32][16 tiles][1024 bf16]"""
    return packed[:n * 512].view(n // 32, 16, 1024)[:, :8]


def full_backward(p, x, d_out, chunks, fill=0.0):
    """train_forward, then backward, weight gradients and reduce + Adam (lr 0: the gradient alone).  The slabs start as NaN: an entry the weight-gradient or bias
    jobs do not write - the shared trunk skips the value half's - must not be read by the reduction"""
    from gym_continuousdoubleauction_amd._lib import check
    L = p.L
    n = x.shape[0]
    ws = train_forward(p, x, fill)
    bf = torch.bfloat16
    pad, tiles = ws["pad"], ws["tiles"]
    ws.update(dz1p=torch.zeros(pad * 512, dtype=bf, device=DEV), dz2p=torch.zeros(pad * 512, dtype=bf, device=DEV), doutp=torch.zeros(pad * 32, dtype=bf, device=DEV),
              bias_slab=torch.full((tiles * mlp.BSLAB,), float("nan"), dtype=torch.float32, device=DEV),
              slab=torch.full((chunks * L.SLAB,), float("nan"), dtype=torch.float32, device=DEV),
              grad=torch.zeros(L.PARAMS, dtype=torch.float32, device=DEV), norm2=torch.zeros(512, dtype=torch.float64, device=DEV))
    dd = d_out.to(DEV).float().contiguous()
    st = torch.cuda.current_stream().cuda_stream
    check(L.fn("cda_mlp_backward")(p.wb.data_ptr(), dd.data_ptr(), ws["h1p"].data_ptr(), ws["h2p"].data_ptr(), n, ws["dz1p"].data_ptr(), ws["dz2p"].data_ptr(),
                                   ws["doutp"].data_ptr(), ws["bias_slab"].data_ptr(), st), "bwd")
    check(L.fn("cda_mlp_wgrad")(ws["x_pk"].data_ptr(), ws["h1p"].data_ptr(), ws["h2p"].data_ptr(), ws["dz1p"].data_ptr(), ws["dz2p"].data_ptr(), ws["doutp"].data_ptr(), n, chunks,
                                ws["slab"].data_ptr(), st), "wgrad")
    check(L.fn("cda_mlp_adam")(p.theta.data_ptr(), p.adam_m.data_ptr(), p.adam_v.data_ptr(), p.adam_step.data_ptr(), p.wb.data_ptr(), ws["slab"].data_ptr(), chunks,
                               ws["bias_slab"].data_ptr(), tiles, None, 0, 0.0, 0.0, 0.0, None, 0.0, 0.9, 0.999, 1e-8, 0.5, ws["grad"].data_ptr(), ws["norm2"].data_ptr(), st), "adam")
    torch.cuda.synchronize()
    return ws


def blocks_of(L):
    return ((L.OFF_W1, L.OFF_B1, "W1"), (L.OFF_B1, L.OFF_W2, "b1"), (L.OFF_W2, L.OFF_B2, "W2"), (L.OFF_B2, L.OFF_WO, "b2"), (L.OFF_WO, L.OFF_BO, "Wo"), (L.OFF_BO, L.OFF_LS, "bo"))


# ---- the sampler against tests/sampler_ref.py --------------------------------------------------------------------------------------------------------------------
#: the largest |n_dev - n_ref| seen on an MI355X over every case of tests/test_hip_sampler.py, rounded up (that module's docstring)
MEASURED_GAUSS = 1.9e-6
GAUSS_BOUND = min(4 * MEASURED_GAUSS, 1e-4)
ACTION_KEYS = ("category", "price", "price_offset", "size_mean", "size_sigma", "a_cont", "logp")


def log_std_rows(p, out):
    """the log-stds every row is sampled with: the free vector + output columns 25, 26 (zero without the state-dependent head), float32 as the kernels add them"""
    return (p.theta[p.L.OFF_LS:].cpu().numpy()[None, :] + out[:, 25:27]).astype(np.float32)


def flat(o, rows=None):
    """a policy step's outputs as flat per-sample numpy arrays (rows: the markets to keep)"""
    d = {}
    for k in (kk for kk in ACTION_KEYS if kk in o):
        v = o[k].detach().cpu().numpy()
        v = v if rows is None else v[rows]
        d[k] = v.reshape(-1, 2) if k == "a_cont" else v.reshape(-1)
    return d


def compare(tag, dev, key, i, out_rows, ls_rows, mean_tol=1e-6, a_cont_rounding=False):
    """the device's samples `dev` (flat arrays) with global indices i against the restatement; out_rows [m, >= 24] / ls_rows [m, 2]: each sample's row of network
    outputs and log-stds (or one row for all).  Prints and returns (undecided share, largest Gaussian deviation, largest logp deviation).
    a_cont_rounding: the normal draw is read back from the stored float32 sample, n_dev = (a_cont - mu) exp(-log_std), and a_cont = fl(mu + fl(sigma n)) carries
    two float32 roundings of its own: at most 2^-24 (|sigma n| + |a_cont|), which in units of n is that times exp(-log_std).  Where sigma is of the order of |mu|
    (every network without the state-dependent head: sigma = e^-0.5) the term is below 1e-6 and inside GAUSS_BOUND; a head's offset can make sigma a thousand
    times smaller than |mu|, and then the read-back, not the sampler, loses the digits.  True: each sample's deviation is held to GAUSS_BOUND + its own term."""
    import sampler_ref as R
    ref = R.sample(key, i, out_rows, ls_rows)
    undecided = np.zeros(i.shape, bool)
    for head, _, _ in R.HEADS:
        a = dev[head].astype(np.int64)
        u = R.u_exact(ref["k"][head])
        decided = ref["dist_" + head] > R.EPS
        wrong = np.nonzero(decided & (a != ref[head]))[0]
        assert wrong.size == 0, (tag, head, wrong.size, [(int(i[w]), int(a[w]), int(ref[head][w]), float(ref["dist_" + head][w])) for w in wrong[:5]])
        lo, hi = ref["heads"][head].neighbours(u, R.EPS)
        assert ((a >= lo) & (a <= hi)).all(), (tag, head)
        undecided |= ~decided
    share = float(undecided.mean())
    x = dev["a_cont"].astype(np.float64)
    ls = np.broadcast_to(np.asarray(ls_rows, np.float32).astype(np.float64), x.shape)
    mu = np.broadcast_to(np.asarray(out_rows, np.float32)[..., 22:24].astype(np.float64), x.shape)
    dn = np.abs((x - mu) * np.exp(-ls) - ref["n"])
    raw = float(dn.max())
    if a_cont_rounding:
        dn = dn - 2.0 ** -24 * (np.abs(x - mu) + np.abs(x)) * np.exp(-ls)
    gauss = float(dn.max())
    sq = max(float(np.abs(dev["size_mean"] - np.tanh(x[:, 0])).max()), float(np.abs(dev["size_sigma"] - 1.0 / (1.0 + np.exp(-x[:, 1]))).max()))
    lp = float(np.abs(R.logp_of(out_rows, ls_rows, dev["category"], dev["price"], dev["price_offset"], x) - dev["logp"]).max())
    print(f"[sampler] {tag}: samples {i.size} undecided {share:.3e} gauss {gauss:.3e} squash {sq:.3e} logp {lp:.3e}" + (f" (gauss before the read-back term {raw:.3e})" if a_cont_rounding else ""))
    assert share <= R.UNDECIDED_CAP, (tag, share)
    assert gauss <= GAUSS_BOUND, (tag, gauss)
    assert sq <= mean_tol, (tag, sq)
    assert lp <= 2e-4, (tag, lp)
    return share, gauss, lp


# ---- mode actions (tests/test_hip_evaluate.py's relation) --------------------------------------------------------------------------------------------------------
ULP1 = float(np.spacing(np.float32(1.0)))          # 2^-23


def check_mode(o, out, log_std, head):
    """o: a greedy launch's dict for [n, A] samples; out: forward() rows of the same markets (f32 tensor).  argmax of each categorical head (torch: the lowest
    index on a tie), the means, and the mode's log-probability in float64"""
    import math
    A = o["category"].shape[1]
    o64 = out.double().cpu()
    heads = ((0, 9), (9, 19), (19, 22))
    idx = [torch.argmax(out[:, a:b].cpu(), dim=1) for a, b in heads]
    ls = log_std.double().cpu().view(1, 2) + (o64[:, 25:27] if head else 0.0)
    lp = sum(o64[:, a:b].gather(1, i.view(-1, 1)).view(-1) - torch.logsumexp(o64[:, a:b], dim=1) for (a, b), i in zip(heads, idx))
    lp = lp - ls[:, 0] - ls[:, 1] - math.log(2 * math.pi)
    for k, ref in zip(("category", "price", "price_offset"), idx):
        assert torch.equal(o[k].cpu().long(), ref.view(-1, 1).expand(-1, A)), k
    means = out[:, 22:24].cpu()
    assert torch.equal(o["a_cont"].cpu(), means.view(-1, 1, 2).expand(-1, A, 2))
    tol = 4 * ULP1           # (the device's 1 - 2 / (e^2x + 1) is accurate to a few ulp OF ONE, not of tanh near zero: an absolute bound)
    assert (o["size_mean"].cpu() - torch.tanh(means[:, :1])).abs().max() <= tol
    assert (o["size_sigma"].cpu() - torch.sigmoid(means[:, 1:])).abs().max() <= tol
    assert (o["logp"].cpu().double() - lp.view(-1, 1)).abs().max() <= 2e-4


def records(R, A, seed=6):
    """synthetic sample records [R, A, 8] (include/cda_learner.h CDA_REC_*): actions, old log-probability, advantage, return"""
    g = torch.Generator().manual_seed(seed)
    rec = torch.zeros(R, A, 8)
    rec[..., 0] = torch.randint(0, 9, (R, A), generator=g).int().view(torch.float32)
    rec[..., 1] = torch.randint(0, 10, (R, A), generator=g).int().view(torch.float32)
    rec[..., 2] = torch.randint(0, 3, (R, A), generator=g).int().view(torch.float32)
    rec[..., 3:5] = torch.randn(R, A, 2, generator=g)
    rec[..., 5] = torch.randn(R, A, generator=g) * 0.1 - 7.0
    rec[..., 6:8] = torch.randn(R, A, 2, generator=g)
    return rec
