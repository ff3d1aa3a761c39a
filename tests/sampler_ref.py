"""The action sampler of the fused policy kernels, restated on the host in numpy (no GPU, no project library).

Written from the documented law - include/cda_mlp.h "Randomness" / "Sampling law", the comments above sample_action in csrc/cda_mlp_dev.inc - not from
the kernels' arithmetic: integers in uint64, everything else in float64, except where the law itself names a float32 value (the uniforms).

The law, for sample i = market * agents + agent of one launch:

    key        = mix64(seed + counter * 0xd1342543de82ef95 + draw * 0x2545f4914f6cdd1d)          (mod 2^64; cda_policy_sample: no draw term)
    w0, w1, w2 = mix64(key + i), mix64(w0), mix64(w1)
    k          = the top 24 bits of a 32-bit half-word:  category <- w0 low, price <- w0 high, price_offset <- w1 low,
                 Box-Muller radius <- w1 high, Box-Muller angle <- w2 low
    u          = (k + 1/2) / 2^24                                                               (intended: u_exact)
                 as float32 arithmetic (u_f32): exact for k < 2^23; above, k + 1/2 is not representable and rounds to even - u takes the even 24-bit
                 values, and the top value k = 2^24 - 1 gives 1.0, which the kernels clamp to 1 - 2^-24 (u_device)
    head       = the first class j with u * sum_q e_q < sum_{q <= j} e_q,  e_q = exp(l_q - max l)    (inverse CDF)
    n0, n1     = sqrt(-2 ln u_radius) * (cos, sin)(2 pi u_angle);  x = mu + exp(log_std) * n;  size_mean = tanh(x0), size_sigma = sigmoid(x1)
    logp       = sum over the three heads of log softmax(l)[class]  +  sum over the two Gaussians of -n^2 / 2 - log_std - log(2 pi) / 2
"""
import math

import numpy as np

M64 = (1 << 64) - 1
K_COUNTER = 0xd1342543de82ef95
K_DRAW = 0x2545f4914f6cdd1d
K_RANDOM = 0x9e3779b97f4a7c15                   # the league's random module: its stream's seed is random_seed + counter * K_RANDOM
N_CAT, N_PRICE, N_OFF = 9, 10, 3
HEADS = (("category", 0, N_CAT), ("price", N_CAT, N_CAT + N_PRICE), ("price_offset", N_CAT + N_PRICE, N_CAT + N_PRICE + N_OFF))
#: the five uniforms of a sample: name -> (word, half)
UNIFORMS = {"category": (0, 0), "price": (0, 1), "price_offset": (1, 0), "radius": (1, 1), "angle": (2, 0)}
TOP = (1 << 24) - 1
U_MAX = 1.0 - 2.0 ** -24                         # the largest float32 below 1: what the kernels return for k = TOP


def mix64(z):
    """splitmix64's finaliser (Steele, Lea, Flood 2014) on uint64 arrays, or on one Python int"""
    if isinstance(z, int):
        z = (z + 0x9e3779b97f4a7c15) & M64
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
        return z ^ (z >> 31)
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return z ^ (z >> np.uint64(31))


def rollout_key(seed, counter, draw=0):
    """the key of one launch (Python ints, exact mod 2^64).  cda_policy_sample's key is this with draw = 0."""
    return mix64((int(seed) + int(counter) * K_COUNTER + int(draw) * K_DRAW) & M64)


def words(key, i):
    """(w0, w1, w2) of the samples i (an integer array of global sample indices)"""
    with np.errstate(over="ignore"):
        w0 = mix64(np.uint64(int(key)) + np.asarray(i).astype(np.uint64))
    w1 = mix64(w0)
    return w0, w1, mix64(w1)


def draws24(key, i):
    """the five 24-bit integers of every sample: {name: int64 array}"""
    w = words(key, i)
    out = {}
    for name, (word, half) in UNIFORMS.items():
        x = (w[word] >> np.uint64(32)) if half else (w[word] & np.uint64(0xffffffff))
        out[name] = (x >> np.uint64(8)).astype(np.int64)
    return out


def u_exact(k):
    """the intended uniform, float64: (k + 1/2) / 2^24, strictly inside (0, 1)"""
    return (np.asarray(k, dtype=np.float64) + 0.5) / 16777216.0


def u_f32(k):
    """the float32 expression as the kernels write it, unclamped: ((float) k + 0.5f) * 2^-24"""
    return (np.asarray(k).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def u_device(k):
    """the uniform the kernels use: u_f32 clamped to the largest float32 below 1 (float32 array)"""
    return np.minimum(u_f32(k), np.float32(U_MAX))


class Head:
    """one categorical head: the float64 CDF of float32 logits [..., n] (one row of logits, or one per sample)"""

    def __init__(self, logits):
        l = np.asarray(logits, dtype=np.float32).astype(np.float64)
        self.n = l.shape[-1]
        e = np.exp(l - l.max(-1, keepdims=True))
        cum = np.cumsum(e, -1)
        self.logp = (l - l.max(-1, keepdims=True)) - np.log(cum[..., -1:])
        self.bounds = cum[..., :-1] / cum[..., -1:]                # the n - 1 interior boundaries of the inverse CDF, ascending

    def interval(self, u):
        """the class of u: the first j with u < bounds[j] (n - 1 if none)"""
        u = np.asarray(u, dtype=np.float64)
        return (u[..., None] >= self.bounds).sum(-1).astype(np.int64)

    def distance_to_boundary(self, u):
        u = np.asarray(u, dtype=np.float64)
        return np.abs(u[..., None] - self.bounds).min(-1)

    def neighbours(self, u, eps):
        """(lo, hi) = the classes of u - eps and u + eps: equal where the sample is decided; where it is not, the two classes next to the boundary - and whatever
        lies between them when a class is narrower than the band (a probability below 2 eps: hi - lo > 1)"""
        u = np.asarray(u, dtype=np.float64)
        return self.interval(u - eps), self.interval(u + eps)

    def log_prob(self, a):
        a = np.asarray(a, dtype=np.int64)
        lp = np.broadcast_to(self.logp, a.shape + (self.n,))
        return np.take_along_axis(lp, a[..., None], -1)[..., 0]

    def mode(self):
        """argmax, the lowest index on a tie"""
        return np.argmax(self.logp, -1).astype(np.int64)


def heads_of(outputs):
    """the three heads of network outputs [..., >= 24]"""
    o = np.asarray(outputs, dtype=np.float32)
    return {name: Head(o[..., lo:hi]) for name, lo, hi in HEADS}


def box_muller(k_radius, k_angle):
    """(n0, n1) in float64 from the kernels' two uniforms"""
    ur, ua = u_device(k_radius).astype(np.float64), u_device(k_angle).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(ur))
    return r * np.cos(2.0 * math.pi * ua), r * np.sin(2.0 * math.pi * ua)


def sample(key, i, outputs, log_std):
    """The whole law for the samples i.  outputs: float32 [..., >= 24] network outputs, one row or one row per sample; log_std: [..., 2] the log-stds each
    sample is drawn with (the free vector, plus output columns 25, 26 with the state-dependent head).  Returns a dict of float64 / int64 arrays:
    category, price, price_offset (the class of u_exact), dist_<head> (distance of u_exact to the nearest boundary), n [.., 2], a_cont [.., 2], size_mean,
    size_sigma, logp, k (the 24-bit draws)."""
    i = np.asarray(i)
    o = np.asarray(outputs, dtype=np.float32)
    k = draws24(key, i)
    hs = heads_of(o)
    out = {"k": k, "heads": hs}
    logp = np.zeros(i.shape)
    for name in ("category", "price", "price_offset"):
        u = u_exact(k[name])
        a = hs[name].interval(u)
        out[name], out["dist_" + name] = a, hs[name].distance_to_boundary(u)
        logp = logp + hs[name].log_prob(a)
    n0, n1 = box_muller(k["radius"], k["angle"])
    n = np.stack([n0, n1], -1)
    ls = np.broadcast_to(np.asarray(log_std, dtype=np.float32).astype(np.float64), n.shape)
    mu = np.broadcast_to(o[..., 22:24].astype(np.float64), n.shape)
    x = mu + np.exp(ls) * n
    out.update(n=n, a_cont=x, size_mean=np.tanh(x[..., 0]), size_sigma=1.0 / (1.0 + np.exp(-x[..., 1])),
               logp=logp + (-0.5 * n * n - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1))
    return out


def logp_of(outputs, log_std, cat, price, off, a_cont):
    """float64 log-probability of given actions under the distribution of `outputs` / `log_std`"""
    o = np.asarray(outputs, dtype=np.float32)
    hs = heads_of(o)
    lp = hs["category"].log_prob(cat) + hs["price"].log_prob(price) + hs["price_offset"].log_prob(off)
    x = np.asarray(a_cont, dtype=np.float64)
    ls = np.broadcast_to(np.asarray(log_std, dtype=np.float32).astype(np.float64), x.shape)
    z = (x - np.broadcast_to(o[..., 22:24].astype(np.float64), x.shape)) * np.exp(-ls)
    return lp + (-0.5 * z * z - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1)


def mode(outputs, log_std):
    """the deterministic action: argmax of each head (lowest index on ties), the Gaussian means; logp = the sampled formula with n = 0"""
    o = np.asarray(outputs, dtype=np.float32)
    hs = heads_of(o)
    out = {name: hs[name].mode() for name in hs}
    ls = np.broadcast_to(np.asarray(log_std, dtype=np.float32).astype(np.float64), o.shape[:-1] + (2,))
    x = o[..., 22:24].astype(np.float64)
    out.update(a_cont=x, size_mean=np.tanh(x[..., 0]), size_sigma=1.0 / (1.0 + np.exp(-x[..., 1])),
               logp=sum(hs[name].log_prob(out[name]) for name in hs) + (-ls - 0.5 * math.log(2.0 * math.pi)).sum(-1))
    return out


def random_module(seed, market, step, agent):
    """include/cda_random_agents.h cda_random_action: the uniform random module's action of (seed, global market, step, agent); arrays broadcast.
    Returns (category, size_mean f32, size_sigma f32, price, price_offset)."""
    m, a = np.asarray(market).astype(np.uint64), np.asarray(agent).astype(np.uint64)
    with np.errstate(over="ignore"):
        h0 = mix64(np.uint64(int(seed) & M64) + m * np.uint64(K_COUNTER))
        w0 = mix64(h0 + ((np.uint64(int(step)) << np.uint64(32)) | a))
    w1 = mix64(w0)
    lo = np.uint64(0xffffffff)
    cat = (((w0 & lo) * np.uint64(9)) >> np.uint64(32)).astype(np.int32)
    price = (((w0 >> np.uint64(32)) * np.uint64(10)) >> np.uint64(32)).astype(np.int32)
    off = (((w1 & lo) * np.uint64(3)) >> np.uint64(32)).astype(np.int32)
    mean = ((w1 >> np.uint64(32)) & np.uint64(0xffffff)).astype(np.float32) * np.float32(1.0 / 8388608.0) - np.float32(1.0)
    sigma = (w1 >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return cat, mean, sigma, price, off


def find_top_draw(name, n_samples, counter=0, draw=0, seeds=range(3000)):
    """the first (seed, i) with i < n_samples whose 24-bit draw `name` is the top value 2^24 - 1 (the float32 uniform's u == 1 edge); None if there is none"""
    i = np.arange(n_samples, dtype=np.int64)
    for seed in seeds:
        hit = np.nonzero(draws24(rollout_key(seed, counter, draw), i)[name] == TOP)[0]
        if hit.size:
            return int(seed), int(hit[0])
    return None


# ---- the law tests' statistics (tests/test_sampler_ref_host.py proves every threshold on this file's own samples; tests/test_hip_sampler.py applies them to the
# device's) -------------------------------------------------------------------------------------------------------------------------------------------------
P_MIN = 1e-6                                      # every chi-square below must give p > P_MIN
LAW_N = 1 << 22                                   # samples per constructed distribution (4 M)
#: constructed logits of the law tests: name -> the 22 categorical logits (float32); NEVER lists the classes whose logit is -100 (probability 0 in float32)
DEAD = -100.0


def law_distributions():
    d = {}
    d["uniform"] = np.zeros(22, np.float32)
    d["linspace"] = np.concatenate([np.linspace(-4, 4, n) for n in (N_CAT, N_PRICE, N_OFF)]).astype(np.float32)
    rare = np.zeros(22, np.float32)
    rare[[4, N_CAT + 7, N_CAT + N_PRICE + 1]] = np.float32(math.log(1e-6))     # one class per head at (about) 1e-6
    d["rare"] = rare
    for pos, idx in (("first", (0, 0, 0)), ("middle", (4, 5, 1)), ("last", (N_CAT - 1, N_PRICE - 1, N_OFF - 1))):
        l = np.linspace(-1, 1, 22).astype(np.float32)
        l[[idx[0], N_CAT + idx[1], N_CAT + N_PRICE + idx[2]]] = DEAD
        d["dead_" + pos] = l
    return d


def dead_classes(logits22):
    """per head, the classes that must never be drawn"""
    return {name: np.nonzero(np.asarray(logits22)[lo:hi] <= DEAD)[0] for name, lo, hi in HEADS}


def chi2_p(counts, probs):
    """chi-square goodness of fit over the classes of non-zero probability (p-value); classes of probability zero must have count zero (asserted by the caller)"""
    from scipy import stats
    counts, probs = np.asarray(counts, dtype=np.float64).ravel(), np.asarray(probs, dtype=np.float64).ravel()
    live = probs > 0
    exp = probs[live] / probs[live].sum() * counts[live].sum()
    return float(stats.chisquare(counts[live], exp).pvalue)


def head_probs(logits22):
    """float64 softmax of each head, classes at DEAD set to exactly 0 (float32 exp(-100 - max) is below the smallest normal: flushed)"""
    out = {}
    for name, lo, hi in HEADS:
        l = np.asarray(logits22, dtype=np.float32)[lo:hi].astype(np.float64)
        e = np.where(l <= DEAD, 0.0, np.exp(l - l.max()))
        out[name] = e / e.sum()
    return out


def law_checks(logits22, cat, price, off, n0, n1):
    """every statistic of the law tests for one constructed distribution; returns {name: (value, passes)}.  cat / price / off integer arrays, n0 / n1 the
    standard normal draws, all of one length."""
    from scipy import stats
    res = {}
    n = cat.size
    pr = head_probs(logits22)
    acts = {"category": cat, "price": price, "price_offset": off}
    for name, lo, hi in HEADS:
        c = np.bincount(acts[name], minlength=hi - lo)
        dead = dead_classes(logits22)[name]
        res["never_" + name] = (int(c[dead].sum()), int(c[dead].sum()) == 0)
        p = chi2_p(c, pr[name])
        res["fit_" + name] = (p, p > P_MIN)
    # the joint table against the product law (category and price share one 64-bit word, offset shares one with the radius)
    joint = np.bincount((cat * N_PRICE + price) * N_OFF + off, minlength=N_CAT * N_PRICE * N_OFF).reshape(N_CAT, N_PRICE, N_OFF)
    prod = pr["category"][:, None, None] * pr["price"][None, :, None] * pr["price_offset"][None, None, :]
    big = prod * n >= 5.0                                     # chi-square's usual floor on the expected count; the rest are pooled into one cell
    cnt = np.append(joint[big], joint[~big].sum()) if (~big & (prod > 0)).any() else joint[big]
    exp = np.append(prod[big], prod[~big].sum()) if (~big & (prod > 0)).any() else prod[big]
    p = chi2_p(cnt, exp)
    res["joint"] = (p, p > P_MIN)
    live_off = np.nonzero(pr["price_offset"] > 0)[0]
    for label, cls in (("off_x_sign_n0", (n0 > 0).astype(np.int64)), ("off_x_tercile_abs_n0", np.digitize(np.abs(n0), stats.halfnorm.ppf([1 / 3, 2 / 3])))):
        k = int(cls.max()) + 1
        tab = np.bincount(off * k + cls, minlength=N_OFF * k).reshape(N_OFF, k)[live_off]
        p = float(stats.chi2_contingency(tab)[1]) if live_off.size > 1 else 1.0
        res[label] = (p, p > P_MIN)
    edges = stats.norm.ppf(np.arange(1, 64) / 64.0)
    for label, x in (("n0", n0), ("n1", n1)):
        c = np.bincount(np.digitize(x, edges), minlength=64)
        p = float(stats.chisquare(c).pvalue)
        res["bins_" + label] = (p, p > P_MIN)
        for s in (3.0, 4.0):
            q = 2.0 * stats.norm.sf(s)
            got = int((np.abs(x) > s).sum())
            p = float(stats.binomtest(got, n, q).pvalue)
            res[f"tail{int(s)}_{label}"] = (p, p > P_MIN)
    lim = 5.0 / math.sqrt(n)
    for label, a, b in (("corr_n", n0, n1), ("corr_n2", n0 * n0, n1 * n1)):
        r = float(np.corrcoef(a, b)[0, 1])
        res[label] = (r, abs(r) < lim)
    return res


def serial_p(cat_a, cat_b):
    """independence of two category streams: the 9 x 9 contingency table's p-value"""
    from scipy import stats
    tab = np.bincount(np.asarray(cat_a) * N_CAT + np.asarray(cat_b), minlength=N_CAT * N_CAT).reshape(N_CAT, N_CAT)
    tab = tab[tab.sum(1) > 0][:, tab.sum(0) > 0]
    return float(stats.chi2_contingency(tab)[1])


# ---- the constants the host test proves and the device test applies --------------------------------------------------------------------------------------
EPS = 1e-5                                        # u-space band around a CDF boundary inside which a float32 sampler may take either neighbouring class
UNDECIDED_CAP = 2e-3                              # largest share of a case's samples that may lie inside the band (expected from the law: 2 EPS x 19 boundaries ~ 4e-4)
LAW_SEED, LAW_COUNTER, LAW_DRAW = 20240229, 3, 11  # the key of the law tests
LAW_MARKETS, LAW_AGENTS = 1 << 18, 16             # 262144 x 16 = LAW_N samples in one launch
assert LAW_MARKETS * LAW_AGENTS == LAW_N


def sample_head_f32(logits, u):
    """the inverse-CDF head in float32 arithmetic with sequential sums (numpy's exp, not the GPU's): the restatement's float32 twin.  logits [n] or [m, n], u float32 [m]"""
    l = np.broadcast_to(np.asarray(logits, dtype=np.float32), (u.shape[0], np.asarray(logits).shape[-1]))
    e = np.exp(l - l.max(-1, keepdims=True)).astype(np.float32)
    e = np.where(e < np.float32(2.0 ** -126), np.float32(0), e)      # (below the smallest normal: flushed)
    c = np.zeros((u.shape[0], l.shape[1]), np.float32)
    s = np.zeros(u.shape[0], np.float32)
    for j in range(l.shape[1]):
        s = (s + e[:, j]).astype(np.float32)
        c[:, j] = s
    t = (np.asarray(u, dtype=np.float32) * s).astype(np.float32)
    below = t[:, None] < c
    return np.where(below.any(-1), below.argmax(-1), l.shape[1] - 1).astype(np.int64)
