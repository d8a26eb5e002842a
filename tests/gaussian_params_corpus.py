"""A fitted Gaussian network (include/dvs_gaussian_params.h; csrc/dvs_gaussian_params.h): the cases, the restatement of the
header's definitions in Python floats, the exact references and the checks that tests/test_emu_gaussian_params.py and
tests/test_gpu_gaussian_params.py run unchanged through the C ABI on their own back end (tests/scoring_corpus.py: EmuBackend,
GpuBackend); tests/test_gaussian_params_ref.py holds the restatement itself against the references on the CPU.

The generator's site 510 is restated here (site_key, draw) the way oracle/rng.py restates the sites before it.

References
  quantile     Phi^-1(u) = sqrt(2) erfinv(2 u - 1) from mpmath at 60 digits, u = (k + 1/2) 2^-52 exactly; the round trip through
               erfc is asserted at the ends of the domain.
  joint        exact rationals (the inputs are doubles, so Fraction arithmetic is exact) by the matrix form, not the header's
               recursion: A = (I - B)^-1 by forward substitution in topological order, mean = A c, cov = A diag(sd^2) A^T.
  loglik       mpmath on the header's formula, the constant as log(2 pi) / 2.
  prediction   mode 1 against conditioning the rational joint on all other variables with an mpmath LU solve at 60 digits:
               m_t + S_to S_oo^-1 (x_o - m_o) and S_tt - S_to S_oo^-1 S_ot.  Neither side shares a formula with the other, which
               pins dvs_gbn_joint and mode 1 against each other.

Tolerances.  None is fitted to a kernel's output; u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Lemma 3.1).
  quantile     QUANTILE_MEASURED is the largest relative error of the *restatement* against mpmath per branch over the grid
               (quantile_grid); QUANTILE_RTOL is that rounded up to two digits, which tests/test_gaussian_params_ref.py measures
               again and holds.  The central branch has no library call, so a build equals the restatement as bytes; a tail
               branch's log may differ between builds and is held to BUILD_FACTOR = 4 times the tolerance, the factor and the
               reason of tests/pc_corpus.py.
  joint        a sum of p rounded products is within gamma_p of sum |terms| (p products, p - 1 additions with the start at +0
               exact, or p additions after a rounded start).  With E the bound of an entry already computed:
                 off-diagonal  E[v][u] = sum_k |b_vk| E[k][u] + gamma_(p+1) sum_k |b_vk| (|S_ku| + E[k][u])
                 diagonal      E[v][v] = sum_k |b_vk| E[v][k] + gamma_(p+2) (sd_v^2 + sum_k |b_vk| (|S_vk| + E[v][k]))
                 mean          M[v]    = sum_k |b_vk| M[k]    + gamma_(p+1) (|c_v| + sum_k |b_vk| (|m_k| + M[k]))
               evaluated in exact rationals from the exact S and m (joint_bounds).
  mu           dmu_v(x) = gamma_(p+1) (|c_v| + sum |b_vk x_k|): p products, p additions.
  loglik       e = (x - mu) / sd:  de = (dmu + u (|x - mu| + dmu)) / sd + u |e|_hat;  e^2: de (2 |e| + de) + u e^2;  c_v: the log
               within LOG_ULPS = 2 ulp (the allowance of tests/gaussian_corpus.py) and one addition; the two additions of a
               variable's term: u each on the running magnitude.  A row's bound is the sum over the variables (row_bound);
               out's adds the summation: 16 + ceil(chunks / 256) additions in the two trees and the chunk chain (out_bound).
  mode 1       prec is a sum of positive terms, each three roundings, so its relative error is below gamma_(children + 4); num's
               is the absolute sum of its terms' errors (r_c carries dmu_c and one subtraction, w two roundings, the product
               one) plus gamma_(children + 1) on sum |terms|; pred = num / prec and var = 1 / prec add one rounding each
               (predict_bound).  The reference's own error, an LU solve at 60 digits, is far below every bound here.
  sampler      a row whose draws all take the central branch equals the restatement as bytes.  Elsewhere
               |dx_v| <= sum |b_vk| |dx_k| + sd_v |dz_v| + 2 gamma_(p+2) (|c_v| + sum |b_vk x_k| + sd_v |z_v|), dz_v = BUILD_FACTOR *
               QUANTILE_RTOL[branch] |z_v| on a tail draw and 0 on a central one (sample_bounds).
  builds       the emulator and the device are also held to the restatement on every row and structure, not only to mpmath on a
               share of them: restated_loglik_rows_fast derives what two builds' logs may differ by; the predictions and the
               joint have no library call and are compared as bytes.
Measured here (the restatement on the CPU; DESIGN.md §31 repeats them): QUANTILE_MEASURED."""
import ctypes
import functools
import math
from fractions import Fraction
from types import SimpleNamespace

import mpmath as mp
import numpy as np

from tests import gaussian_corpus as gc

U64 = np.uint64
U = gc.U
NAN = gc.NAN
SENTINEL = gc.SENTINEL
SITE = 510
TWO52 = 1 << 52
LOG_ULPS = 2
BUILD_FACTOR = 4
HALF_LOG_2PI = 0.9189385332046727
BRANCHES = ("central", "tail", "far")
# the largest relative error of restated_quantile against mpmath per branch over quantile_grid(), as measured on the CPU;
# tests/test_gaussian_params_ref.py measures it again and holds it to QUANTILE_RTOL, the measurement rounded up to two digits
QUANTILE_MEASURED = {"central": 5.530e-16, "tail": 6.581e-16, "far": 3.102e-16}
QUANTILE_RTOL = {"central": 5.6e-16, "tail": 6.6e-16, "far": 3.2e-16}
N_VALUES = (1, 5, 17, 48)
SAMPLE_ROWS = (1, 255, 257, 600)
LOGLIK_B = (1, 3, 65)
LOGLIK_S = (1, 256, 257, 700)
PREDICT_N = (5, 17, 48)


def gamma(k):
    return k * U / (1 - k * U)


# ---------------------------------------------------------------------------------------------------------------------
# The generator (csrc/dvs_device.h: dvs_fmix32, dvs_site_key, dvs_draw) in Python ints
# ---------------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def fmix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def site_key(seed, site, g):
    seed_lo, seed_hi = seed & M32, (seed >> 32) & M32
    k = fmix32(seed_lo ^ (((site + 1) * 0x632BE5AB) & M32))
    return fmix32(k ^ seed_hi ^ (((g & M32) * 0x9E3779B1) & M32))


def draw(key, pair):
    return fmix32(key ^ ((pair * 0x9E3779B1) & M32))


def draw_k(seed, g, v):
    """the 52-bit integer variable v of global row g draws"""
    key = site_key(seed, SITE, g)
    return ((draw(key, 2 * v) >> 6) << 26) + (draw(key, 2 * v + 1) >> 6)


# ---------------------------------------------------------------------------------------------------------------------
# The restatement of include/dvs_gaussian_params.h in Python floats (every operation one rounding, in the header's order)
# ---------------------------------------------------------------------------------------------------------------------
PA = (3.3871328727963666080, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
      4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3)
PB = (1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
      3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3)
PC = (1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550, 3.64784832476320460504,
      1.27045825245236838258, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
PD = (1.0, 2.05319162663775882187, 1.67638483018380384940, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
      1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
PE = (6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580, 2.96560571828504891230e-1,
      2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
PF = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
      1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def horner(p, r):
    t = p[7]
    for i in range(6, -1, -1):
        t = t * r
        t = t + p[i]
    return t


def restated_quantile(k):
    """(z, branch index) of the header's transform at the integer k; (NaN, -1) at k >= 2^52"""
    k = int(k)
    if k >= TWO52:
        return NAN, -1
    u, uc = (float(k) + 0.5) * 2.0 ** -52, (float(TWO52 - 1 - k) + 0.5) * 2.0 ** -52
    q = u - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        return (q * horner(PA, r)) / horner(PB, r), 0
    p = u if u < uc else uc
    r = math.sqrt(-math.log(p))
    if r <= 5.0:
        r = r - 1.6
        z, branch = horner(PC, r) / horner(PD, r), 1
    else:
        r = r - 5.0
        z, branch = horner(PE, r) / horner(PF, r), 2
    return (-z if q < 0.0 else z), branch


class Net(SimpleNamespace):
    """one network: n, parents (Python ints [n]), coef float64 [n, n], intercept, sd float64 [n]"""

    def pa(self, v):
        return [u for u in gc.bits_of(self.parents[v] & ~(1 << v)) if u < self.n]


def net_status(net):
    """(status bits, topological order) by the header's three rules"""
    n, bits = net.n, 0
    for v in range(n):
        pm = net.parents[v] & ~(1 << v)
        if pm >> n:
            bits |= 16
        if not (math.isfinite(net.intercept[v]) and math.isfinite(net.sd[v]) and net.sd[v] > 0.0):
            bits |= 64
        if any(not math.isfinite(net.coef[v, u]) for u in net.pa(v)):
            bits |= 64
    placed, order = 0, []
    low = (1 << n) - 1
    for _ in range(n):
        pick = next((v for v in range(n) if not (placed >> v) & 1 and not (net.parents[v] & low & ~(1 << v) & ~placed)), None)
        if pick is None:
            return bits | 1, order
        order.append(pick)
        placed |= 1 << pick
    return bits, order


def restated_mu(net, v, x, skip=-1):
    mu = float(net.intercept[v])
    for u in net.pa(v):
        if u != skip:
            mu = mu + float(net.coef[v, u]) * float(x[u])
    return mu


def restated_joint(net):
    """(mean [n], cov [n, n]); NaNs for a malformed network"""
    n = net.n
    bits, order = net_status(net)
    mean, cov = np.full(n, NAN), np.full((n, n), NAN)
    if bits:
        return mean, cov
    for i, v in enumerate(order):
        mean[v] = restated_mu(net, v, mean)
        for u in order[:i]:
            s = 0.0
            for k in net.pa(v):
                s = s + float(net.coef[v, k]) * float(cov[k, u])
            cov[v, u] = cov[u, v] = s
        s = float(net.sd[v]) * float(net.sd[v])
        for k in net.pa(v):
            s = s + float(net.coef[v, k]) * float(cov[v, k])
        cov[v, v] = s
    return mean, cov


@functools.lru_cache(maxsize=None)
def _restated_sample_cached(key, n_rows, seed, row_offset):
    net = NETS[key]
    _, order = net_status(net)
    x, z, branch = np.zeros((n_rows, net.n)), np.zeros((n_rows, net.n)), np.zeros((n_rows, net.n), np.int8)
    for i in range(n_rows):
        g = (row_offset + i) & M32
        for v in order:
            z[i, v], branch[i, v] = restated_quantile(draw_k(seed, g, v))
            x[i, v] = restated_mu(net, v, x[i]) + float(net.sd[v]) * float(z[i, v])
    for a in (x, z, branch):
        a.setflags(write=False)
    return x, z, branch


def restated_sample(key, n_rows, seed, row_offset=0):
    """(x [n_rows, n], z, branch index of every draw) of the sound network NETS[key]"""
    return _restated_sample_cached(key, int(n_rows), int(seed), int(row_offset))


def restated_loglik_rows(net, x, log=math.log):
    """the row terms [S] of the header; NaNs for a malformed network"""
    if net_status(net)[0]:
        return np.full(len(x), NAN)
    c = [log(float(net.sd[v])) + HALF_LOG_2PI for v in range(net.n)]
    out = np.zeros(len(x))
    for i, row in enumerate(x):
        term = 0.0
        for v in range(net.n):
            e = (float(row[v]) - restated_mu(net, v, row)) / float(net.sd[v])
            term = term - (c[v] + 0.5 * (e * e))
        out[i] = term
    return out


def tree256(values):
    """the header's tree over 256 slots: for s = 128 .. 1, slot t < s adds slot t + s"""
    a = np.array(values, np.float64, copy=True)
    assert a.shape == (256,)
    s = 128
    while s:
        a[:s] = a[:s] + a[s:2 * s]
        s >>= 1
    return float(a[0])


def stated_sum(terms):
    """out of dvs_gbn_loglik from the row terms: a tree per 256-row chunk (absent rows +0), slot t of a second array adds the
    chunks t, t + 256, ... in ascending order, the tree again"""
    terms = np.asarray(terms, np.float64)
    chunks = -(-len(terms) // 256)
    padded = np.zeros(chunks * 256)
    padded[:len(terms)] = terms
    parts = [tree256(padded[c * 256:(c + 1) * 256]) for c in range(chunks)]
    second = np.zeros(256)
    for c, p in enumerate(parts):
        second[c % 256] = second[c % 256] + p
    return tree256(second)


def restated_predict(net, t, mode, x):
    """(pred [S], var) of the header"""
    if net_status(net)[0]:
        return np.full(len(x), NAN), NAN
    n = net.n
    s = float(net.sd[t]) * float(net.sd[t])
    children = [c for c in range(n) if c != t and t in net.pa(c)]
    pred, var = np.zeros(len(x)), s
    for i, row in enumerate(x):
        mu = restated_mu(net, t, row)
        if mode == 0:
            pred[i] = mu
            continue
        prec = 1.0 / s
        num = mu * prec
        for c in children:
            beta = float(net.coef[c, t])
            w = beta / (float(net.sd[c]) * float(net.sd[c]))
            r = float(row[c]) - restated_mu(net, c, row, skip=t)
            num = num + w * r
            prec = prec + beta * w
        pred[i], var = num / prec, 1.0 / prec
    return pred, var


def restated_mu_rows(net, v, x, skip=-1):
    """restated_mu for every row at once: numpy's elementwise float64 operations round as Python's do, one at a time"""
    mu = np.full(len(x), float(net.intercept[v]))
    for u in net.pa(v):
        if u != skip:
            mu = mu + float(net.coef[v, u]) * x[:, u]
    return mu


def restated_loglik_rows_fast(net, x):
    """(restated_loglik_rows over all rows at once, as bytes; the bound [S] of another build's rows against them).  Two builds
    differ in c_v alone: their logs lie within LOG_ULPS ulp of the truth each and the addition rounds once each, dc_v = 2
    LOG_ULPS 2 u |ln sd_v| + 2 u |c_v|; after that the two additions of a variable's term round on either side: 2 u on the
    piece and 2 u on the running magnitude."""
    x = np.asarray(x, np.float64)
    if net_status(net)[0]:
        return np.full(len(x), NAN), np.zeros(len(x))
    term, running, bound = np.zeros(len(x)), np.zeros(len(x)), np.zeros(len(x))
    for v in range(net.n):
        sd = float(net.sd[v])
        c = math.log(sd) + HALF_LOG_2PI
        e = (x[:, v] - restated_mu_rows(net, v, x)) / sd
        piece = c + 0.5 * (e * e)
        term = term - piece
        dc = 2 * LOG_ULPS * 2 * U * abs(math.log(sd)) + 2 * U * abs(c)
        running = running + np.abs(piece) + dc
        bound = bound + dc + 2 * U * (np.abs(piece) + dc) + 2 * U * running
    return term, bound * (1 + 1e-9)


def out_bound_between_builds(terms, bounds):
    """the bound of one build's out against stated_sum of another's row terms: the rows' bounds and both sides' summation"""
    chunks = -(-len(terms) // 256)
    return float(np.sum(bounds)) + 2 * gamma(16 + -(-chunks // 256)) * float(np.sum(np.abs(terms)) + np.sum(bounds))


def restated_predict_fast(net, t, mode, x):
    """restated_predict over all rows at once, as bytes: (pred [S], var)"""
    x = np.asarray(x, np.float64)
    if net_status(net)[0]:
        return np.full(len(x), NAN), NAN
    s = float(net.sd[t]) * float(net.sd[t])
    mu = restated_mu_rows(net, t, x)
    if mode == 0:
        return mu, s
    prec = 1.0 / s
    num = mu * prec
    for c in range(net.n):
        if c == t or t not in net.pa(c):
            continue
        beta = float(net.coef[c, t])
        w = beta / (float(net.sd[c]) * float(net.sd[c]))
        r = x[:, c] - restated_mu_rows(net, c, x, skip=t)
        num = num + w * r
        prec = prec + beta * w
    return num / prec, 1.0 / prec


# ---------------------------------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------------------------------
def random_net(n, seed, max_parents=3, full=None, strength=(0.3, 0.9)):
    """a DAG in a random order (so the topological order is not the index order), up to max_parents parents each; ``full``: that
    variable comes last in the order and has every other variable as a parent (small coefficients: 47 of them at n = 48)"""
    rng = np.random.default_rng(31000 + 101 * n + seed)
    order = [int(v) for v in rng.permutation(n)]
    if full is not None:
        order.remove(full)
        order.append(full)
    parents, coef = [0] * n, np.zeros((n, n))
    for k, v in enumerate(order):
        pa = order[:k] if v == full else [int(u) for u in rng.choice(order[:k], size=min(k, int(rng.integers(0, max_parents + 1))), replace=False)] if k else []
        for u in pa:
            parents[v] |= 1 << u
            coef[v, u] = float(rng.choice([-1.0, 1.0])) * (float(rng.uniform(0.02, 0.1)) if v == full else float(rng.uniform(*strength)))
    net = Net(n=n, parents=parents, coef=coef, intercept=rng.uniform(-2.0, 2.0, n), sd=rng.uniform(0.5, 2.0, n))
    if n > 2 and net_status(net)[1] == list(range(n)):       # the index order would hide a kernel that ignores the order
        return random_net(n, seed + 1000, max_parents, full, strength)
    return net


def _nets():
    nets = {("one", 1): random_net(1, 0)}
    for n in (5, 17, 48):
        nets[("dag", n)] = random_net(n, 1)
        nets[("full", n)] = random_net(n, 2, full=n // 2 - 1)         # a variable with n - 1 parents, not the last index
    # the prediction cases at n: targets with no children, no parents, many children
    for n in PREDICT_N:
        net = random_net(n, 3)
        hub = net_status(net)[1][0]                          # first in the order: no parents; give it many children
        rng = np.random.default_rng(31900 + n)
        for c in range(n):
            if c != hub and rng.random() < 0.6:
                net.parents[c] |= 1 << hub
                net.coef[c, hub] = float(rng.uniform(0.3, 0.9)) * float(rng.choice([-1.0, 1.0]))
        nets[("hub", n)] = net
    for i in range(65):
        nets[("batch", i)] = random_net(5, 100 + i)
    nets[("pair", 2)] = Net(n=2, parents=[0, 1], coef=np.array([[0.0, 0.0], [0.75, 0.0]]), intercept=np.array([0.5, -1.0]), sd=np.array([1.5, 0.7]))
    return nets


NETS = _nets()
# the generator of the closed loop: strong coefficients, a collider (0 -> 2 <- 1) and a chain behind it, so its equivalence
# class fixes every arc but none by index order alone
LOOP_NET = Net(n=5, parents=[0, 0, 0b00011, 0b00100, 0b01100],
               coef=np.array([[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0.9, -0.8, 0, 0, 0], [0, 0, 0.85, 0, 0], [0, 0, 0.7, 0.8, 0]], np.float64),
               intercept=np.array([1.0, -2.0, 0.5, 0.0, 3.0]), sd=np.array([1.0, 1.2, 0.8, 1.0, 0.9]))
NETS[("loop", 5)] = LOOP_NET
LOOP_ROWS, LOOP_SEED = 2000, 510


def sinks_and_sources(net):
    """(a target with no children, one with no parents, the one with the most children)"""
    n = net.n
    kids = [sum(1 for c in range(n) if c != t and t in net.pa(c)) for t in range(n)]
    none = next(t for t in range(n) if kids[t] == 0)
    root = next(t for t in range(n) if not net.pa(t) and kids[t])
    return none, root, int(np.argmax(kids))


def malformed(net, rule):
    """a copy of the sound network that breaks one rule alone: "cycle", "bit", "nan-coef", "inf-intercept", "sd0", "nan-sd" """
    m = Net(n=net.n, parents=list(net.parents), coef=net.coef.copy(), intercept=net.intercept.copy(), sd=net.sd.copy())
    n = m.n
    if rule == "cycle":
        order = net_status(net)[1]
        a, b = order[0], order[-1]
        m.parents[a] |= 1 << b
        m.parents[b] |= 1 << a
        m.coef[a, b] = m.coef[b, a] = 0.5
    elif rule == "bit":
        m.parents[0] |= 1 << n
    elif rule == "nan-coef":
        v = next(v for v in range(n) if m.pa(v))
        m.coef[v, m.pa(v)[0]] = NAN
    elif rule == "inf-intercept":
        m.intercept[n - 1] = math.inf
    elif rule == "sd0":
        m.sd[0] = 0.0
    elif rule == "nan-sd":
        m.sd[n - 1] = NAN
    else:
        raise KeyError(rule)
    return m


RULES = {"cycle": 1, "bit": 16, "nan-coef": 64, "inf-intercept": 64, "sd0": 64, "nan-sd": 64}


@functools.lru_cache(maxsize=None)
def rows_for(n, S, seed=0):
    """held-out rows float64 [S, n]: tests/gaussian_corpus.py's dependent columns"""
    return gc.gauss_data(n, S, seed + 5)


def stack(nets):
    """the device layout of a batch: parents u64 [B, n], coef [B, n, n], intercept, sd [B, n]"""
    return (np.asarray([[p & ((1 << 64) - 1) for p in t.parents] for t in nets], U64), np.stack([t.coef for t in nets]),
            np.stack([t.intercept for t in nets]), np.stack([t.sd for t in nets]))


# ---------------------------------------------------------------------------------------------------------------------
# References and bounds
# ---------------------------------------------------------------------------------------------------------------------
@gc.at60
def exact_quantile(k):
    u = (mp.mpf(int(k)) + mp.mpf(1) / 2) / mp.mpf(TWO52)
    return mp.sqrt(2) * mp.erfinv(2 * u - 1)


def quantile_grid():
    """the integers the transform is held on: the ends, both sides of |q| = 0.425 and of r = 5, powers of two, 4096 seeded values"""
    ks = {0, 1, TWO52 - 1, TWO52 - 2}
    lo = int(0.075 * TWO52)                                  # u = 0.075: q = -0.425
    ks |= {lo + d for d in range(-3, 4)} | {TWO52 - 1 - lo - d for d in range(-3, 4)}
    far = int(math.exp(-25.0) * TWO52)                       # p = exp(-25): r = 5
    ks |= {far + d for d in range(-3, 4)} | {TWO52 - 1 - far - d for d in range(-3, 4)}
    ks |= {1 << e for e in range(52)} | {TWO52 - 1 - (1 << e) for e in range(52)}
    rng = np.random.default_rng(5100)
    ks |= {int(v) for v in rng.integers(0, TWO52, 3072)}
    ks |= {int(v) for v in rng.integers(0, 1 << 20, 512)} | {TWO52 - 1 - int(v) for v in rng.integers(0, 1 << 20, 512)}
    return sorted(ks)


@functools.lru_cache(maxsize=None)
@gc.at60
def quantile_grid_error():
    """{branch: the largest relative error of the restatement against mpmath} over the grid, and the points per branch"""
    worst, points = {b: 0.0 for b in BRANCHES}, {b: 0 for b in BRANCHES}
    for k in quantile_grid():
        z, br = restated_quantile(k)
        want = exact_quantile(k)
        b = BRANCHES[br]
        worst[b] = max(worst[b], float(abs(mp.mpf(z) - want) / abs(want)))
        points[b] += 1
    return worst, points


def _frac(a):
    return Fraction(float(a))


@functools.lru_cache(maxsize=None)
def exact_joint(key):
    """(mean [n], cov [n][n]) of the sound network NETS[key] in exact rationals: A = (I - B)^-1, mean = A c, cov = A D A^T"""
    net = NETS[key]
    n = net.n
    _, order = net_status(net)
    A = [[Fraction(0)] * n for _ in range(n)]
    for v in order:                                          # row v of A: e_v + sum_k b_vk A[k]
        A[v][v] = Fraction(1)
        for k in net.pa(v):
            b = _frac(net.coef[v, k])
            for j in range(n):
                if A[k][j]:
                    A[v][j] += b * A[k][j]
    c = [_frac(x) for x in net.intercept]
    d = [_frac(s) * _frac(s) for s in net.sd]
    mean = [sum(A[v][j] * c[j] for j in range(n) if A[v][j]) for v in range(n)]
    cov = [[sum(A[v][j] * d[j] * A[u][j] for j in range(n) if A[v][j] and A[u][j]) for u in range(n)] for v in range(n)]
    return mean, cov


@functools.lru_cache(maxsize=None)
def joint_bounds(key):
    """(M [n], E [n][n]): the module docstring's recursion, in exact rationals from the exact joint"""
    net = NETS[key]
    n = net.n
    mean, cov = exact_joint(key)
    _, order = net_status(net)
    g = lambda k: Fraction(k) * Fraction(U) / (1 - Fraction(k) * Fraction(U))
    M, E = [Fraction(0)] * n, [[Fraction(0)] * n for _ in range(n)]
    for i, v in enumerate(order):
        pa = net.pa(v)
        p, ab = len(pa), {k: abs(_frac(net.coef[v, k])) for k in pa}
        M[v] = sum(ab[k] * M[k] for k in pa) + g(p + 1) * (abs(_frac(net.intercept[v])) + sum(ab[k] * (abs(mean[k]) + M[k]) for k in pa))
        for u in order[:i]:
            E[v][u] = E[u][v] = sum(ab[k] * E[k][u] for k in pa) + g(p + 1) * sum(ab[k] * (abs(cov[k][u]) + E[k][u]) for k in pa)
        E[v][v] = sum(ab[k] * E[v][k] for k in pa) + g(p + 2) * (_frac(net.sd[v]) ** 2 + sum(ab[k] * (abs(cov[v][k]) + E[v][k]) for k in pa))
    return M, E


def assert_joint(mean, cov, key, what):
    """the computed joint against the exact one under joint_bounds -> the largest error / bound (0 where both are exact)"""
    em, ec = exact_joint(key)
    M, E = joint_bounds(key)
    n, worst = NETS[key].n, 0.0
    for v in range(n):
        err = abs(_frac(mean[v]) - em[v])
        assert err <= M[v], (what, "mean", v, float(err), float(M[v]))
        worst = max(worst, float(err / M[v]) if M[v] else 0.0)
        for u in range(n):
            err = abs(_frac(cov[v, u]) - ec[v][u])
            assert err <= E[v][u], (what, "cov", v, u, float(err), float(E[v][u]))
            worst = max(worst, float(err / E[v][u]) if E[v][u] else 0.0)
    return worst


def mu_bound(net, v, row, skip=-1):
    pa = [u for u in net.pa(v) if u != skip]
    return gamma(len(pa) + 1) * (abs(float(net.intercept[v])) + sum(abs(float(net.coef[v, u]) * float(row[u])) for u in pa))


@gc.at60
def exact_loglik_row(net, row):
    """(the row term in mpmath, its bound by the module docstring)"""
    term, bound, running = mp.mpf(0), 0.0, 0.0
    for v in range(net.n):
        sd = mp.mpf(float(net.sd[v]))
        mu = mp.mpf(float(net.intercept[v])) + sum(mp.mpf(float(net.coef[v, u])) * mp.mpf(float(row[u])) for u in net.pa(v))
        d = mp.mpf(float(row[v])) - mu
        e = d / sd
        c = mp.log(sd) + mp.log(2 * mp.pi) / 2
        piece = c + e * e / 2
        term -= piece
        dmu = mu_bound(net, v, row)
        ea = float(abs(e))
        de = (dmu + U * (float(abs(d)) + dmu)) / float(sd) + U * (ea + 1e-300)
        de = de * (1 + 4 * U)
        dq = 0.5 * (de * (2 * ea + de) + U * (ea + de) ** 2)
        dc = LOG_ULPS * 2 * U * float(abs(mp.log(sd))) + U * float(abs(c)) * (1 + 8 * U) + U * HALF_LOG_2PI      # the log, the addition, the constant's own rounding
        running += float(abs(piece)) + dq + dc
        bound += dq + dc + U * (float(abs(piece)) + dq + dc) + U * running
    return term, bound * (1 + 1e-9)


def out_bound(row_terms_abs, row_bounds, S):
    """the bound of out: the rows' bounds plus the two trees and the chunk chain over sum |terms|"""
    chunks = -(-S // 256)
    total = float(sum(row_terms_abs)) + float(sum(row_bounds))
    return float(sum(row_bounds)) + gamma(16 + -(-chunks // 256)) * total


@functools.lru_cache(maxsize=None)
def loglik_reference(key, n, S):
    """(terms [S] as mpf, bounds [S]) of NETS[key] on rows_for(n, S)"""
    net, x = NETS[key], rows_for(n, S)
    pairs = [exact_loglik_row(net, row) for row in x]
    return [p[0] for p in pairs], [p[1] for p in pairs]


@functools.lru_cache(maxsize=None)
@gc.at60
def conditional_reference(key, t):
    """the exact conditional of variable t of NETS[key] given all others from the rational joint: (weights over the others
    [n - 1] as mpf, the others' ids, the conditional variance)"""
    net = NETS[key]
    mean, cov = exact_joint(key)
    n = net.n
    others = [v for v in range(n) if v != t]
    mpq = lambda q: mp.mpf(q.numerator) / mp.mpf(q.denominator)
    if not others:
        return [], others, mpq(cov[t][t])
    Soo = mp.matrix([[mpq(cov[a][b]) for b in others] for a in others])
    Sot = mp.matrix([mpq(cov[a][t]) for a in others])
    w = mp.lu_solve(Soo, Sot)
    var = mpq(cov[t][t]) - sum(w[i] * Sot[i] for i in range(len(others)))
    return [w[i] for i in range(len(others))], others, var


@gc.at60
def exact_conditional_row(key, t, row):
    net = NETS[key]
    mean, _ = exact_joint(key)
    w, others, var = conditional_reference(key, t)
    mpq = lambda q: mp.mpf(q.numerator) / mp.mpf(q.denominator)
    return mpq(mean[t]) + sum(w[i] * (mp.mpf(float(row[o])) - mpq(mean[o])) for i, o in enumerate(others)), var


def predict_bound(net, t, row):
    """(the bound of mode 1's pred at this row, the relative bound of its var) by the module docstring, from the restated values"""
    n = net.n
    children = [c for c in range(n) if c != t and t in net.pa(c)]
    s = float(net.sd[t]) ** 2
    mu = restated_mu(net, t, row)
    prec, num_abs, num_err = 1.0 / s, abs(mu) / s, (mu_bound(net, t, row) + 3 * U * abs(mu)) / s
    num = mu / s
    for c in children:
        beta = float(net.coef[c, t])
        w = beta / float(net.sd[c]) ** 2
        m = restated_mu(net, c, row, skip=t)
        r = float(row[c]) - m
        dr = mu_bound(net, c, row, skip=t) + U * abs(r)
        num_err += abs(w) * dr + 3 * U * abs(w) * (abs(r) + dr)
        num_abs += abs(w * r)
        num += w * r
        prec += beta * w
    num_err += gamma(len(children) + 1) * (num_abs + num_err)
    rel_prec = gamma(len(children) + 4)
    pred = num / prec
    bound = (num_err + abs(pred) * rel_prec * prec) / (prec * (1 - rel_prec)) + U * abs(pred)
    return bound * (1 + 1e-9), (rel_prec / (1 - rel_prec) + U) * (1 + 1e-9)


def sample_bounds(key, x, z, branch):
    """[n_rows, n]: the bound of every cell of a build's sample against the restated one (0 where the row is all central)"""
    net = NETS[key]
    _, order = net_status(net)
    out = np.zeros_like(x)
    for i in range(len(x)):
        if not branch[i].any():
            continue
        for v in order:
            pa = net.pa(v)
            br = int(branch[i, v])
            dz = BUILD_FACTOR * QUANTILE_RTOL[BRANCHES[br]] * abs(float(z[i, v])) if br else 0.0
            mag = abs(float(net.intercept[v])) + sum(abs(float(net.coef[v, u]) * float(x[i, u])) for u in pa) + float(net.sd[v]) * abs(float(z[i, v]))
            out[i, v] = (sum(abs(float(net.coef[v, u])) * out[i, u] for u in pa) + float(net.sd[v]) * dz + 2 * gamma(len(pa) + 2) * mag) * (1 + 1e-9)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI on a back end
# ---------------------------------------------------------------------------------------------------------------------
def _put_nets(be, nets):
    return [be.put(a) for a in stack(nets)]


def run_joint(be, nets, guard=1):
    B, n = len(nets), nets[0].n
    par, coef, icpt, sd = _put_nets(be, nets)
    mean, cov, status = be.put(np.full((B + 2 * guard, n), SENTINEL)), be.put(np.full((B + 2 * guard, n, n), SENTINEL)), be.put(np.zeros(1, np.int32))
    at = lambda h, b: ctypes.c_void_p(be.ptr(h).value + b)
    gc.call(be, "dvs_gbn_joint", batch=B, n_vars=n, parents=par, coef=coef, intercept=icpt, sd=sd, mean=at(mean, guard * n * 8),
            cov=at(cov, guard * n * n * 8), cov_bytes=B * n * n * 8, status=status)
    m, c = np.array(be.get(mean), copy=True), np.array(be.get(cov), copy=True)
    for a in (m, c):
        assert (a[:guard] == SENTINEL).all() and (a[B + guard:] == SENTINEL).all()
    return m[guard:B + guard], c[guard:B + guard], int(be.get(status)[0])


def run_quantiles(be, ks):
    ks = np.asarray(ks, U64)
    z = be.put(np.full(len(ks) + 2, SENTINEL))
    gc.call(be, "dvs_gbn_quantiles", count=len(ks), k=be.put(ks), z=ctypes.c_void_p(be.ptr(z).value + 8))
    out = np.array(be.get(z), copy=True)
    assert out[0] == SENTINEL and out[-1] == SENTINEL
    return out[1:-1]


def run_sample(be, net, n_rows, seed, row_offset=0, guard=1):
    """dvs_gbn_sample -> (rows [n_rows, n], status); ``guard`` rows of sentinels around data_out must survive"""
    n = net.n
    par, coef, icpt, sd = _put_nets(be, [net])
    need = be.lib.dvs_gbn_sample_workspace_bytes(n)
    assert need == 256
    ws, out, status = be.put(np.zeros(need, np.uint8)), be.put(np.full((n_rows + 2 * guard, n), SENTINEL)), be.put(np.zeros(1, np.int32))
    gc.call(be, "dvs_gbn_sample", n_vars=n, n_rows=n_rows, parents=par, coef=coef, intercept=icpt, sd=sd, seed=seed, row_offset=row_offset,
            workspace=ws, workspace_bytes=need, data_out=ctypes.c_void_p(be.ptr(out).value + guard * n * 8), status=status)
    o = np.array(be.get(out), copy=True)
    assert (o[:guard] == SENTINEL).all() and (o[n_rows + guard:] == SENTINEL).all()
    return o[guard:n_rows + guard], int(be.get(status)[0])


def loglik_workspace(B, n, S):
    up = lambda v: (v + 255) & ~255
    return up(B * -(-S // 256) * 8) + up(B * n * 4) + B * n * 8


def run_loglik(be, nets, x, per_row=True):
    """dvs_gbn_loglik -> (out [B], per_row [B, S] or None, status)"""
    B, n, S = len(nets), nets[0].n, len(x)
    par, coef, icpt, sd = _put_nets(be, nets)
    need = loglik_workspace(B, n, S)
    ws, out, status = be.put(np.zeros(need, np.uint8)), be.put(np.full(B + 2, SENTINEL)), be.put(np.zeros(1, np.int32))
    rows = be.put(np.full((B + 2, S), SENTINEL)) if per_row else None
    gc.call(be, "dvs_gbn_loglik", batch=B, n_vars=n, n_rows=S, data=be.put(np.ascontiguousarray(x, np.float64)), parents=par, coef=coef,
            intercept=icpt, sd=sd, per_row=None if rows is None else ctypes.c_void_p(be.ptr(rows).value + S * 8),
            out=ctypes.c_void_p(be.ptr(out).value + 8), workspace=ws, workspace_bytes=need, status=status)
    o = np.array(be.get(out), copy=True)
    assert o[0] == SENTINEL and o[-1] == SENTINEL
    r = None
    if per_row:
        r = np.array(be.get(rows), copy=True)
        assert (r[0] == SENTINEL).all() and (r[-1] == SENTINEL).all()
        r = r[1:-1]
    return o[1:-1], r, int(be.get(status)[0])


def run_predict(be, nets, x, target, mode):
    """dvs_gbn_predict -> (pred [B, S], var [B], status)"""
    B, n, S = len(nets), nets[0].n, len(x)
    par, coef, icpt, sd = _put_nets(be, nets)
    need = (B * 4 + 255) & ~255
    ws, pred, var, status = (be.put(np.zeros(need, np.uint8)), be.put(np.full((B + 2, S), SENTINEL)), be.put(np.full(B + 2, SENTINEL)),
                             be.put(np.zeros(1, np.int32)))
    gc.call(be, "dvs_gbn_predict", batch=B, n_vars=n, n_rows=S, data=be.put(np.ascontiguousarray(x, np.float64)), parents=par, coef=coef,
            intercept=icpt, sd=sd, target=target, mode=mode, pred=ctypes.c_void_p(be.ptr(pred).value + S * 8),
            var=ctypes.c_void_p(be.ptr(var).value + 8), workspace=ws, workspace_bytes=need, status=status)
    p, v = np.array(be.get(pred), copy=True), np.array(be.get(var), copy=True)
    assert (p[0] == SENTINEL).all() and (p[-1] == SENTINEL).all() and v[0] == SENTINEL and v[-1] == SENTINEL
    return p[1:-1], v[1:-1], int(be.get(status)[0])


# ---------------------------------------------------------------------------------------------------------------------
# Checks on a back end
# ---------------------------------------------------------------------------------------------------------------------
def check_quantiles(be):
    """central outputs equal the restatement as bytes, tail outputs are within BUILD_FACTOR * QUANTILE_RTOL of it, k >= 2^52 is
    NaN, z(k) = -z(2^52 - 1 - k) as bytes -> {branch: (points, the largest relative difference)}"""
    ks = quantile_grid()
    got = run_quantiles(be, ks + [TWO52, TWO52 + 5, (1 << 64) - 1])
    assert np.isnan(got[len(ks):]).all()
    seen = {b: [0, 0.0] for b in BRANCHES}
    index = {k: i for i, k in enumerate(ks)}
    for i, k in enumerate(ks):
        z, br = restated_quantile(k)
        b = BRANCHES[br]
        seen[b][0] += 1
        if br == 0:
            assert np.float64(z).tobytes() == got[i].tobytes(), (k, z, got[i])
        else:
            rel = abs(float(got[i]) - z) / abs(z)
            assert rel <= BUILD_FACTOR * QUANTILE_RTOL[b], (k, z, got[i], rel)
            seen[b][1] = max(seen[b][1], rel)
        mirror = index.get(TWO52 - 1 - k)
        if mirror is not None:
            assert np.float64(-got[mirror]).tobytes() == got[i].tobytes(), (k, got[i], got[mirror])
    assert all(seen[b][0] > 10 for b in BRANCHES), seen
    return {b: tuple(v) for b, v in seen.items()}


def joint_cases():
    return [("one", 1), ("dag", 5), ("full", 5), ("dag", 17), ("full", 17), ("dag", 48), ("full", 48)]


def check_joint(be, n):
    """the networks of n variables in one call, a malformed one of every rule between them: sound ones equal the restatement as
    bytes with both triangles alike, the malformed ones are NaN and set their bit alone"""
    keys = [k for k in joint_cases() if k[1] == n]
    assert keys
    if n >= 5:
        assert len(NETS[("full", n)].pa(n // 2 - 1)) == n - 1
        assert net_status(NETS[("dag", n)])[1] != list(range(n))
    sound = [NETS[k] for k in keys]
    m, c, st = run_joint(be, sound)
    assert st == 0
    for b, net in enumerate(sound):
        rm, rc = restated_joint(net)
        assert m[b].tobytes() == rm.tobytes() and c[b].tobytes() == rc.tobytes(), (keys[b], np.argwhere(c[b] != rc)[:4])
        assert c[b].tobytes() == np.ascontiguousarray(c[b].T).tobytes()
    if n == 1:
        rules = ("inf-intercept", "sd0", "nan-sd", "bit")
    else:
        rules = tuple(RULES)
    for rule in rules:
        bad = malformed(sound[0], rule)
        assert net_status(bad)[0] == RULES[rule], rule
        m2, c2, st2 = run_joint(be, [sound[0], bad, sound[-1]])
        assert st2 == RULES[rule], (rule, st2)
        assert np.isnan(m2[1]).all() and np.isnan(c2[1]).all()
        assert m2[0].tobytes() == m[0].tobytes() and c2[2].tobytes() == c[-1].tobytes(), rule


def sample_key(n):
    return ("one", 1) if n == 1 else ("full", n)


def check_sample(be, n, n_rows, seed=77):
    """rows whose draws are all central equal the restatement as bytes, every other cell lies within sample_bounds; two calls
    give equal bytes -> (central rows, the largest error / bound elsewhere)"""
    key = sample_key(n)
    net = NETS[key]
    x, z, branch = restated_sample(key, n_rows, seed)
    got, st = run_sample(be, net, n_rows, seed)
    again, _ = run_sample(be, net, n_rows, seed)
    assert st == 0 and got.tobytes() == again.tobytes()
    central = ~branch.any(axis=1)
    if n == 5 and n_rows > 1:                                # on the restatement first: 0.85^5 = 0.44 of the rows are expected
        assert int(central.sum()) >= n_rows // 4, (n_rows, int(central.sum()))
    assert got[central].tobytes() == x[central].tobytes(), (n, n_rows, np.argwhere(got[central] != x[central])[:4])
    bounds = sample_bounds(key, x, z, branch)
    err = np.abs(got - x)
    assert (err <= bounds).all(), (n, n_rows, np.argwhere(err > bounds)[:4])
    worst = float(np.max(err[~central] / bounds[~central])) if (~central).any() else 0.0
    return int(central.sum()), worst


def check_sample_cut(be, n=17, seed=78):
    """a request cut into three calls with consecutive row_offset gives the bytes of the uncut one; an offset that wraps 2^32"""
    net = NETS[sample_key(n)]
    whole, _ = run_sample(be, net, 600, seed, row_offset=40)
    parts = [run_sample(be, net, m, seed, row_offset=40 + at)[0] for at, m in ((0, 255), (255, 88), (343, 257))]
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    other, _ = run_sample(be, net, 600, seed + 1, row_offset=40)
    assert other.tobytes() != whole.tobytes()
    wrap, _ = run_sample(be, net, 4, seed, row_offset=(1 << 32) - 2)
    assert wrap[2:].tobytes() == run_sample(be, net, 2, seed, row_offset=0)[0].tobytes()


def check_sample_refusals(be, n=5):
    """each status rule, alone, leaves data_out untouched between sentinels"""
    net = NETS[("dag", n)]
    for rule, bit in RULES.items():
        got, st = run_sample(be, malformed(net, rule), 300, 5)
        assert st == bit and (got == SENTINEL).all(), (rule, st)
    got, st = run_sample(be, net, 300, 5)
    assert st == 0 and not (got == SENTINEL).any()


def batch_nets(B):
    return [NETS[("batch", i)] for i in range(B)]


def assert_loglik_near_restatement(net, x, rows, out, what):
    """one structure's row terms and out against the restatement under restated_loglik_rows_fast's bound -> worst error / bound"""
    rest, bounds = restated_loglik_rows_fast(net, x)
    err = np.abs(rows - rest)
    assert (err <= bounds).all(), (what, int(np.argmax(err - bounds)), float(err.max()))
    ob = out_bound_between_builds(rest, bounds)
    assert abs(float(out) - stated_sum(rest)) <= ob, (what, "out", float(out), stated_sum(rest), ob)
    return float(np.max(err / bounds))


def check_loglik(be, B, S):
    """per_row null and given give equal out bytes; out is the stated tree over per_row as bytes; every structure's rows and out
    lie within the derived bound of the restatement, and structures 0, B // 2 and B - 1 within it of mpmath -> worst error / bound"""
    n = 5
    nets, x = batch_nets(B), rows_for(n, S)
    out, rows, st = run_loglik(be, nets, x)
    out2, _, st2 = run_loglik(be, nets, x, per_row=False)
    assert st == 0 and st2 == 0 and out.tobytes() == out2.tobytes()
    worst = 0.0
    for b in range(B):
        assert np.float64(stated_sum(rows[b])).tobytes() == out[b].tobytes(), (B, S, b)
        assert_loglik_near_restatement(nets[b], x, rows[b], out[b], (B, S, b))
    for b in sorted({0, B // 2, B - 1}):
        terms, bounds = loglik_reference(("batch", b), n, S)
        rest = restated_loglik_rows(nets[b], x)
        for i in range(S):
            for have in (rows[b, i], rest[i]):
                err = float(abs(mp.mpf(float(have)) - terms[i]))
                assert err <= bounds[i], (B, S, b, i, float(have), float(terms[i]), err, bounds[i])
            worst = max(worst, float(abs(mp.mpf(float(rows[b, i])) - terms[i])) / bounds[i])
        ob = out_bound([float(abs(t)) for t in terms], bounds, S)
        with mp.workdps(gc.DPS):
            err = float(abs(mp.mpf(float(out[b])) - mp.fsum(terms)))
        assert err <= ob, (B, S, b, "out", err, ob)
        worst = max(worst, err / ob)
    return worst


def check_loglik_two_chunks_in_a_slot(be):
    """n = 2, S = 65 537: 257 chunks, so slot 0 of the second array adds chunks 0 and 256.  The row terms lie within the derived
    bound of mpmath on every 61st row and on the last one; out is the stated tree over per_row as bytes"""
    n, S = 2, 65537
    net, x = NETS[("pair", 2)], rows_for(n, S)
    out, rows, st = run_loglik(be, [net], x)
    out2, _, _ = run_loglik(be, [net], x, per_row=False)
    assert st == 0 and out.tobytes() == out2.tobytes()
    assert np.float64(stated_sum(rows[0])).tobytes() == out[0].tobytes()
    for i in list(range(0, S, 61)) + [S - 1]:
        term, bound = exact_loglik_row(net, x[i])
        assert float(abs(mp.mpf(float(rows[0, i])) - term)) <= bound, (i, rows[0, i], float(term), bound)


def check_loglik_malformed(be):
    """a malformed structure of every rule is NaN between well-formed neighbours, which keep their bytes; bit 4 alone"""
    n, S = 5, 300
    nets, x = batch_nets(3), rows_for(n, S)
    out, rows, _ = run_loglik(be, nets, x)
    for rule in RULES:
        mixed = [nets[0], malformed(nets[1], rule), nets[2]]
        o, r, st = run_loglik(be, mixed, x)
        assert st == 16, (rule, st)
        assert np.isnan(o[1]) and np.isnan(r[1]).all() and np.isnan(restated_loglik_rows(mixed[1], x)).all()
        assert o[[0, 2]].tobytes() == out[[0, 2]].tobytes() and r[[0, 2]].tobytes() == rows[[0, 2]].tobytes(), rule
    poisoned = np.array(x, copy=True)
    poisoned[7, 2], poisoned[9, 0] = NAN, math.inf
    o, r, st = run_loglik(be, nets, poisoned)
    assert st == 0 and np.isnan(r[:, 7]).all() and not np.isfinite(r[:, 9]).any() and np.isfinite(np.delete(r, [7, 9], axis=1)).all()


MANY_B, MANY_S = 65, 10241
MANY_BAD = {7: "cycle", 32: "sd0", 40: "bit"}


def many_nets():
    """65 structures on 10 241 rows: 41 chunks, so the launcher (csrc/dvs_gaussian_params.h: gpar_bsplit) cuts the batch into
    ceil(1024 / 41) = 25 parts and a workgroup loops over two or three structures, b, b + 25, b + 50; part 7 holds the malformed
    7 and 32 and the sound 57, part 15 the sound 15 and the malformed 40"""
    chunks = -(-MANY_S // 256)
    parts = -(-1024 // chunks)
    assert parts < MANY_B and MANY_B > 2 * parts and (32 - 7) % parts == 0
    return [malformed(net, MANY_BAD[b]) if b in MANY_BAD else net for b, net in enumerate(batch_nets(MANY_B))]


def check_loglik_many_structures_per_workgroup(be):
    """every sound structure's rows within the bound of the restatement and out the stated tree over them; the malformed ones
    NaN, bit 4; structures 0, 25 and 50 (one workgroup's loop) against mpmath on every 499th row -> worst error / bound"""
    n = 5
    nets, x = many_nets(), rows_for(n, MANY_S)
    out, rows, st = run_loglik(be, nets, x)
    out2, _, _ = run_loglik(be, nets, x, per_row=False)
    assert st == 16 and out.tobytes() == out2.tobytes()
    worst = 0.0
    for b, net in enumerate(nets):
        if b in MANY_BAD:
            assert np.isnan(out[b]) and np.isnan(rows[b]).all(), b
            continue
        assert np.float64(stated_sum(rows[b])).tobytes() == out[b].tobytes(), b
        worst = max(worst, assert_loglik_near_restatement(net, x, rows[b], out[b], ("many", b)))
    for b in (0, 25, 50):
        for i in list(range(0, MANY_S, 499)) + [MANY_S - 1]:
            term, bound = exact_loglik_row(nets[b], x[i])
            assert float(abs(mp.mpf(float(rows[b, i])) - term)) <= bound, (b, i, rows[b, i], float(term), bound)
    return worst


def check_predict_many_structures_per_workgroup(be):
    """both modes have no library call: every sound structure's predictions and variance equal the restatement as bytes, the
    malformed ones are NaN, bit 4"""
    n, t = 5, 2
    nets, x = many_nets(), rows_for(n, MANY_S)
    for mode in (0, 1):
        pred, var, st = run_predict(be, nets, x, t, mode)
        assert st == 16
        for b, net in enumerate(nets):
            rp, rv = restated_predict_fast(net, t, mode, x)
            if b in MANY_BAD:
                assert np.isnan(pred[b]).all() and np.isnan(var[b]) and np.isnan(rp).all(), (mode, b)
                continue
            assert pred[b].tobytes() == rp.tobytes(), (mode, b, np.argwhere(pred[b] != rp)[:4])
            assert np.float64(rv).tobytes() == var[b].tobytes(), (mode, b)


def check_loglik_wide(be, n, S=300):
    """n = 17 and 48 (the 96 KiB image, a variable with n - 1 parents): three structures against the restatement on every row
    and against mpmath on the first 12 -> worst error / bound of the mpmath comparison"""
    keys = [("hub", n), ("dag", n), ("full", n)]
    nets, x = [NETS[k] for k in keys], rows_for(n, S)
    out, rows, st = run_loglik(be, nets, x)
    assert st == 0
    worst = 0.0
    for b, net in enumerate(nets):
        assert np.float64(stated_sum(rows[b])).tobytes() == out[b].tobytes(), (n, b)
        assert_loglik_near_restatement(net, x, rows[b], out[b], (n, keys[b]))
        for i in range(12):
            term, bound = exact_loglik_row(net, x[i])
            err = float(abs(mp.mpf(float(rows[b, i])) - term))
            assert err <= bound, (n, keys[b], i, err, bound)
            worst = max(worst, err / bound)
    return worst


def check_predict(be, n, S=300):
    """both modes for a target with no children, one with no parents and one with many children, three structures a call: mode
    0 and mode 1 equal the restatement as bytes (neither has a library call), mode 1 lies within predict_bound of the mpmath
    conditional on the first 40 rows, var alike; the target's
    column filled with NaN changes nothing -> worst mode 1 error / bound"""
    keys = [("hub", n), ("dag", n), ("full", n)]
    nets, x = [NETS[k] for k in keys], rows_for(n, S)
    kids = lambda net, t: sum(1 for c in range(n) if c != t and t in net.pa(c))
    targets = sinks_and_sources(nets[0])
    assert kids(nets[0], targets[0]) == 0 and not nets[0].pa(targets[1]) and kids(nets[0], targets[2]) >= n // 3
    worst = 0.0
    for t in targets:
        blind = np.array(x, copy=True)
        blind[:, t] = NAN
        for mode in (0, 1):
            pred, var, st = run_predict(be, nets, x, t, mode)
            pred2, var2, _ = run_predict(be, nets, blind, t, mode)
            assert st == 0 and pred.tobytes() == pred2.tobytes() and var.tobytes() == var2.tobytes()
            for b, net in enumerate(nets):
                if mode == 0:
                    rp, rv = restated_predict(net, t, 0, x)
                    assert pred[b].tobytes() == rp.tobytes() and np.float64(rv).tobytes() == var[b].tobytes(), (n, t, keys[b])
                    continue
                fp, fv = restated_predict_fast(net, t, 1, x)
                assert pred[b].tobytes() == fp.tobytes() and np.float64(fv).tobytes() == var[b].tobytes(), (n, t, keys[b])
                rp, rv = restated_predict(net, t, 1, x[:40])
                for i in range(40):
                    want, wvar = exact_conditional_row(keys[b], t, x[i])
                    bound, rel = predict_bound(net, t, x[i])
                    for have in (pred[b, i], rp[i]):
                        err = float(abs(mp.mpf(float(have)) - want))
                        assert err <= bound, (n, t, keys[b], i, float(have), float(want), err, bound)
                    worst = max(worst, float(abs(mp.mpf(float(pred[b, i])) - want)) / bound)
                assert float(abs(mp.mpf(float(var[b])) - wvar) / wvar) <= rel, (n, t, keys[b], "var", float(var[b]), float(wvar))
    return worst


def check_predict_malformed(be):
    n, S = 5, 300
    nets, x = batch_nets(3), rows_for(n, S)
    for mode in (0, 1):
        pred, var, _ = run_predict(be, nets, x, 2, mode)
        for rule in ("cycle", "bit", "sd0"):
            p, v, st = run_predict(be, [nets[0], malformed(nets[1], rule), nets[2]], x, 2, mode)
            assert st == 16 and np.isnan(p[1]).all() and np.isnan(v[1]), (rule, st)
            assert p[[0, 2]].tobytes() == pred[[0, 2]].tobytes() and v[[0, 2]].tobytes() == var[[0, 2]].tobytes()


def check_argument_refusals(lib, ptr):
    """the codes the header states, each before anything is enqueued (dummy non-null pointers do), in the documented order"""
    def joint(**kw):
        a = dict(B=2, n=5, par=ptr, coef=ptr, icpt=ptr, sd=ptr, mean=ptr, cov=ptr, cb=2 * 25 * 8, status=ptr)
        a.update(kw)
        return lib.dvs_gbn_joint(a["B"], a["n"], a["par"], a["coef"], a["icpt"], a["sd"], a["mean"], a["cov"], a["cb"], a["status"], None)
    assert joint(B=0) == 2 and joint(n=0) == 3 and joint(n=49) == 3 and joint(B=0, n=0) == 2
    assert joint(B=(1 << 31) // (48 * 48) + 1, n=48) == 2 and b"2^31" in lib.dvs_last_error()
    assert all(joint(**{k: None}) == 10 for k in ("par", "coef", "icpt", "sd", "mean", "cov", "status"))
    assert joint(n=0, par=None) == 3 and joint(par=None, cb=0) == 10 and joint(cb=399) == 14 and b"400" in lib.dvs_last_error()

    assert lib.dvs_gbn_quantiles(0, ptr, ptr, None) == 2 and lib.dvs_gbn_quantiles(1 << 31, ptr, ptr, None) == 2
    assert lib.dvs_gbn_quantiles(4, None, ptr, None) == 10 and lib.dvs_gbn_quantiles(4, ptr, None, None) == 10
    assert lib.dvs_gbn_quantiles(0, None, ptr, None) == 2

    assert lib.dvs_gbn_sample_workspace_bytes(0) == 0 and lib.dvs_gbn_sample_workspace_bytes(49) == 0
    assert lib.dvs_gbn_sample_workspace_bytes(1) == 256 and lib.dvs_gbn_sample_workspace_bytes(48) == 256

    def sample(**kw):
        a = dict(n=5, rows=10, par=ptr, coef=ptr, icpt=ptr, sd=ptr, seed=1, off=0, ws=ptr, wb=256, out=ptr, status=ptr)
        a.update(kw)
        return lib.dvs_gbn_sample(a["n"], a["rows"], a["par"], a["coef"], a["icpt"], a["sd"], a["seed"], a["off"], a["ws"], a["wb"], a["out"],
                                  a["status"], None)
    assert sample(rows=0) == 2 and sample(rows=1 << 31) == 2 and sample(n=0) == 3 and sample(n=49) == 3 and sample(off=-1) == 12
    assert all(sample(**{k: None}) == 10 for k in ("par", "coef", "icpt", "sd", "ws", "out", "status"))
    assert sample(wb=255) == 14 and b"256" in lib.dvs_last_error()
    assert sample(rows=0, n=0) == 2 and sample(n=0, off=-1) == 3 and sample(off=-1, par=None) == 12 and sample(par=None, wb=0) == 10

    def loglik(**kw):
        a = dict(B=3, n=5, rows=300, data=ptr, par=ptr, coef=ptr, icpt=ptr, sd=ptr, per=ptr, out=ptr, ws=ptr, wb=loglik_workspace(3, 5, 300), status=ptr)
        a.update(kw)
        return lib.dvs_gbn_loglik(a["B"], a["n"], a["rows"], a["data"], a["par"], a["coef"], a["icpt"], a["sd"], a["per"], a["out"], a["ws"], a["wb"],
                                  a["status"], None)

    def predict(**kw):
        a = dict(B=3, n=5, rows=300, data=ptr, par=ptr, coef=ptr, icpt=ptr, sd=ptr, t=2, mode=1, pred=ptr, var=ptr, ws=ptr, wb=256, status=ptr)
        a.update(kw)
        return lib.dvs_gbn_predict(a["B"], a["n"], a["rows"], a["data"], a["par"], a["coef"], a["icpt"], a["sd"], a["t"], a["mode"], a["pred"],
                                   a["var"], a["ws"], a["wb"], a["status"], None)
    for fn in (loglik, predict):
        assert fn(B=0) == 2 and fn(rows=0) == 2 and fn(rows=1 << 31) == 2 and fn(n=0) == 3 and fn(n=49) == 3
        assert fn(B=1 << 30, n=48) == 2 and b"2^31" in lib.dvs_last_error()
        assert all(fn(**{k: None}) == 10 for k in ("data", "par", "coef", "icpt", "sd", "ws", "status"))
        assert fn(B=0, n=0) == 2 and fn(n=0, data=None) == 3 and fn(data=None, wb=0) == 10
    assert loglik(per=None, out=None) == 10 and loglik(out=None) == 10
    assert loglik(wb=loglik_workspace(3, 5, 300) - 1) == 14 and str(loglik_workspace(3, 5, 300)).encode() in lib.dvs_last_error()
    assert predict(t=-1) == 13 and predict(t=5) == 13 and predict(mode=2) == 12 and predict(mode=-1) == 12
    assert predict(n=0, t=-1) == 3 and predict(t=-1, mode=2) == 13 and predict(mode=2, data=None) == 12
    assert predict(pred=None) == 10 and predict(var=None) == 10 and predict(wb=255) == 14 and b"256" in lib.dvs_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# Closing the loop on the CPU: the restated sample, the restated bge scores, every DAG on five variables
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loop_reference():
    """the restated rows of LOOP_NET, the restated bge local scores of all 5 * 16 families on their restated moments, the best
    equivalence class over all 29 281 DAGs and its gap to the best other class"""
    x, _, _ = restated_sample(("loop", 5), LOOP_ROWS, LOOP_SEED)
    mom = gc.restated_moments(np.ascontiguousarray(x))[0]
    n = 5
    table = np.full((n, 1 << n), NAN)
    for v in range(n):
        for pm in range(1 << n):
            if not (pm >> v) & 1:
                table[v, pm] = gc.restated_local(mom, n, v, pm, "bge")
    dags = gc.all_dags(n)
    scores = sum(table[v, dags[:, v]] for v in range(n))
    best = int(np.argmax(scores))
    truth = gc.cpdag_key(LOOP_NET.parents)
    best_key = gc.cpdag_key([int(m) for m in dags[best]])
    others = [float(s) for d, s in zip(dags, scores) if s > scores[best] - 50.0 and gc.cpdag_key([int(m) for m in d]) != best_key]
    gap = float(scores[best]) - max(others) if others else 50.0
    return SimpleNamespace(x=x, best=[int(m) for m in dags[best]], best_key=best_key, truth=truth, gap=gap, n_dags=len(dags),
                           score=float(scores[best]))
