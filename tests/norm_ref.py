"""fp64 numpy restatement of csrc/norm.hip (per-channel statistics, GroupNorm / InstanceNorm coefficients forward and
backward, the apply passes, MaxPool3d(2) with its first-maximum winners, the lazy InstanceNorm backward, nearest upsample +
concat, the range scale) and the case table of its conformance tests.  Every op takes ONE sample in NDHWC order (fp32 arrays
are promoted to fp64); only gn_bwd_coeffs takes the batch, because dgamma and dbeta sum over it.

u = eps32 / 2 (one fp32 rounding).  Bars, each derived from the arithmetic the kernel is built on, none from a run of it:

  statistics   a lane adds at most 64 fp32 terms before it hands over to fp64, so with the running-error bound of a
               sequential sum (63 additions, plus the rounding of each product where there is one)
                   |sum a - truth| <= 64 u sum|a|,   |sum a^2 - truth| <= 65 u sum a^2,   |sum ab - truth| <= 65 u sum|ab|.
               emulate_stats_fp32 sums in the kernel's own order (lane stride `rows`, chunks of 64, block split `per`, fp64
               above) with the product rounded separately (the compiler may fuse it, which only removes a rounding).
               Worst ratio error / bar of the emulation over the whole statistics table (test_norm_reference_cpu.py):
               sum a 0.044, sum a^2 0.064 (both at V = 333, C = 1024, one lane per channel quad), sum ab 0.027 (V = 333, C =
               255) -- the rounding errors of a lane's terms add like a random walk, not like the worst case.  The kernel on
               gfx950 measures 0.056 over the same table (test_norm_edges_gpu.py).
  coefficients fp64 inside, one rounding on the store:  |got - truth| <= 2 u |truth| + 8 floor, per element, the floor per
               output array = max |fp64 restatement - the same formulas in long double| on the same inputs (coeff_floor;
               the GPU tests evaluate it for the very case they check).  Measured per case group over the (C, G) table, N =
               3, x = 1.5 + randn, relative to max|truth| of the array (test_norm_reference_cpu.py prints them):
                 forward   count 333: scale, shift <= 5.0e-16, mean_rstd <= 2.9e-16; count 1: <= 6.8e-16, but 3.0e-14 at (C,
                           G) = (12, 4) without affine, where a group is 3 values and var = ss / m - mean^2 loses two digits;
                           count 1 with G = C is a variance of exactly 0: rstd = 1 / sqrt(eps) to 1.3e-16
                 backward  c1 0 (one product), c2 <= 3.8e-16, c3 <= 3.8e-16, dgamma <= 2.7e-16, dbeta 0 (a plain sum)
                 fold      c123 <= 1.4e-16, dgamma <= 2.3e-16 (S2 = sum(bhat - beta A) cancels beta A at most one digit here)
               Everywhere 8 floor <= 2e-6 of 2 u max|truth|: the one fp32 rounding carries the bar, and the kernels sit at
               0.50 of it.
  apply        fp32 arithmetic, three terms: 3 u (|c1 g| + |c2 x| + |c3|) per element (two products, two additions, each
               result bounded by the sum of magnitudes; a fused multiply-add only removes roundings).  norm_apply the same
               with two terms: 3 u (|x scale| + |shift|).  Masked elements are exactly 0.
  moving ops   pooling, winners, scatter, upcat forward, upcat's skip gradient, layout, ReLU mask: bit equality.
               upcat's low gradient sums up to 27 fp32 terms (3 per axis at n_out = 2 n_in + 1): 27 u sum|terms|.
  chains       the statistics bounds pushed to first order through every formula by `Err` below -- value and absolute error
               bound travel together:  (a + b).e = a.e + b.e,  (a b).e = |a| b.e + |b| a.e (+ a.e b.e),  (a / b).e = a.e / |b| + |a| b.e /
               b^2,  rsqrt(a).e = a.e / (2 |a|^1.5),  a sum adds its terms' bounds, and every value that the kernels store
               as fp32 gains u |value| (Err.r32).  Written out for the forward of a group of m = count cpg elements:
                   d_mean <= 64 u mean|x|                     d_var <= 65 u mean(x^2) + 2 |mean| d_mean
                   d_rstd <= rstd^3 d_var / 2 + u rstd        (so d_rstd / rstd ~ 97 u (mean / std)^2: 5e-3 at mean / std
                                                              = 30, 6e-2 at 100, 6 at 1000 -- the sum-of-squares design is
                                                              good to mean / std ~ 40 for a 1e-2 bar on rstd)
                   d_scale <= |gamma| d_rstd + u |scale|      d_shift <= |gamma| (|mean| d_rstd + rstd d_mean) + u |shift|
                   d_y <= |x| d_scale + d_shift + 3 u (|x scale| + |shift|)
               and the backward likewise from d_A <= 64 u sum|g|, d_B <= 65 u sum|g x| and the fp32 mean, rstd it reads.
               The bound treats |x| d_scale and d_shift as independent although they nearly cancel ((x - mean) d_rstd is the
               true sensitivity), so it is loose by ~ mean / std; it is an upper bound all the same.  So that it stays one
               where the errors are not small (mean / std >= 100: d_var can exceed var), a product also carries a.e b.e and
               rsqrt takes the larger of the first-order term and the exact one-sided value 1 / sqrt(max(a - a.e, eps)) -
               1 / sqrt(a): the kernels clamp the variance at 0, so rstd never exceeds 1 / sqrt(eps).

Classes of the data generators (asserted in test_norm_reference_cpu.py): "const" has one channel of variance exactly 0;
tie volumes have a tie for the maximum in every window; kink-free volumes have |zhat| >= 1e-3 everywhere, so that the fp32
ReLU mask of the kernels and the fp64 one of the truth cannot differ and no element is left out of a comparison.
"""
import functools

import numpy as np

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
U = EPS32 / 2
EPS = float(np.float32(1e-5))            # GroupNorm's eps as the kernels receive it (a C float)
LD = np.longdouble


def _d(a, dtype=np.float64):
    return None if a is None else np.asarray(a, dtype=dtype)


# --------------------------------------------------------------------------------------------------------- statistics
def channel_sums(a, b=None):
    """a, b (V, C) -> (sum a, sum a^2) or (sum a, sum a b) per channel, fp64"""
    a = _d(a)
    return a.sum(0), (a * a if b is None else a * _d(b)).sum(0)


def stats_bars(a, b=None):
    a = _d(a)
    return 64 * U * np.abs(a).sum(0), 65 * U * np.abs(a * a if b is None else a * _d(b)).sum(0)


def stats_geometry(V, C):
    """the launch of kmh_channel_stats / kmh_in_bwd_stats: (VEC, CQ, rows, nblk, per), or None where it answers -22"""
    v4 = C % 4 == 0 and C // 4 <= 256
    CQ = C // 4 if v4 else C
    if C > 1024 or CQ > 256 or (256 // CQ) * C * 16 > 64 * 1024:
        return None
    nblk = max(1, min(512, -(-V // 2048)))
    return (4 if v4 else 1), CQ, 256 // CQ, nblk, -(-V // nblk)


def emulate_stats_fp32(a, b, V, C):
    """the kernel's own summation order in float32: voxel v of block k goes to lane (v - k per) % rows, a lane adds its terms
    in order in fp32 and hands over to fp64 every 64; lanes, then blocks, add in fp64.  a, b (V, C) float32 -> two (C,) fp64"""
    _, _, rows, nblk, per = stats_geometry(V, C)
    a = np.asarray(a, F32).reshape(V, C)
    p = a * a if b is None else a * np.asarray(b, F32).reshape(V, C)          # fp32 product, rounded on its own
    out = np.zeros((2, C))
    for k in range(nblk):
        lo, hi = k * per, min(V, (k + 1) * per)
        if hi <= lo:
            continue
        L = -(-(hi - lo) // rows)
        L64 = -(-L // 64) * 64
        for j, t in enumerate((a, p)):
            buf = np.zeros((L64 * rows, C), F32)                              # zero padding: x + 0 is exact
            buf[:hi - lo] = t[lo:hi]
            buf = buf.reshape(L64 // 64, 64, rows, C)
            f = np.zeros((L64 // 64, rows, C), F32)
            for i in range(64):
                f = f + buf[:, i]
            out[j] += f.astype(np.float64).sum((0, 1))
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------------- coefficients
def gn_fwd_coeffs(stats, gamma, beta, G, count, eps=EPS, dtype=np.float64):
    """stats (C, 2) -> scale (C), shift (C), mean_rstd (G, 2): scale = rstd gamma, shift = beta - mean rstd gamma"""
    st = _d(stats, dtype)
    C = st.shape[0]
    cpg = C // G
    m = dtype(count) * dtype(cpg)
    s, ss = st[:, 0].reshape(G, cpg).sum(1), st[:, 1].reshape(G, cpg).sum(1)
    mean = s / m
    var = np.maximum(ss / m - mean * mean, dtype(0))
    rstd = dtype(1) / np.sqrt(var + dtype(eps))
    ga = np.ones(C, dtype) if gamma is None else _d(gamma, dtype)
    be = np.zeros(C, dtype) if beta is None else _d(beta, dtype)
    mc, rc = np.repeat(mean, cpg), np.repeat(rstd, cpg)
    return rc * ga, be - mc * rc * ga, np.stack([mean, rstd], 1)


def _bwd_tail(S1, S2, ga, mean, rstd, m, cpg, N, C):
    rep = lambda t: np.repeat(t, cpg, axis=1)                                                           # noqa: E731
    c1 = rep(rstd) * ga
    c2 = rep(-rstd * rstd * S2 / m)
    c3 = rep(-rstd * S1 / m + rstd * rstd * S2 * mean / m)
    return np.stack([c1, c2 + 0 * c1, c3 + 0 * c1], -1)


def gn_bwd_coeffs(ab, gamma, mean_rstd, G, count, dtype=np.float64):
    """ab (N, C, 2) = (sum dxn, sum dxn x), mean_rstd (N, G, 2) -> c123 (N, C, 3), dgamma (C), dbeta (C) summed over N;
    dx = c1 dxn + c2 x + c3"""
    ab, mr = _d(ab, dtype), _d(mean_rstd, dtype)
    N, C = ab.shape[:2]
    cpg = C // G
    m = dtype(count) * dtype(cpg)
    ga = np.ones(C, dtype) if gamma is None else _d(gamma, dtype)
    A, B = ab[..., 0], ab[..., 1]
    mean, rstd = mr[..., 0], mr[..., 1]
    mc, rc = np.repeat(mean, cpg, 1), np.repeat(rstd, cpg, 1)
    S1 = (ga * A).reshape(N, G, cpg).sum(2)
    S2 = (ga * rc * (B - mc * A)).reshape(N, G, cpg).sum(2)
    return _bwd_tail(S1, S2, ga, mean, rstd, m, cpg, N, C), (rc * (B - mc * A)).sum(0), A.sum(0)


def fold_inputs(ab, gamma, beta, mean_rstd, G):
    """(dstats, bhat) that the fold route receives for the same data: bhat = sum dxn xhat, xhat = gamma (x - mean) rstd + beta"""
    ab, mr = _d(ab), _d(mean_rstd)
    C = ab.shape[1]
    cpg = C // G
    ga = np.ones(C) if gamma is None else _d(gamma)
    be = np.zeros(C) if beta is None else _d(beta)
    A, B = ab[..., 0], ab[..., 1]
    mc, rc = np.repeat(mr[..., 0], cpg, 1), np.repeat(mr[..., 1], cpg, 1)
    return np.stack([A, np.zeros_like(A)], -1), ga * rc * (B - mc * A) + be * A


def gn_bwd_coeffs_fold(dstats, bhat, gamma, beta, mean_rstd, G, count, dtype=np.float64):
    """the same coefficients from (dstats (N, C, 2)[..., 0] = A, bhat (N, C), beta): gamma sum dxn xt = bhat - beta A"""
    ds, bh, mr = _d(dstats, dtype), _d(bhat, dtype), _d(mean_rstd, dtype)
    N, C = bh.shape
    cpg = C // G
    m = dtype(count) * dtype(cpg)
    ga = np.ones(C, dtype) if gamma is None else _d(gamma, dtype)
    be = np.zeros(C, dtype) if beta is None else _d(beta, dtype)
    A = ds[..., 0]
    S1 = (ga * A).reshape(N, G, cpg).sum(2)
    S2 = (bh - be * A).reshape(N, G, cpg).sum(2)
    return _bwd_tail(S1, S2, ga, mr[..., 0], mr[..., 1], m, cpg, N, C), ((bh - be * A) / ga).sum(0), A.sum(0)


def coeff_floor(fn, *args):
    """per output array: max |fp64 restatement - the same formulas in long double| (the cancellation floor), and the fp64 outputs"""
    lo, hi = fn(*args, dtype=np.float64), fn(*args, dtype=LD)
    return [float(np.abs(a.astype(LD) - b).max()) for a, b in zip(lo, hi)], lo


def coeff_bar(truth, floor):
    return 2 * U * np.abs(truth) + 8 * floor


# -------------------------------------------------------------------------------------------------------------- apply
def gn_bwd_apply(dxn, x, c123, relu_mask):
    """dxn, x (V, C), c123 (C, 3) -> dx = [x > 0] (c1 dxn + c2 x + c3) and its bar 3 u (|c1 dxn| + |c2 x| + |c3|)"""
    g, x, c = _d(dxn), _d(x), _d(c123)
    t1, t2, t3 = c[:, 0] * g, c[:, 1] * x, c[:, 2] + 0 * x
    keep = (x > 0) if relu_mask else np.ones(x.shape, bool)
    return np.where(keep, t1 + t2 + t3, 0.0), np.where(keep, 3 * U * (np.abs(t1) + np.abs(t2) + np.abs(t3)), 0.0)


def norm_apply(x, scale, shift, relu):
    x = _d(x)
    y = x * _d(scale) + _d(shift)
    return (np.maximum(y, 0.0) if relu else y), 3 * U * (np.abs(x * _d(scale)) + np.abs(_d(shift)))


def relu_mask(dy, y):
    """dz = dy where y > 0 else +0 (so y = NaN, -0.0, 0 give 0; a positive denormal passes)"""
    return np.where(np.asarray(y) > 0, np.asarray(dy), np.zeros_like(dy))


# ------------------------------------------------------------------------------------------------------------ pooling
def _windows(x):
    D, H, W, C = x.shape
    Do, Ho, Wo = D // 2, H // 2, W // 2
    return x[:2 * Do, :2 * Ho, :2 * Wo].reshape(Do, 2, Ho, 2, Wo, 2, C).transpose(0, 2, 4, 1, 3, 5, 6).reshape(Do, Ho, Wo, 8, C)


def maxpool2(x):
    """x (D, H, W, C) -> y (D/2, H/2, W/2, C), winners (uint8): the first maximum in scan order z, y, x of the 2 x 2 x 2 window
    (k = 4 dz + 2 dy + dx), a NaN always taking over (ATen's rule: val > max || isnan(val)); floor mode"""
    w = _windows(np.asarray(x))
    m = np.full(w.shape[:3] + w.shape[4:], -np.inf, w.dtype)
    am = np.zeros(m.shape, np.uint8)
    for k in range(8):
        v = w[:, :, :, k]
        with np.errstate(invalid="ignore"):
            up = (v > m) | np.isnan(v)
        m, am = np.where(up, v, m), np.where(up, np.uint8(k), am)
    return m, am


def maxpool2_scatter(dy, arg, shape, add=None):
    """dx (D, H, W, C): dy at the winner of each window, 0 elsewhere, trailing planes of odd sizes 0 (+ add everywhere)"""
    D, H, W = shape
    Do, Ho, Wo, C = dy.shape
    dy = np.asarray(dy)
    one = np.where(np.arange(8)[None, None, None, :, None] == np.asarray(arg)[:, :, :, None, :], dy[:, :, :, None, :],
                   np.zeros((), dy.dtype))
    dx = np.zeros((D, H, W, C), dy.dtype)
    dx[:2 * Do, :2 * Ho, :2 * Wo] = one.reshape(Do, Ho, Wo, 2, 2, 2, C).transpose(0, 3, 1, 4, 2, 5, 6).reshape(2 * Do, 2 * Ho, 2 * Wo, C)
    return dx if add is None else dx + np.asarray(add, dy.dtype)


def to_blocked(x):
    """(D, H, W, C) -> (C / 8, D, H, W, 8): the channel-blocked layout of a gradient hand-off"""
    D, H, W, C = x.shape
    return np.ascontiguousarray(x.reshape(D, H, W, C // 8, 8).transpose(3, 0, 1, 2, 4))


# ------------------------------------------------------------------------------------------ lazy InstanceNorm backward
def instance_stats(z, eps=EPS):
    zf = _d(z).reshape(-1, z.shape[-1])
    mean = zf.mean(0)
    var = ((zf - mean) ** 2).mean(0)
    return mean, 1.0 / np.sqrt(var + eps)


def in_bwd(z, du, pool, eps=EPS):
    """gradient of z (D, H, W, C) through u = [MaxPool3d(2)](ReLU(InstanceNorm(z))) for the gradient du of u, fp64, two-pass
    variance: dz = rstd (g - mean g - zhat mean(g zhat)), g = scatter(du) [zhat > 0]"""
    z, du = _d(z), _d(du)
    mean, rstd = instance_stats(z, eps)
    zhat = (z - mean) * rstd
    g = maxpool2_scatter(du, maxpool2(z)[1], z.shape[:3]) if pool else du
    g = g * (zhat > 0)
    ax = (0, 1, 2)
    return rstd * (g - g.mean(ax) - zhat * (g * zhat).mean(ax))


# ------------------------------------------------------------------------------------------------------------- upcat
def nearest_src(dst, n_in, n_out):
    """ATen's legacy 'nearest' in its own float32 arithmetic: min(floor(dst * (float(n_in) / float(n_out))), n_in - 1)"""
    scale = F32(n_in) / F32(n_out)
    s = np.floor(np.asarray(dst, F32) * scale).astype(np.int64)
    return np.minimum(s, n_in - 1)


def upcat(skip, low):
    """skip (D, H, W, Cs), low (Dl, Hl, Wl, Cl) -> cat(skip, nearest-upsampled low) (D, H, W, Cs + Cl)"""
    D, H, W = skip.shape[:3]
    iz, iy, ix = (nearest_src(np.arange(n), m, n) for n, m in zip((D, H, W), low.shape[:3]))
    return np.concatenate([np.asarray(skip), np.asarray(low)[iz][:, iy][:, :, ix]], -1)


def upcat_bwd(dout, Cs, low_shape):
    """-> dskip (a copy of values), dlow in fp64, and sum|terms| of dlow for its bar 27 u sum|terms|"""
    D, H, W = dout.shape[:3]
    Dl, Hl, Wl = low_shape
    iz, iy, ix = (nearest_src(np.arange(n), m, n) for n, m in zip((D, H, W), low_shape))
    g = _d(dout)[..., Cs:]
    dlow, mag = np.zeros((Dl, Hl, Wl, g.shape[-1])), np.zeros((Dl, Hl, Wl, g.shape[-1]))
    idx = np.ix_(iz, iy, ix)
    np.add.at(dlow, idx, g)
    np.add.at(mag, idx, np.abs(g))
    return np.asarray(dout)[..., :Cs], dlow, mag


# ------------------------------------------------------------------------------------------------------- range scale
def range_scale_property(bound, S, slack=0.0):
    """S is a power of two with bound S in [2^14, 2^15) (S = 1 for a zero or non-finite bound); slack: relative uncertainty of
    `bound` itself where the kernel computes it in fp32"""
    S, bound = float(S), float(bound)
    if not (bound > 0 and np.isfinite(bound)):
        return S == 1.0
    return float(np.log2(S)).is_integer() and 2.0 ** 14 * (1 - slack) <= bound * S < 2.0 ** 15 * (1 + slack)


def ascale_bound(gamma, beta, count, cpg):
    """the guaranteed bound of the normalised tensor as the forward coefficient kernel forms it in fp32"""
    gmax = F32(1) if gamma is None else np.abs(np.asarray(gamma, F32)).max()
    bmax = F32(0) if beta is None else np.abs(np.asarray(beta, F32)).max()
    return float(F32(gmax * np.sqrt(F32(count * cpg))) + bmax)


# --------------------------------------------------------------------------------------- first-order error propagation
class Err:
    """a value with an absolute first-order error bound (module docstring: chains)"""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def __add__(self, o):
        o = Err.of(o)
        return Err(self.v + o.v, self.e + o.e)

    def __neg__(self):
        return Err(-self.v, self.e)

    def __sub__(self, o):
        return self + (-Err.of(o))

    def __mul__(self, o):
        o = Err.of(o)
        return Err(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = Err.of(o)
        return Err(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))

    def rsqrt(self, lo):
        """the argument is known to be >= lo > 0 (the kernels clamp the variance at 0 before eps is added)"""
        return Err(self.v ** -0.5, np.maximum(self.e * 0.5 * self.v ** -1.5, np.maximum(self.v - self.e, lo) ** -0.5 - self.v ** -0.5))

    def sum(self, axis):
        return Err(self.v.sum(axis), self.e.sum(axis))

    def rep(self, k, axis):
        return Err(np.repeat(self.v, k, axis), np.repeat(self.e, k, axis))

    def reshape(self, *s):
        return Err(self.v.reshape(*s), self.e.reshape(*s))

    def r32(self):
        return Err(self.v, self.e + U * np.abs(self.v))


def chain_bars(x, dy, gamma, beta, G, mask=None, eps=EPS):
    """One sample: x, dy (V, C) fp32 through statistics -> forward coefficients -> apply, then statistics of (g, x) ->
    backward coefficients -> apply, g = dy * mask.  Returns a dict name -> Err with .v the fp64 value BY THE KERNELS' FORMULAS
    (ss / m - mean^2) and .e the propagated bound of what the kernels compute around it: rstd (G), y, dx (V, C), dgamma,
    dbeta (C).  The truth of a test is fp64 autograd; |.v - truth| is the fp64 cancellation of the formula, ~1e-16 (mean / std)^2,
    and is added to the bar by the caller."""
    x, dy = _d(x), _d(dy)
    V, C = x.shape
    cpg = C // G
    m = float(V * cpg)
    ga = np.ones(C) if gamma is None else _d(gamma)
    be = np.zeros(C) if beta is None else _d(beta)
    b0, b1 = stats_bars(x)
    s0, s1 = channel_sums(x)
    s, ss = Err(s0, b0).reshape(G, cpg).sum(1), Err(s1, b1).reshape(G, cpg).sum(1)
    mean = s / m
    var = ss / m - mean * mean
    rstd = (var + eps).rsqrt(eps)
    mean32, rstd32 = mean.r32(), rstd.r32()
    scale = (rstd.rep(cpg, 0) * ga).r32()
    shift = (Err(be) - mean.rep(cpg, 0) * rstd.rep(cpg, 0) * ga).r32()
    y = Err(x) * scale + shift
    y = Err(y.v, y.e + 3 * U * (np.abs(x * scale.v) + np.abs(shift.v)))
    g = dy if mask is None else dy * mask
    a0, a1 = channel_sums(g, x)
    e0, e1 = stats_bars(g, x)
    A, B = Err(a0, e0), Err(a1, e1)
    mc, rc = mean32.rep(cpg, 0), rstd32.rep(cpg, 0)
    S1 = (A * ga).reshape(G, cpg).sum(1)
    xt = B - mc * A
    S2 = (rc * xt * ga).reshape(G, cpg).sum(1)
    c1 = (rc * ga).r32()
    c2 = (-(rstd32 * rstd32 * S2) / m).r32().rep(cpg, 0)
    c3 = (-(rstd32 * S1) / m + rstd32 * rstd32 * S2 * mean32 / m).r32().rep(cpg, 0)
    dx = c1 * Err(g) + c2 * Err(x) + c3
    dx = Err(dx.v, dx.e + 3 * U * (np.abs(c1.v * g) + np.abs(c2.v * x) + np.abs(c3.v)))
    return {"mean": mean32, "rstd": rstd32, "y": y, "dx": dx, "dgamma": (rc * xt).r32(), "dbeta": A.r32()}


# --------------------------------------------------------------------------------------------------------- case table
STAT_CLASSES = ("zero_mean", "relu", "offset100", "const", "big_channel", "outlier")
STAT_C = (1, 3, 4, 12, 20, 200, 255, 260, 512, 1024)          # at V = 333: idle threads at 3, 12, 200, 260; rows = 1 from 516
STAT_V = (1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5)      # at C = 3 and 8: the chunk of 64 and the block of 2048
STAT_V_CAP = (512 * 2048 + 3, 4)                              # past the 512-block cap
STAT_SHAPES = tuple((333, c) for c in STAT_C) + tuple((v, c) for c in (3, 8) for v in STAT_V) + (STAT_V_CAP,)
STAT_REFUSED_C = (257, 1028)
COEFF_CG = ((8, 8), (12, 4), (16, 1), (200, 200), (96, 8), (320, 320))      # G > 64, N G > 256 (at N = 3), C > 256
COEFF_COUNTS = (1, 333)
CONST_VALUE = 0.75


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def stat_data(cls, N, V, C, seed=0):
    """(N, V, C) float32 of a data class of the statistics tests"""
    r = np.random.default_rng([_seed(cls), N, V % 100003, C, seed])
    a = r.standard_normal((N, V, C), dtype=F32)
    if cls == "relu":
        a = np.maximum(a, F32(0))
    elif cls == "offset100":
        a = a + F32(100)
    elif cls == "const":
        a[..., 0] = CONST_VALUE
    elif cls == "big_channel":
        a[..., C // 2] *= F32(1e4)
    elif cls == "outlier":
        a[..., C - 1] = 0
        a[:, V // 2, C - 1] = 1e6
    elif cls != "zero_mean":
        raise KeyError(cls)
    return a


def coeff_case(C, G, N, count, affine, seed=0):
    """inputs of the coefficient kernels from data x = 1.5 + randn, dxn = randn: fp64 statistics by the reference"""
    r = np.random.default_rng([C, G, N, count, int(affine), seed, 77])
    x = (1.5 + r.standard_normal((N, count, C))).astype(F32)
    dxn = r.standard_normal((N, count, C)).astype(F32)
    gamma = (1 + 0.5 * r.standard_normal(C)).astype(F32) if affine else None
    beta = (0.3 * r.standard_normal(C)).astype(F32) if affine else None
    stats = np.stack([np.stack(channel_sums(x[n]), -1) for n in range(N)])
    ab = np.stack([np.stack(channel_sums(dxn[n], x[n]), -1) for n in range(N)])
    return {"x": x, "dxn": dxn, "gamma": gamma, "beta": beta, "stats": stats, "ab": ab}


@functools.lru_cache(maxsize=None)
def kink_free(shape, C, seed, quantised=False):
    """(D, H, W, C) float32 with |zhat| >= 1e-3 everywhere (InstanceNorm's standardised value): elements nearer than 2e-3 to
    their channel's mean are pushed out by 0.05 std, repeated until none is left.  quantised: multiples of 0.25 from {-0.25 ..
    0.5}, four values in eight slots, and the maximum of every window placed twice: the winner rule decides the result."""
    r = np.random.default_rng([seed, C, int(quantised)] + list(shape))
    for _ in range(1000 if quantised else 0):   # redrawn until no value sits on its channel's mean (a multiple of 0.25 / V)
        z = (r.integers(-1, 3, size=shape + (C,)) * 0.25).astype(F32)
        w = _windows(z)                         # a copy: write the window maximum into two slots, then put it back
        k = r.integers(0, 8, size=w.shape[:3] + (1, C))
        for kk in (k, (k + r.integers(1, 8, size=k.shape)) % 8):
            np.put_along_axis(w, kk, w.max(3, keepdims=True), 3)
        D, H, W = shape
        z[:2 * (D // 2), :2 * (H // 2), :2 * (W // 2)] = w.reshape(D // 2, H // 2, W // 2, 2, 2, 2, C).transpose(
            0, 3, 1, 4, 2, 5, 6).reshape(2 * (D // 2), 2 * (H // 2), 2 * (W // 2), C)
        mean, rstd = instance_stats(z)
        if (np.abs((z.astype(np.float64) - mean) * rstd) >= 2e-3).all():
            z.setflags(write=False)
            return z
    z = (0.7 + 1.3 * r.standard_normal(shape + (C,))).astype(F32)
    for _ in range(20):
        mean, rstd = instance_stats(z)
        zh = (z.astype(np.float64) - mean) * rstd
        near = np.abs(zh) < 2e-3
        if not near.any():
            break
        z = np.where(near, z + np.where(zh >= 0, 0.05, -0.05) / rstd, z).astype(F32)
    z.setflags(write=False)
    return z


POOL_CLASSES = ("all_equal", "relu", "neg_inf", "all_negative", "nan_first", "nan_middle", "nan_last", "nan_first_last")


def pool_data(cls, shape, C, seed=0):
    """(D, H, W, C) float32 of a class of the pooling tests; every window holds the feature the class is named after"""
    D, H, W = shape
    r = np.random.default_rng([_seed(cls), C, seed] + list(shape))
    x = r.standard_normal(shape + (C,)).astype(F32)
    if cls == "all_equal":
        x = np.broadcast_to(r.standard_normal((D // 2 + 1, 1, H // 2 + 1, 1, W // 2 + 1, 1, C)).astype(F32),
                            (D // 2 + 1, 2, H // 2 + 1, 2, W // 2 + 1, 2, C)).reshape(D + 2 - D % 2, H + 2 - H % 2, W + 2 - W % 2, C)
        x = np.ascontiguousarray(x[:D, :H, :W])
    elif cls == "relu":
        x = np.maximum(x, F32(0))
        x[::2, ::2] = 0                        # at least two zeros per window; the first window all zero
        x[1::2, 1::2, :, ::2] = 0
        x[:2, :2, :2] = 0
    elif cls == "neg_inf":
        x[r.random(x.shape) < 0.6] = -np.inf
        x[:2, :2, :2] = -np.inf                # one window all -inf
    elif cls == "all_negative":
        x = -np.abs(x) - F32(1)
    elif cls.startswith("nan"):
        x = np.round(x * 2) / 2                # ties around the NaN as well
        x = x.astype(F32)
        if cls in ("nan_first", "nan_first_last"):
            x[::2, ::2, ::2] = np.nan
        if cls == "nan_middle":
            x[::2, 1::2, 1::2] = np.nan
        if cls in ("nan_last", "nan_first_last"):
            x[1::2, 1::2, 1::2] = np.nan
    else:
        raise KeyError(cls)
    return x


def nearest_pairs():
    return [(i, o) for i in range(1, 18) for o in range(i, 2 * i + 2)]
