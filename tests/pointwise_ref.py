"""fp64 numpy restatement of csrc/pointwise.hip (the 1x1x1 head convolution as fp32-MFMA GEMMs: forward, data gradient, weight /
bias gradient) in the kernels' own layouts, the bars its conformance tests hold the kernels to, the two data generators and the
case table.  x is (N, V, Cin), w (Cout, Cin), b (Cout) or None, y and dy (N, Cout, V):

    fwd    y[n, co, v]  = b[co] + sum_ci w[co, ci] x[n, v, ci]              K = Cin
    dgrad  dx[n, v, ci] = sum_co dy[n, co, v] w[co, ci]                     K = Cout
    wgrad  dw[co, ci]   = sum_{n, v} dy[n, co, v] x[n, v, ci]               K = N V
           db[co]       = sum_{n, v} dy[n, co, v]                           K = N V

Every sum starts from +0 (the accumulators are cleared), so no result is -0.0; the restatement adds +0.0 to say the same.

u = 2**-24 (one fp32 rounding).  Bars, none from a run of the kernels:

  dot product  A K-term fp32 dot product summed in any order, the products rounded on their own or fused, followed by a bias add
               and the store: a term passes through its product's rounding, at most K - 1 additions and the bias add, the bias
               through at most K additions, the store of an fp32 accumulator rounds nothing.  With S = sum_k |a_k b_k| (+ |b|,
               the bias counted as one more term) the error is at most ((1 + u)^(K + 1) - 1) S <= (K + 1) u / (1 - (K + 1) u) S,
               and that is <= (K + 3) u S as long as (K + 1)(K + 3) u <= 2, which holds for K <= 4096:
                   bar = (K + 3) u S                                        (fwd_bar, dgrad_bar, wgrad_bar)
               The head's K are Cin <= 200 and Cout <= 257 here.  For the weight gradient the plain K = N V of the table's
               largest row (20001) is past that; (K + 3) u S is then the first-order bound only.  The tests do not use it there:
  one slab     the weight-gradient kernel cuts the N V voxels into `nslab` slabs of equal length L (the last one shorter), adds
               one slab in one fp32 chain (MFMA accumulators; the bias gradient: one fp32 sum per lane, two lanes joined by one
               more addition), and adds the slab partials in double, rounded once on the store.  nslab slabs of length L cover N V
               voxels with the last one not empty, so (nslab - 1) L < N V, and a chain holds at most
                   K1 = min(N V, floor((N V - 1) / (nslab - 1)))            (nslab > 1;  K1 = N V for one slab)
               terms that are not exact zeros.  Per slab s the error is at most ((1 + u)^K1 - 1) S_s (product, K1 - 1 additions),
               the double sum of the partials adds nslab 2^-53 S at most (< u S / 2 up to 2^28 slabs), the store u |dw| <= u S.
               Summed over the slabs: ((1 + u)^K1 - 1 + 3 u / 2) S <= (K1 + 3) u S as long as K1 (K1 + 3 / 2) u <= 3 / 2, which
               holds for K1 <= 4096 too.  wgrad_bar(dy, x, nslab) is that bar with nslab THE LIBRARY'S OWN ANSWER (workspace
               bytes / ((Cout Cin + Cout) 4)), and asserts K1 <= 4096.
  accumulate   out = dw0 + fl(dw): one more fp32 addition, + u |dw0 + dw|      (the `acc0` argument of wgrad_bar)

Generators.  exact_case: integer-valued float32 in [-8, 8]; every product and every partial sum of every kernel is an integer
below 2^24 in magnitude (asserted: max sum|a b|, the bias and the pre-filled dw0 / db0 included, < 2^24), so fp32 arithmetic in
any order is exact and the kernels must return the float32 cast of the fp64 result bit for bit -- a dropped, duplicated or
misplaced term at any K shows.  real_case: x[.., ci] = +-2^s(ci) m, w[co, ci] = +-2^(t(co) - s(ci)) m, dy[.., co, ..] = +-2^-t(co) m,
b[co] = +-2^t(co) m with m uniform in [1, 2), random signs, s a permutation of an even spread over [-6, 6] (2^12 between the
channels of x), t one over [-3, 3]: all magnitudes lie in [2^-9, 2^10) (asserted within [2^-10, 2^10]: nothing is subnormal, no
product leaves [2^-20, 2^20]), and the scales cancel in every CORRECT pairing only -- the K terms of one output element lie within
a factor 4 of each other, so one missing term moves it by at least S / (4 K), which is 2^22 / ((K + 1)(K + 3)) bars (the bias one
more term): 102 at K = 200, 62 at K = 257; a term paired with a neighbouring channel is off by the ratio of two scales.
"""
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24
K_RIGOROUS = 4096                      # (K + 1)(K + 3) u <= 2 and K (K + 3 / 2) u <= 3 / 2


def _d(a):
    return None if a is None else np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------------- restatement
def fwd(x, w, b=None):
    """x (N, V, Cin), w (Cout, Cin), b (Cout) | None -> y (N, Cout, V), fp64"""
    x, w, b = _d(x), _d(w), _d(b)
    y = np.matmul(w[None], x.transpose(0, 2, 1))
    return (y if b is None else y + b[None, :, None]) + 0.0


def fwd_bar(x, w, b=None):
    x, w, b = _d(x), _d(w), _d(b)
    S = np.matmul(np.abs(w)[None], np.abs(x).transpose(0, 2, 1))
    if b is not None:
        S = S + np.abs(b)[None, :, None]
    return (w.shape[1] + 3) * U * S


def dgrad(dy, w):
    """dy (N, Cout, V), w (Cout, Cin) -> dx (N, V, Cin), fp64"""
    dy, w = _d(dy), _d(w)
    return np.matmul(dy.transpose(0, 2, 1), w[None]) + 0.0


def dgrad_bar(dy, w):
    dy, w = _d(dy), _d(w)
    return (w.shape[0] + 3) * U * np.matmul(np.abs(dy).transpose(0, 2, 1), np.abs(w)[None])


def _flat(dy, x):
    dy, x = _d(dy), _d(x)
    N, Cout, V = dy.shape
    return dy.transpose(1, 0, 2).reshape(Cout, N * V), x.reshape(N * V, x.shape[2])


def wgrad(dy, x):
    """dy (N, Cout, V), x (N, V, Cin) -> dw (Cout, Cin), db (Cout), fp64"""
    d, xf = _flat(dy, x)
    return d @ xf + 0.0, d.sum(1) + 0.0


def wgrad_terms(N, V, nslab=None):
    """the K of the weight-gradient bars: N V, or with the library's slab count the longest fp32 chain (module docstring)"""
    tot = N * V
    if nslab is None or nslab <= 1:
        return tot
    return min(tot, (tot - 1) // (nslab - 1))


def wgrad_bar(dy, x, nslab=None, acc0=None):
    """-> bar of dw, bar of db.  nslab: the library's own slab count (None: the plain K = N V); acc0 = (dw0, db0 | None) for
    accumulate = 1"""
    d, xf = _flat(dy, x)
    K = wgrad_terms(dy.shape[0], dy.shape[2], nslab)
    assert nslab is None or K <= K_RIGOROUS, (K, nslab)
    bw, bb = (K + 3) * U * (np.abs(d) @ np.abs(xf)), (K + 3) * U * np.abs(d).sum(1)
    if acc0 is not None:
        dw, db = wgrad(dy, x)
        bw = bw + U * np.abs(_d(acc0[0]) + dw)
        if acc0[1] is not None:
            bb = bb + U * np.abs(_d(acc0[1]) + db)
    return bw, bb


def worst_sums(c):
    """largest sum of |products| (bias and pre-filled gradients included) over the three kernels of a case"""
    x, w, b, dy = (np.abs(_d(c[k])) for k in ("x", "w", "b", "dy"))
    d, xf = _flat(dy, x)
    return max(float((np.matmul(w[None], x.transpose(0, 2, 1)) + b[None, :, None]).max()),
               float(np.matmul(dy.transpose(0, 2, 1), w[None]).max()),
               float((d @ xf + np.abs(_d(c["dw0"]))).max()), float((d.sum(1) + np.abs(_d(c["db0"]))).max()))


# --------------------------------------------------------------------------------------------------------- generators
def _freeze(c):
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def exact_case(N, V, Cin, Cout, seed=0):
    """integer-valued float32 in [-8, 8]: x, w, b, dy and the pre-filled dw0, db0 of the accumulate test"""
    r = np.random.default_rng([N, V, Cin, Cout, seed, 1])
    i = lambda *s: r.integers(-8, 9, size=s).astype(F32)                                                  # noqa: E731
    c = {"x": i(N, V, Cin), "w": i(Cout, Cin), "b": i(Cout), "dy": i(N, Cout, V), "dw0": i(Cout, Cin), "db0": i(Cout)}
    assert worst_sums(c) < 2.0 ** 24, (N, V, Cin, Cout)
    return _freeze(c)


def _spread(r, n, half):
    return r.permutation(np.linspace(-half, half, n) if n > 1 else np.zeros(1))


@functools.lru_cache(maxsize=None)
def real_case(N, V, Cin, Cout, seed=0):
    """float32 with compensating per-channel scales (module docstring): x, w, b, dy, dw0, db0"""
    r = np.random.default_rng([N, V, Cin, Cout, seed, 2])
    s, t = _spread(r, Cin, 6.0), _spread(r, Cout, 3.0)
    m = lambda *sh: r.uniform(1.0, 2.0, size=sh) * r.choice([-1.0, 1.0], size=sh)                           # noqa: E731
    c = {"x": m(N, V, Cin) * 2.0 ** s, "w": m(Cout, Cin) * 2.0 ** (t[:, None] - s[None, :]), "b": m(Cout) * 2.0 ** t,
         "dy": m(N, Cout, V) * 2.0 ** -t[None, :, None], "dw0": m(Cout, Cin) * 2.0 ** (s[None, :] - t[:, None]),
         "db0": m(Cout) * 2.0 ** -t}
    c = {k: v.astype(F32) for k, v in c.items()}
    for k, v in c.items():
        a = np.abs(v)
        assert 2.0 ** -10 <= a.min() and a.max() <= 2.0 ** 10, (k, a.min(), a.max())
    return _freeze(c)


def case(arm, row):
    return {"exact": exact_case, "real": real_case}[arm](*row)


def drop_term(c, n, v, ci, co):
    """what a kernel that leaves out the one product of (n, v, ci, co) would return: y, dx, dw (fp64)"""
    x, w, dy = _d(c["x"]), _d(c["w"]), _d(c["dy"])
    y, dx, dw = fwd(x, w, c["b"]), dgrad(dy, w), wgrad(dy, x)[0]
    y[n, co, v] -= w[co, ci] * x[n, v, ci]
    dx[n, v, ci] -= dy[n, co, v] * w[co, ci]
    dw[co, ci] -= dy[n, co, v] * x[n, v, ci]
    return y, dx, dw


# --------------------------------------------------------------------------------------------------------- case table
# (N, V, Cin, Cout).  The kernels' own sizes: 128-voxel workgroup tiles and 32-voxel wave tiles (forward), 256 / 64 / 32 voxels
# (data gradient), 64-voxel chunks of the flat N V axis in slabs (weight gradient); 64-channel LDS chunks of Cin (forward), 32-
# wide MFMA tiles of Cin in pairs (NT = 2 above 32 channels; launches of 64 channels for the weight gradient, the last one with
# NT = 1 when at most 32 are left); Cout in 32-wide tiles and groups of 128; K pairs ((k + 1) >> 1) of Cin, Cout and voxels.
CASES = (
    (1, 1, 1, 1),            # everything is one lane
    (2, 31, 3, 31),          # V < 32, odd K pair loops both ways
    (1, 32, 31, 32),         # one full wave tile
    (2, 33, 32, 33),         # NT = 1 at its largest Cin; one voxel and one channel past a tile
    (1, 127, 33, 127),       # dgrad NT = 2 with a second tile one lane wide; odd Cout with Cin > 32
    (2, 128, 63, 128),       # one full workgroup tile, one full Cout group
    (1, 129, 64, 129),       # one LDS chunk at its largest; a second Cout group one row high, x not restaged
    (2, 255, 65, 1),         # two chunks (the second one channel), wgrad tail launch with NT = 1, dgrad cig = 2; Cout = 1
    (1, 256, 96, 257),       # Cin > 64 with three Cout groups: restaged per group
    (2, 257, 127, 31),       # one voxel past the data gradient's 256
    (1, 300, 128, 129),      # two full chunks, two full wgrad launches
    (2, 300, 129, 33),       # a third chunk / third ci0 launch (NT = 1), dgrad cig = 3; N V = 600 not a multiple of 64
    (1, 33, 200, 257),       # four chunks x three groups
    (3, 21, 65, 127),        # N V = 63 < 64: one partial chunk spanning three samples
    (3, 6667, 65, 31),       # chunks straddle samples; many slabs, the last one ragged (x is 5.2 MB)
    (3, 129, 1, 128),        # Cin = 1 under a full Cout group
    (1, 255, 3, 257),        # thin K under three Cout groups
    (2, 1, 129, 32),         # V = 1 with the widest chunking
    (3, 257, 64, 1),         # Cout = 1 at a full chunk
    (1, 31, 200, 129),       # V < 32 with Cin > 64 and Cout > 128
)
REQUIRED = {"Cin": (1, 3, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 200), "Cout": (1, 31, 32, 33, 127, 128, 129, 257),
            "V": (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300), "N": (1, 2, 3)}
REQUIRED_ROWS = {
    "Cin > 64 with Cout > 128": lambda N, V, Cin, Cout: Cin > 64 and Cout > 128,
    "Cin = 65": lambda N, V, Cin, Cout: Cin == 65,
    "Cin = 129": lambda N, V, Cin, Cout: Cin == 129,
    "Cin = 33": lambda N, V, Cin, Cout: Cin == 33,
    "odd Cout with Cin > 32": lambda N, V, Cin, Cout: Cout % 2 == 1 and Cin > 32,
    "N = 3, V = 21": lambda N, V, Cin, Cout: (N, V) == (3, 21),
    "N = 3, V = 6667": lambda N, V, Cin, Cout: (N, V) == (3, 6667),
}
AUTOGRAD_ROWS = ((2, 300, 129, 33), (1, 256, 96, 257), (3, 21, 65, 127))
CONTAINMENT_ROW = (2, 300, 129, 33)     # V = 2 x 128 + 44 = 256 + 44, Cout = 32 + 1, Cin = 2 x 64 + 1: every last index is ragged


def ids(rows=CASES):
    return [f"N{n}-V{v}-Cin{ci}-Cout{co}" for n, v, ci, co in rows]
