"""fp64 restatement of Gaussian smoothing (csrc/gauss.hip, ops.gaussian_smooth / ops.gaussian_kernel1d) and of its transpose, for the
conformance tests of the HIP kernels and, on the CPU, against scipy.ndimage.gaussian_filter(mode="nearest").

Per axis with sigma > 0:  R = int(truncate sigma + 0.5),  w[k] = exp(-k^2 / 2 sigma^2) / sum_k exp(-k^2 / 2 sigma^2), k = -R .. R,
    out[i] = sum_k w[k] x[clamp(i + k, 0, n - 1)]                      (the replicated border),
along W, then H, then D; an axis with R = 0 is left as it is.  Transpose, along D, then H, then W:
    0 < j < n - 1:  dx[j] = sum_k w[k] g[j - k] over the k with 0 <= j - k <= n - 1,
    dx[0] = sum_i g[i] T[i],  dx[n - 1] = sum_i g[n - 1 - i] T[i],  T[i] = sum_{k >= i} w[k],  i = 0 .. min(R, n - 1);
    n = 1 is its own transpose.
The weights and tail sums are always computed in fp64.  dtype=float64 is the reference; dtype=float32 is the same code at the
kernels' precision (weights and tails rounded to fp32 once, fp32 sums) -- the distance between the two is the measure of the
tests' tolerances (tolerance()).

estimate() is tests/mi_ref.estimate with the smoothed pyramid; noisy_pair() the pair of the noise-recovery experiment.
"""
import numpy as np

TRUNCATE = 4.0


def radius(sigma, truncate=TRUNCATE):
    return int(float(truncate) * float(sigma) + 0.5)


def kernel1d(sigma, truncate=TRUNCATE):
    """the 2 R + 1 weights, fp64"""
    R = radius(sigma, truncate)
    if R == 0:
        return np.ones(1)
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 * k * k / (float(sigma) * float(sigma)))
    return w / w.sum()


def sigmas3(sigma):
    return (float(sigma),) * 3 if np.isscalar(sigma) else tuple(float(s) for s in sigma)


def _fwd_axis(x, axis, w, dtype):
    R = (len(w) - 1) // 2
    n = x.shape[axis]
    x = np.moveaxis(x, axis, 0)
    w = w.astype(dtype)
    idx = np.arange(n)
    out = np.zeros_like(x)
    for k in range(-R, R + 1):
        out = out + w[k + R] * x[np.clip(idx + k, 0, n - 1)]
    return np.moveaxis(out, 0, axis)


def _bwd_axis(g, axis, w, dtype):
    R = (len(w) - 1) // 2
    n = g.shape[axis]
    if n == 1:
        return _fwd_axis(g, axis, w, dtype)
    g = np.moveaxis(g, axis, 0)
    tails = np.array([w[R + i:].sum() for i in range(R + 1)]).astype(dtype)      # fp64 sums, rounded once
    w = w.astype(dtype)
    dx = np.zeros_like(g)
    for k in range(-R, R + 1):
        lo, hi = max(1, k), min(n - 2, n - 1 + k)                                # interior j with 0 <= j - k <= n - 1
        if lo <= hi:
            dx[lo:hi + 1] = dx[lo:hi + 1] + w[k + R] * g[lo - k:hi + 1 - k]
    for i in range(min(R, n - 1) + 1):
        dx[0] = dx[0] + tails[i] * g[i]
        dx[n - 1] = dx[n - 1] + tails[i] * g[n - 1 - i]
    return np.moveaxis(dx, 0, axis)


def smooth(x, sigma, truncate=TRUNCATE, dtype=np.float64):
    """x (..., D, H, W) smoothed along W, then H, then D; sigma a number or (z, y, x)"""
    out = np.array(x, dtype=dtype)
    sz, sy, sx = sigmas3(sigma)
    for axis, s in ((-1, sx), (-2, sy), (-3, sz)):
        if radius(s, truncate) > 0:
            out = _fwd_axis(out, axis, kernel1d(s, truncate), dtype)
    return out


def smooth_bwd(g, sigma, truncate=TRUNCATE, dtype=np.float64):
    """the transpose of smooth applied to g (..., D, H, W): along D, then H, then W"""
    out = np.array(g, dtype=dtype)
    sz, sy, sx = sigmas3(sigma)
    for axis, s in ((-3, sz), (-2, sy), (-1, sx)):
        if radius(s, truncate) > 0:
            out = _bwd_axis(out, axis, kernel1d(s, truncate), dtype)
    return out


def tolerance(f, *args):
    """(f in float64, the bound of a kernel's distance from it): 4 times the largest distance of f in float32 from f in float64 on
    the same inputs (tests/cubic_ref.tolerance).  The 4 covers another association of the same sums and fused multiply-adds."""
    ref = f(*args, dtype=np.float64)
    low = f(*args, dtype=np.float32)
    assert low.dtype == np.float32
    d = np.abs(low.astype(np.float64) - ref)
    return ref, 4.0 * (float(d.max()) if d.size else 0.0)


# ---- the noise-recovery experiment ---------------------------------------------------------------------------------------
NOISE_SEED, NOISE_LEVEL, NOISE_SIZE = 100, 0.3, 64
NOISE_SHRINK, NOISE_SIGMAS = (4, 2), (2.0, 1.0)
# estimate()'s fp64 answers on noisy_pair() with this schedule (30 iterations, lr 0.25), (z, y, x) voxels: 3.743 and 0.593 from the
# true shift (2.3, -1.6, 0.8).  tests/test_gauss_cpu.py recomputes them; the GPU test reports its distance from them.
NOISE_ANSWERS = {"as today": (-0.6585, -0.9755, 3.0058), "smoothed": (2.7235, -1.2398, 1.0059)}


def noisy_pair(size=NOISE_SIZE, seed=NOISE_SEED, noise=NOISE_LEVEL):
    """mi_ref.recovery_pair(size) plus voxel noise, fp64: one generator, the fixed image's noise drawn first"""
    import torch
    from tests import mi_ref
    f, m = (v.double() for v in mi_ref.recovery_pair(size))
    g = torch.Generator().manual_seed(seed)
    f = f + noise * torch.randn(f.shape, generator=g, dtype=torch.float64)
    m = m + noise * torch.randn(m.shape, generator=g, dtype=torch.float64)
    return f, m


def estimate(fixed, moving, bins=32, shrink=(4, 2, 1), iters=30, lr=0.25, smoothing=None):
    """tests/mi_ref.estimate (the schedule of io.estimate_translation on the CPU, in the inputs' dtype) with the smoothed pyramid:
    smoothing[l] is the sigma applied at the full size before level l is resized (None: no smoothing).  Returns (t, the t after
    every level that ran)."""
    import torch
    import torch.nn.functional as F
    from tests import mi_ref
    fixed, moving = fixed.detach(), moving.detach()
    dims = tuple(fixed.shape[2:])
    t = mi_ref.centroid(moving) - mi_ref.centroid(fixed)
    trace = []
    for lvl, sh in enumerate(shrink):
        ldims = tuple(n // int(sh) for n in dims)
        if min(ldims) < 16:
            continue
        f_l, m_l = fixed, moving
        if smoothing is not None and max(sigmas3(smoothing[lvl])) > 0:
            f_l, m_l = (torch.from_numpy(smooth(v.numpy(), smoothing[lvl], dtype=v.numpy().dtype.type)) for v in (f_l, m_l))
        if ldims != dims:
            f_l = F.interpolate(f_l, size=ldims, mode="trilinear", align_corners=False)
            m_l = F.interpolate(m_l, size=ldims, mode="trilinear", align_corners=False)
        ratio = torch.tensor([n / l for n, l in zip(dims, ldims)], dtype=fixed.dtype)
        t_l = (t / ratio).requires_grad_(True)
        opt = torch.optim.Adam([t_l], lr=lr)
        for _ in range(iters):
            opt.zero_grad(set_to_none=True)
            loss = -mi_ref.mutual_information(mi_ref.translate(m_l, t_l), f_l, bins).sum()
            loss.backward()
            opt.step()
        t = t_l.detach() * ratio
        trace.append(t.clone())
    return t, trace
