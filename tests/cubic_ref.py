"""fp64 restatement of cubic B-spline resampling (csrc/cubic.hip, ops.cubic_coefficients / ops.cubic_sample), for the conformance
tests of the HIP kernels and, on the CPU, against scipy.ndimage.spline_filter / map_coordinates (order=3, mode="mirror").

Coefficients: per line of length n >= 2, with z = sqrt(3) - 2 and the whole-sample mirror fold (period 2 (n - 1)),
    c+[0] = sum_{k=0}^{2n-3} z^k x[fold(k)] / (1 - z^(2n-2)),   c+[i] = x[i] + z c+[i-1],
    c-[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]),              c-[i] = z (c-[i+1] - c+[i]),       c = 6 c-,
separably along W, H and D -- the FULL initial sum, no truncation; an axis of length 1 is left as it is.

The source coordinate is the trilinear sampler's (tests/sampler_ref.source_coord: fp32, every operation rounded on its own, clipped
to [0, size - 1] with a zero derivative where clipped, NaN to the far border), so the reference picks the kernel's cell and clamp
mask.  Value: i0 = floor(p), t = p - i0 per axis, the sum over the taps i0 - 1 .. i0 + 2 of wz wy wx c[fold(.)].  Grid gradient: the
derivative weights on one axis, times the cotangent, summed over the channels, times the coordinate's multiplier; a voxel with any
NaN coordinate passes none.

Everything after the coordinate takes a dtype: float64 is the reference, float32 is the same code at the kernels' precision -- the
distance between the two is the measure of the tests' tolerances (tolerance()).
"""
import numpy as np

from tests.sampler_ref import source_coord

POLE = np.sqrt(3.0) - 2.0


def fold(i, n):
    """whole-sample mirror of integer indices into [0, n - 1]: -1 -> 1, n -> n - 2, period 2 (n - 1); n = 1: everything -> 0"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i > n - 1, p - i, i)


def _filter_axis(x, axis, dtype):
    n = x.shape[axis]
    if n == 1:
        return x
    x = np.moveaxis(x, axis, 0)
    z, one = dtype(POLE), dtype(1)
    s, zk = np.zeros_like(x[0]), one
    with np.errstate(under="ignore"):
        for k in range(2 * n - 2):
            s = s + zk * x[int(fold(k, n))]
            zk = zk * z
    cp = np.empty_like(x)
    cp[0] = s / (one - zk)
    for i in range(1, n):
        cp[i] = x[i] + z * cp[i - 1]
    cm = np.empty_like(x)
    cm[n - 1] = (z / (z * z - one)) * (cp[n - 1] + z * cp[n - 2])
    for i in range(n - 2, -1, -1):
        cm[i] = z * (cm[i + 1] - cp[i])
    return np.moveaxis(dtype(6) * cm, 0, axis)


def coefficients(x, dtype=np.float64):
    """x (..., D, H, W) -> cubic B-spline coefficients of the same shape, filtered along W, then H, then D"""
    c = np.array(x, dtype=dtype)
    for axis in (-1, -2, -3):
        c = _filter_axis(c, axis, dtype)
    return c


def weights(t, dtype=np.float64):
    """B3 at the taps i0 - 1 .. i0 + 2 for the fraction t"""
    t = np.asarray(t).astype(dtype)
    a = dtype(1) - t
    return [a * a * a / dtype(6),
            (dtype(3) * t * t * t - dtype(6) * t * t + dtype(4)) / dtype(6),
            (dtype(-3) * t * t * t + dtype(3) * t * t + dtype(3) * t + dtype(1)) / dtype(6),
            t * t * t / dtype(6)]


def dweights(t, dtype=np.float64):
    """d(weights)/dt"""
    t = np.asarray(t).astype(dtype)
    a = dtype(1) - t
    return [-(a * a) / dtype(2),
            (dtype(3) * t * t - dtype(4) * t) / dtype(2),
            (dtype(-3) * t * t + dtype(2) * t + dtype(1)) / dtype(2),
            t * t / dtype(2)]


def _axes(grid, shape, dtype):
    """per axis (x, y, z): (the four folded tap indices, weights, derivative weights, multiplier incl. clamp and NaN mask)"""
    D, H, W = shape
    grid = np.asarray(grid)
    live = ~np.isnan(grid).any(-1)
    out = []
    for k, size in ((0, W), (1, H), (2, D)):
        c, m = source_coord(grid[..., k], size)
        i0 = np.floor(c).astype(np.int64)
        t = c - i0                                           # exact: c is an fp32 number
        idx = [fold(i0 - 1 + j, size) for j in range(4)]
        out.append((idx, weights(t, dtype), dweights(t, dtype), (m * live).astype(dtype)))
    return out


def _contract(coef, ax, wx, wy, wz, dtype):
    """sum over the 64 taps of coef * wz wy wx, x innermost, then y, then z -> (N, C, *out)"""
    (xi, _, _, _), (yi, _, _, _), (zi, _, _, _) = ax
    N = coef.shape[0]
    nidx = np.arange(N).reshape((N,) + (1,) * (xi[0].ndim - 1))
    total = None
    for a in range(4):
        plane = None
        for b in range(4):
            row = None
            for k in range(4):
                v = np.moveaxis(coef[nidx, :, zi[a], yi[b], xi[k]], -1, 1) * wx[k][:, None]
                row = v if row is None else row + v
            row = row * wy[b][:, None]
            plane = row if plane is None else plane + row
        plane = plane * wz[a][:, None]
        total = plane if total is None else total + plane
    return total


def sample(coef, grid, dtype=np.float64):
    """the spline of coef (N, C, D, H, W) at grid (N, Do, Ho, Wo, 3) -> (N, C, Do, Ho, Wo)"""
    coef = np.asarray(coef).astype(dtype)
    ax = _axes(grid, coef.shape[2:], dtype)
    return _contract(coef, ax, ax[0][1], ax[1][1], ax[2][1], dtype)


def sample_bwd_grid(coef, grid, gout, dtype=np.float64):
    """d(sum gout * sample)/d(grid) -> (N, Do, Ho, Wo, 3)"""
    coef = np.asarray(coef).astype(dtype)
    gout = np.asarray(gout).astype(dtype)
    ax = _axes(grid, coef.shape[2:], dtype)
    (_, wx, dwx, mx), (_, wy, dwy, my), (_, wz, dwz, mz) = ax
    gx = (_contract(coef, ax, dwx, wy, wz, dtype) * gout).sum(1)
    gy = (_contract(coef, ax, wx, dwy, wz, dtype) * gout).sum(1)
    gz = (_contract(coef, ax, wx, wy, dwz, dtype) * gout).sum(1)
    return np.stack([gx * mx, gy * my, gz * mz], -1)


def resample(x, grid, dtype=np.float64):
    """grid_sample3d(x, grid, "cubic"): sample(coefficients(x), grid)"""
    return sample(coefficients(x, dtype), grid, dtype)


def resample_bwd_grid(x, grid, gout, dtype=np.float64):
    return sample_bwd_grid(coefficients(x, dtype), grid, gout, dtype)


def tolerance(f, *args):
    """(f in float64, the bound of a kernel's distance from it): 4 times the largest distance of f in float32 from f in float64 on
    the same inputs.  The 4 covers another association, fused multiply-adds and the truncated start of the recursion."""
    ref = f(*args, dtype=np.float64)
    low = f(*args, dtype=np.float32)
    assert low.dtype == np.float32
    d = np.abs(low.astype(np.float64) - ref)
    return ref, 4.0 * (float(d.max()) if d.size else 0.0)
