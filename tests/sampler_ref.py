"""fp64 restatement of the 3-D grid sampler (F.grid_sample, padding_mode="border", align_corners=False) and of the losses that
follow it, for conformance tests of the HIP sampler kernels at lattice points, clamp borders and non-finite coordinates.

The source coordinate is computed exactly as ATen's CPU grid_sampler_3d computes it: in fp32, every operation rounded on its
own -- ((g + 1) * size - 1) / 2 -- then clipped by clip_coordinates_set_grad (<= 0: 0, >= size - 1: size - 1, both with a zero
derivative).  So the reference picks ATen's cell even where one ulp of the coordinate moves floor() to the neighbouring
cell.  Everything after the coordinate (floor and fraction, the trilinear blend, the gradients, nearest's half-to-even
rounding, the loss sums) is fp64.

NaN follows ATen's CPU kernels too.  The forward takes a NaN coordinate as the far border (clip_coordinates is
min(size - 1, max(v, 0))), so the voxel gets the value of the last voxel along that axis.  The backward finds no corner of
such a voxel inside the volume, so the voxel passes no gradient at all: zero for all three grid components and nothing
to the input.
"""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32


def source_coord(g, size):
    """normalised fp32 coordinates -> (clipped source coordinate as float64, d(coord)/d(g) incl. the clamp mask)"""
    g = np.asarray(g, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = ((g + F32(1)) * F32(size) - F32(1)) / F32(2)
    hi = F32(size - 1)
    low = v <= 0
    high = ~low & ~(v < hi)                       # v >= hi, and NaN
    c = np.where(low, F32(0), np.where(high, hi, v)).astype(np.float64)
    mult = np.where(low | high, 0.0, size / 2.0)
    return c, mult


def _axes(grid, shape):
    D, H, W = shape
    out = []
    for k, size in ((0, W), (1, H), (2, D)):
        c, m = source_coord(grid[..., k], size)
        i0 = np.floor(c).astype(np.int64)
        f = c - i0
        i1 = np.minimum(i0 + 1, size - 1)
        ok1 = (i0 + 1 < size).astype(np.float64)   # the +1 corner past the far border contributes 0 (its weight is 0 there)
        out.append((i0, i1, f, ok1, m))
    return out


def _corners(x, grid):
    """per corner (dx, dy, dz) in {0,1}^3: its value (N, C, *out), its x/y/z weight factors (N, *out) and the weights"""
    x = np.asarray(x, dtype=np.float64)
    N, C = x.shape[:2]
    (ix0, ix1, fx, okx, mx), (iy0, iy1, fy, oky, my), (iz0, iz1, fz, okz, mz) = _axes(np.asarray(grid), x.shape[2:])
    live = ~np.isnan(np.asarray(grid)).any(-1)            # a voxel with a NaN coordinate passes no gradient (ATen's backward)
    mx, my, mz = mx * live, my * live, mz * live
    nidx = np.arange(N).reshape((N,) + (1,) * (grid.ndim - 2))
    res = {}
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi, zi = (ix1 if dx else ix0), (iy1 if dy else iy0), (iz1 if dz else iz0)
                ok = (okx if dx else 1.0) * (oky if dy else 1.0) * (okz if dz else 1.0) * np.ones_like(fx)
                val = np.moveaxis(x[nidx, :, zi, yi, xi], -1, 1) * ok[:, None]          # (N, C, *out)
                wx = fx if dx else 1.0 - fx
                wy = fy if dy else 1.0 - fy
                wz = fz if dz else 1.0 - fz
                res[(dx, dy, dz)] = (val, wx, wy, wz, (xi, yi, zi), ok * live)
    return res, (mx, my, mz)


def grid_sample(x, grid):
    """bilinear forward, float64 (N, C, *out)"""
    res, _ = _corners(x, grid)
    return sum(val * (wx * wy * wz)[:, None] for val, wx, wy, wz, _, _ in res.values())


def grid_sample_nearest(x, grid):
    """nearest forward: nearbyint (half to even) of the clipped fp32 coordinate"""
    x = np.asarray(x)
    D, H, W = x.shape[2:]
    idx = [np.rint(source_coord(grid[..., k], s)[0]).astype(np.int64) for k, s in ((0, W), (1, H), (2, D))]
    nidx = np.arange(x.shape[0]).reshape((x.shape[0],) + (1,) * (grid.ndim - 2))
    return np.moveaxis(x[nidx, :, idx[2], idx[1], idx[0]], -1, 1)


def grid_sample_bwd_grid(x, grid, gout):
    """d(sum gout * out)/d(grid), float64 (N, *out, 3)"""
    res, (mx, my, mz) = _corners(x, grid)
    gout = np.asarray(gout, dtype=np.float64)
    gx = gy = gz = 0.0
    for (dx, dy, dz), (val, wx, wy, wz, _, _) in res.items():
        s = (val * gout).sum(1)                                                       # (N, *out)
        gx = gx + s * ((1.0 if dx else -1.0) * wy * wz)
        gy = gy + s * ((1.0 if dy else -1.0) * wx * wz)
        gz = gz + s * ((1.0 if dz else -1.0) * wx * wy)
    return np.stack([gx * mx, gy * my, gz * mz], -1)


def grid_sample_bwd_input(x_shape, grid, gout, absolute=False):
    """d(sum gout * out)/d(x), float64 (N, C, D, H, W); absolute=True scatters |gout| * weights (the size of the sum a
    kernel's atomics add up: the tolerance scale of the input gradient)"""
    N, C, D, H, W = x_shape
    gout = np.asarray(gout, dtype=np.float64)
    if absolute:
        gout = np.abs(gout)
    dx = np.zeros((N, C, D * H * W))
    res, _ = _corners(np.zeros((N, 1, D, H, W)), grid)
    for _, wx, wy, wz, (xi, yi, zi), ok in res.values():
        flat = ((zi * H + yi) * W + xi).reshape(N, -1)
        w = (wx * wy * wz * ok).reshape(N, -1)
        for n in range(N):
            for c in range(C):
                np.add.at(dx[n, c], flat[n], w[n] * gout[n, c].reshape(-1))
    return dx.reshape(N, C, D, H, W)


def mse(pred, fixed):
    """(mean squared error, its cotangent with respect to pred)"""
    d = np.asarray(pred, np.float64) - np.asarray(fixed, np.float64)
    return float((d * d).mean()), 2.0 * d / d.size


def dice_rows(pred, target, g=None):
    """rows 1 - (2 sum t p + 1) / (sum p^2 + sum t^2 + 1) over (N, C); with g (N, C): also d(sum g * rows)/d(pred)"""
    p = np.asarray(pred, np.float64)
    t = np.asarray(target, np.float64)
    ax = tuple(range(2, p.ndim))
    num = 2.0 * (t * p).sum(ax) + 1.0
    den = (p * p).sum(ax) + (t * t).sum(ax) + 1.0
    rows = 1.0 - num / den
    if g is None:
        return rows
    g = np.asarray(g, np.float64)
    ca, cb = -2.0 * g / den, 2.0 * g * num / (den * den)
    ex = (slice(None), slice(None)) + (None,) * len(ax)
    return rows, ca[ex] * t + cb[ex] * p


def dice_cot_scale(pred, target, g):
    """|ca t| + |cb p| of the Dice cotangent ca t + cb p: its two terms cancel where pred == target, so this (not the
    cotangent) is the tolerance scale of a Dice grid gradient"""
    p = np.asarray(pred, np.float64)
    t = np.asarray(target, np.float64)
    ax = tuple(range(2, p.ndim))
    num = 2.0 * (t * p).sum(ax) + 1.0
    den = (p * p).sum(ax) + (t * t).sum(ax) + 1.0
    g = np.abs(np.asarray(g, np.float64))
    ex = (slice(None), slice(None)) + (None,) * len(ax)
    return (2.0 * g / den)[ex] * np.abs(t) + (2.0 * g * np.abs(num) / (den * den))[ex] * np.abs(p)


# ------------------------------------------------------------------------------------------------------------ tolerances
def grid_grad_bar(x, gout, shape):
    """per-axis bar of a grid gradient: 1e-5 * C * (size / 2) * max|x| * max|gout|, (x, y, z) order.  C because the gradient
    sums over the channels; a gradient that took the neighbouring cell's difference, or a flipped clamp mask, is off by
    about (size / 2) * max|x| * |gout| -- far above this bar."""
    C = np.asarray(x).shape[1]
    s = 1e-5 * C * float(np.abs(x).max()) * float(np.abs(gout).max())
    D, H, W = shape
    return np.array([s * W / 2.0, s * H / 2.0, s * D / 2.0])


def assert_grid_grad(got, ref, x, gout, what=""):
    """gout: the cotangent of the warped tensor, or an array of the same shape that bounds its terms"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bar = grid_grad_bar(x, gout, np.asarray(x).shape[2:])
    err = np.abs(got - ref).reshape(-1, 3).max(0) if got.size else np.zeros(3)
    assert np.isfinite(got).all() and (err <= bar).all(), f"{what}: grid gradient error per axis {err} > bar {bar}"


def assert_fwd(got, ref, x, what=""):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    bar = 1e-6 * float(np.abs(x).max())
    assert err <= bar, f"{what}: forward error {err:.3e} > {bar:.3e}"


# ------------------------------------------------------------------------------------------------------------ grids
def identity(N, out_shape):
    """F.affine_grid of the identity (align_corners=False): the grid whose source coordinates are the voxel centres when the
    output has the input's shape; fp32 as the oracle builds it"""
    D, H, W = out_shape
    theta = torch.eye(3, 4).expand(N, 3, 4)
    return F.affine_grid(theta, (N, 1, D, H, W), align_corners=False).numpy()


def shift(grid, in_shape, voxels):
    """identity + an integer number of voxels along each axis (x, y, z), added in fp32"""
    D, H, W = in_shape
    out = grid.copy()
    for k, (s, size) in enumerate(zip(voxels, (W, H, D))):
        out[..., k] = out[..., k] + F32(2.0 * s / size)
    return out


def border_points(size):
    """normalised coordinates of the first and last voxel centre of an axis of `size` voxels and +-1 ulp around them (fp32)"""
    first, last = F32(1.0 / size - 1.0), F32(1.0 - 1.0 / size)
    pts = []
    for p in (first, last):
        pts += [np.nextafter(p, F32(-2)), p, np.nextafter(p, F32(2))]
    return np.array(pts, dtype=F32)


def border_grid(N, in_shape, out_shape, seed):
    """a grid whose every coordinate is one of the border points of its axis (or an interior lattice point), so every
    output voxel sits on or next to a clamp boundary"""
    D, H, W = in_shape
    rng = np.random.default_rng(seed)
    g = np.empty((N,) + tuple(out_shape) + (3,), F32)
    for k, size in enumerate((W, H, D)):
        pts = np.concatenate([border_points(size), identity(1, (1, 1, size))[0, 0, 0, :, 0]])
        g[..., k] = rng.choice(pts, size=g.shape[:-1])
    return g


def ref_grid_sample_cpu(x, grid, mode="bilinear"):
    """F.grid_sample on the CPU (the pinned oracle's call)"""
    return F.grid_sample(torch.as_tensor(x), torch.as_tensor(grid), mode=mode, padding_mode="border", align_corners=False)


def steep_affine(N, out_shape, seed):
    """a strong zoom-out with shear and rotation: neighbouring output voxels sample source points several voxels apart"""
    rng = np.random.default_rng(seed)
    theta = torch.tensor(np.eye(3, 4) * 2.5 + rng.normal(0, 0.8, (N, 3, 4)), dtype=torch.float32)
    D, H, W = out_shape
    return F.affine_grid(theta, (N, 1, D, H, W), align_corners=False).numpy()


def cases():
    """(name, x (N, C, D, H, W) float32, grid (N, Do, Ho, Wo, 3) float32): the lattice, border and shape edges of the sampler.
    Every grid is finite or +-inf (NaN has its own test); outputs cover ovox % 4 in {0, 1, 2, 3}."""
    rng = np.random.default_rng(1234)
    X = lambda *s: rng.random(s, dtype=np.float32) + F32(0.25)          # noqa: E731  (no zeros: every corner matters)
    out = []
    out.append(("identity_W100_C1", X(1, 1, 3, 4, 100), identity(1, (3, 4, 100))))
    out.append(("identity_H97_C2", X(1, 2, 3, 97, 4), identity(1, (3, 97, 4))))
    g = identity(1, (200, 2, 3))
    g[..., 2] = -g[..., 2]
    out.append(("identity_D200_zflip_C3", X(1, 3, 200, 2, 3), g))
    out.append(("identity_W97_xflip_N3_C1", X(3, 1, 2, 3, 97), identity(3, (2, 3, 97))[..., ::-1, :] * 1))
    out.append(("shift_W100_C4", X(1, 4, 6, 7, 100), shift(identity(1, (6, 7, 100)), (6, 7, 100), (3, -2, 1))))
    out.append(("shift_W97_C14", X(1, 14, 5, 6, 97), shift(identity(1, (5, 6, 97)), (5, 6, 97), (-4, 1, -1))))
    g = identity(1, (4, 5, 100))
    g[..., 0], g[..., 2] = -g[..., 0], -g[..., 2]
    out.append(("xz_flip_W100_C2", X(1, 2, 4, 5, 100), g))
    out.append(("permute_cube_C2", X(1, 2, 9, 9, 9), np.ascontiguousarray(identity(1, (9, 9, 9))[..., [1, 2, 0]])))
    out.append(("down2_C128", X(1, 128, 4, 6, 8), identity(1, (2, 3, 4))))          # half-integer coordinates: rint ties
    out.append(("down2_N3_C1", X(3, 1, 8, 12, 16), identity(3, (4, 6, 8))))
    out.append(("up2_C129", X(1, 129, 2, 3, 4), identity(1, (4, 6, 8))))
    out.append(("border_C2_ovox105", X(1, 2, 5, 6, 7), border_grid(1, (5, 6, 7), (3, 5, 7), 1)))
    out.append(("border_W100_C1_ovox42", X(2, 1, 4, 3, 100), border_grid(2, (4, 3, 100), (2, 3, 7), 2)))
    g = rng.choice(np.array([-np.inf, -1e30, -3.0, -1.0000001, 1.0000001, 3.0, 1e30, np.inf, 0.0], F32), size=(1, 3, 1, 5, 3))
    out.append(("beyond_C3_ovox15", X(1, 3, 4, 5, 6), g))
    out.append(("random_N3_C4_ovox45", X(3, 4, 6, 7, 8), (rng.random((3, 3, 3, 5, 3), dtype=np.float32) * F32(2.6) - F32(1.3))))
    out.append(("steep_affine_C2", X(1, 2, 10, 12, 14), steep_affine(1, (7, 9, 11), 5)))
    g = identity(2, (5, 6, 1))
    g[..., 0] = rng.random((2, 5, 6, 1), dtype=np.float32) * F32(3) - F32(1.5)
    out.append(("W1_N2_C2", X(2, 2, 5, 6, 1), g))
    out.append(("W1_C1_random", X(1, 1, 4, 3, 1), rng.random((1, 3, 2, 5, 3), dtype=np.float32) * F32(2.4) - F32(1.2)))
    out.append(("W2_H1_D1_C3", X(1, 3, 1, 1, 2), rng.random((1, 1, 1, 7, 3), dtype=np.float32) * F32(2.4) - F32(1.2)))
    out.append(("W2_H1_D1_identity_C1", X(1, 1, 1, 1, 2), identity(1, (1, 1, 2))))
    return [(n, np.ascontiguousarray(x), np.ascontiguousarray(g, dtype=F32)) for n, x, g in out]


def cotangent(x, grid, seed):
    """a seeded cotangent of the warped tensor (N, C, *out)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((x.shape[0], x.shape[1]) + grid.shape[1:4]).astype(F32)
