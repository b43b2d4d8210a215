"""numpy restatement of the trilinear label vote (csrc/label_warp.hip, ops.warp_labels, grid_sample3d(..., "label")), for the
conformance tests of the HIP kernel, and the volumes and coordinate sets those tests share.

Per output voxel: the fp32 source coordinate of tests/sampler_ref.py (ATen's, every operation rounded on its own, border clamp,
NaN -> far border), its floor corner and fractions (fx, fy, fz), the +1 corner clamped to the far border (its fraction is exactly
0 there), and the eight float32 weights ((1 - fx | fx) * (1 - fy | fy)) * (1 - fz | fz) in the sampler's corner order (x
fastest).  For every label l at a corner, S_l adds the weights of the corners that hold l, in corner order, every addition
rounded to float32 -- what the sampler's fma chain does to the 0 / 1 channel of l.  The largest S_l wins, the smallest label
among equals.  vote() does exactly that in float32; vote64() does it in float64 from the same fp32 coordinates and also returns
the margin between the winner and the best other label, which says where a different order of additions may choose otherwise."""
import numpy as np

from tests import sampler_ref as S

F32 = np.float32


def _corner_labels_and_weights(lab, grid, dtype):
    """lab (N, C, D, H, W) integers, grid (N, *out, 3) float32 -> 8 corner label arrays (N, C, *out) and 8 weights (N, *out) of
    `dtype`, in the sampler's corner order"""
    lab = np.asarray(lab)
    grid = np.asarray(grid, dtype=F32)
    N = lab.shape[0]
    D, H, W = lab.shape[2:]
    ax = []
    for k, size in ((0, W), (1, H), (2, D)):
        c = S.source_coord(grid[..., k], size)[0]                 # the fp32 coordinate, held in float64
        i0 = np.floor(c).astype(np.int64)
        f = (c - i0).astype(dtype)                                # exact in float32 as in float64
        ax.append((i0, np.minimum(i0 + 1, size - 1), f))
    (x0, x1, fx), (y0, y1, fy), (z0, z1, fz) = ax
    one = dtype(1)
    nidx = np.arange(N).reshape((N,) + (1,) * (grid.ndim - 2))
    labs, ws = [], []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi, zi = (x1 if dx else x0), (y1 if dy else y0), (z1 if dz else z0)
                labs.append(np.moveaxis(lab[nidx, :, zi, yi, xi], -1, 1))
                wx, wy, wz = (fx if dx else one - fx), (fy if dy else one - fy), (fz if dz else one - fz)
                ws.append(((wx * wy) * wz).astype(dtype))
    return labs, ws


def _vote(lab, grid, dtype):
    labs, ws = _corner_labels_and_weights(lab, grid, dtype)
    sums = []
    for k in range(8):
        o = np.zeros(labs[0].shape, dtype)
        for j in range(8):
            o = np.where(labs[j] == labs[k], (o + ws[j][:, None]).astype(dtype), o)
        sums.append(o)
    best, bs = labs[0].copy(), sums[0].copy()
    for k in range(1, 8):
        take = (sums[k] > bs) | ((sums[k] == bs) & (labs[k] < best))
        best, bs = np.where(take, labs[k], best), np.where(take, sums[k], bs)
    other = np.zeros(bs.shape, dtype)                             # the best label that is not the winner (0: there is none)
    for k in range(8):
        other = np.where(labs[k] != best, np.maximum(other, sums[k]), other)
    return best.astype(np.asarray(lab).dtype), bs, bs - other


def vote(lab, grid):
    """(labels (N, C, *out) of lab's dtype, weight (N, C, *out) float32): the definition, in float32"""
    best, bs, _ = _vote(lab, grid, F32)
    return best, bs


def vote64(lab, grid):
    """(labels, weight float64, margin float64): the same vote with float64 weights and sums"""
    return _vote(lab, grid, np.float64)


# ---------------------------------------------------------------------------------------------------- volumes and coordinates
OUT_SHAPE = (3, 19, 37)          # 2109 output voxels: two chunks of the kernel and a ragged third


def random_labels(shape, nlab, seed, dtype=np.int64):
    """i.i.d. labels in [0, nlab): (N, C, D, H, W)"""
    return np.random.default_rng(seed).integers(0, nlab, size=shape).astype(dtype)


def _centres(size):
    return S.identity(1, (1, 1, size))[0, 0, 0, :, 0]            # fp32 normalised coordinates of the voxel centres


def _halfway(size):
    if size < 2:
        return np.zeros(1, F32)
    return (F32(2) * np.arange(1, size, dtype=F32) / F32(size) - F32(1)).astype(F32)


def _pick(rng, per_axis, N, out_shape):
    g = np.empty((N,) + tuple(out_shape) + (3,), F32)
    for k in range(3):
        g[..., k] = rng.choice(per_axis[k], size=g.shape[:-1])
    return g


def coordinate_set(name, N, in_shape, out_shape=OUT_SHAPE, seed=0):
    """grid (N, *out_shape, 3) float32 of one kind: "interior", "outside" (beyond +-1, to +-1.3), "lattice" (every coordinate a
    voxel centre), "border" (the first / last centre, one ulp to either side of them, and +-1), "halfway" (every coordinate
    midway between two centres: exact ties where the size is a power of two, near ties elsewhere), "nonfinite" (NaN and +-inf per
    component among finite ones)"""
    D, H, W = in_shape
    rng = np.random.default_rng([seed, D, H, W, sum(map(ord, name))])
    shape = (N,) + tuple(out_shape) + (3,)
    sizes = (W, H, D)
    if name == "interior":
        return (rng.random(shape, dtype=F32) * F32(1.9) - F32(0.95)).astype(F32)
    if name == "outside":
        return (rng.random(shape, dtype=F32) * F32(2.6) - F32(1.3)).astype(F32)
    if name == "lattice":
        return _pick(rng, [_centres(s) for s in sizes], N, out_shape)
    if name == "border":
        return _pick(rng, [np.concatenate([S.border_points(s), np.array([-1, 1], F32)]) for s in sizes], N, out_shape)
    if name == "halfway":
        return _pick(rng, [_halfway(s) for s in sizes], N, out_shape)
    if name == "nonfinite":
        g = (rng.random(shape, dtype=F32) * F32(2.2) - F32(1.1)).astype(F32)
        kind = rng.integers(0, 8, size=shape)
        g[kind == 0], g[kind == 1], g[kind == 2] = np.nan, np.inf, -np.inf
        return g
    raise KeyError(name)


SETS = ("interior", "outside", "lattice", "border", "halfway")


def exact_halfway(size):
    """the normalised fp32 coordinates near 2 i / size - 1 whose fp32 source coordinate is EXACTLY i - 1/2 (i = 1 .. size - 1)"""
    out = []
    for i in range(1, size):
        g = F32(2.0 * i / size - 1.0)
        cand = [g]
        for _ in range(2):
            cand = [np.nextafter(cand[0], F32(-2))] + cand + [np.nextafter(cand[-1], F32(2))]
        hit = [c for c in cand if S.source_coord(np.array([c], F32), size)[0][0] == i - 0.5]
        out += hit[:1]
    return np.array(out, F32)


def ball_shells(size=32):
    """(1, 1, size, size, size) uint8: a ball of radius 6 (label 1), a shell to 11 (2), the x >= centre half of a shell to 13
    (3), background 0 -- the map of the README's rotation figure"""
    c = (size - 1) / 2.0
    z, y, x = np.meshgrid(*(np.arange(size) - c,) * 3, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    lab = np.zeros((size,) * 3, np.uint8)
    lab[(r <= 13) & (x >= 0)] = 3
    lab[r <= 11] = 2
    lab[r <= 6] = 1
    return lab[None, None]


def rotation_z(deg, size=32):
    """(1, 3, 4) float32 matrix of ops.affine_grid / io.apply_mat: rotation of a size^3 volume by deg about the z axis through its
    centre, no shift.  The factor (size - 1) / size cancels affine_grid's linspace(-1, 1) base grid against align_corners=False
    sampling, as in io.translate: without it the identity matrix zooms by size / (size - 1)."""
    a = np.deg2rad(deg)
    m = np.zeros((1, 3, 4), np.float64)
    m[0, 0, 0], m[0, 0, 1], m[0, 1, 0], m[0, 1, 1], m[0, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1
    return (m * ((size - 1) / size)).astype(F32)


def dice_formula(x, y):
    """(mean, labels, per-label) of 2 |x = l and y = l| / (|x = l| + |y = l| + 1e-5) over the labels in either map, in numpy; one
    label alone: 2 |and| / (|x| + |y|), as the reference's fast_dice falls back to dice"""
    x, y = np.asarray(x).ravel(), np.asarray(y).ravel()
    labels = np.union1d(x, y)
    cx = np.array([(x == l).sum() for l in labels], np.float64)
    cy = np.array([(y == l).sum() for l in labels], np.float64)
    cxy = np.array([((x == l) & (y == l)).sum() for l in labels], np.float64)
    per = 2 * cxy / (cy + cx + 1e-5) if len(labels) > 1 else 2 * cxy / (cx + cy)
    return float(np.mean(per)), labels.astype(np.int64), per
