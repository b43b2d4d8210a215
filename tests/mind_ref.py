"""The definition of keymorph_amd.ops.mind_ssc_loss restated in plain torch (dtype-generic: fp64 for the yardstick, fp32 for the
size of fp32's own error), differentiated by autograd and by the closed form the kernel uses (which fixes the tie of the minimum
at the lowest channel index); the operator's cases; a registration pair under an inverted, non-linear contrast and a smooth
bias field; and tests/bspline_ref.py's driver schedule with this similarity.

a, b (N, 1, D, H, W); radius r, dilation d; clamp = the per-axis clamp into the volume, F.pad(mode="replicate").
  neighbours   0: -d z   1: +d z   2: -d y   3: +d y   4: -d x   5: +d x
  channels     CHANNELS below: the 12 unordered pairs (i, j) of distinct, non-opposite neighbours
  E_c(q) = (I(clamp(q + o_i)) - I(clamp(q + o_j)))^2
  D_c = avg_pool3d of the replicate-padded E_c over (2r+1)^3
  m_c = D_c - min_k D_k      V = clamp(mean_c m_c, lo, hi)      M_c = exp(-m_c / V)   (V == 0, only with lo == 0: M_c = 1)
  out[n] = mean over the voxels and the channels of (M_c(a) - M_c(b))^2
bounds (N, 2, 2) = [a or b][lo or hi], constants: by default (1e-3, 1e3) x each sample's mean over the voxels of mean_c m_c."""
import functools

import torch
import torch.nn.functional as F

from tests import bspline_ref as B
from tests import warp_mi_ref as W

F64 = torch.float64
CHANNELS = ((0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (1, 3), (1, 4), (1, 5), (2, 4), (2, 5), (3, 4), (3, 5))


def _views(P, d, dims):
    """The six shifted (D, H, W) windows, in the order above, of a volume P padded by d."""
    D, H, Wd = dims

    def s(dz, dy, dx):
        return P[:, :, d + dz:d + dz + D, d + dy:d + dy + H, d + dx:d + dx + Wd]
    return [s(-d, 0, 0), s(d, 0, 0), s(0, -d, 0), s(0, d, 0), s(0, 0, -d), s(0, 0, d)]


def _neighbours(x, d):
    """The six clamped shifts of x (N, 1, D, H, W)."""
    return _views(F.pad(x, (d,) * 6, mode="replicate"), d, x.shape[2:])


def distances(x, r, d):
    """D (N, 12, D, H, W): the box means of the squared neighbour differences."""
    nb = _neighbours(x, d)
    E = torch.cat([(nb[i] - nb[j]) ** 2 for i, j in CHANNELS], dim=1)
    return F.avg_pool3d(F.pad(E, (r,) * 6, mode="replicate"), 2 * r + 1, stride=1)


def _m(x, r, d):
    Dx = distances(x, r, d)
    m = Dx - Dx.min(dim=1, keepdim=True).values
    return Dx, m, m.mean(dim=1, keepdim=True)


def bounds_of(a, b, r=1, d=2):
    """(N, 2, 2) in the inputs' dtype, detached: (1e-3, 1e3) x the mean over the voxels of mean_c m_c, of a then of b."""
    with torch.no_grad():
        means = torch.stack([_m(x, r, d)[2].mean(dim=(1, 2, 3, 4)) for x in (a, b)], dim=1)           # (N, 2)
        return torch.stack([1e-3 * means, 1e3 * means], dim=2)


def _inv(V):
    pos = V > 0
    return torch.where(pos, 1 / torch.where(pos, V, torch.ones_like(V)), torch.zeros_like(V))


def descriptor(x, r, d, lohi):
    """M (N, 12, D, H, W); lohi (N, 2) of this image."""
    _, m, mean = _m(x, r, d)
    V = torch.clamp(mean, lohi[:, 0].reshape(-1, 1, 1, 1, 1), lohi[:, 1].reshape(-1, 1, 1, 1, 1))
    return torch.exp(-m * _inv(V))


def mind_map(a, b, r=1, d=2, bounds=None):
    """(M_c(a) - M_c(b))^2, (N, 12, D, H, W), in the inputs' dtype.  bounds None: bounds_of(a, b)."""
    if bounds is None:
        bounds = bounds_of(a, b, r, d)
    bounds = bounds.detach().to(a.dtype)
    return (descriptor(a, r, d, bounds[:, 0]) - descriptor(b, r, d, bounds[:, 1])) ** 2


def mind(a, b, r=1, d=2, bounds=None, dtype=F64):
    """(N,) of (N, 1, D, H, W) inputs evaluated in `dtype`."""
    return mind_map(a.to(dtype), b.to(dtype), r, d, bounds).mean(dim=(1, 2, 3, 4))


def evaluate(a, b, r=1, d=2, dtype=F64, bounds=None):
    """(out (N,), d out.sum() / da, d out.sum() / db) of float32 inputs evaluated in `dtype` on the CPU, by autograd."""
    a = a.detach().cpu().to(dtype).requires_grad_(True)
    b = b.detach().cpu().to(dtype).requires_grad_(True)
    out = mind_map(a, b, r, d, bounds).mean(dim=(1, 2, 3, 4))
    da, db = torch.autograd.grad(out.sum(), (a, b))
    return out.detach(), da, db


def _pad_T(g, p):
    """The transpose of F.pad(., (p,) * 6, "replicate"): the padding folded onto the faces."""
    for ax in (2, 3, 4):
        n = g.shape[ax] - 2 * p
        core = g.narrow(ax, p, n).clone()
        core.narrow(ax, 0, 1).add_(g.narrow(ax, 0, p).sum(dim=ax, keepdim=True))
        core.narrow(ax, n - 1, 1).add_(g.narrow(ax, n + p, p).sum(dim=ax, keepdim=True))
        g = core
    return g


def _box_T(g, r):
    """The transpose of the replicate-padded box mean, channel by channel."""
    k = 2 * r + 1
    N, C = g.shape[:2]
    full = F.conv_transpose3d(g.reshape(N * C, 1, *g.shape[2:]), torch.full((1, 1, k, k, k), 1.0 / k ** 3, dtype=g.dtype))
    return _pad_T(full, r).reshape(N, C, *g.shape[2:])


def _side(x, y, lohi_x, lohi_y, r, d):
    """d out.sum() / dx by the kernel's formulas (csrc/mind.hip), ties of the minimum at the lowest channel index."""
    Dx, m, mean = _m(x, r, d)
    lo, hi = lohi_x[:, 0].reshape(-1, 1, 1, 1, 1), lohi_x[:, 1].reshape(-1, 1, 1, 1, 1)
    inv = _inv(torch.clamp(mean, lo, hi))
    Mx, My = torch.exp(-m * inv), descriptor(y, r, d, lohi_y)
    t = 2 * (Mx - My) / (len(CHANNELS) * x[0].numel()) * Mx
    inside = ((mean >= lo) & (mean <= hi)).to(x.dtype)
    gm = -t * inv + inside * (t * m).sum(dim=1, keepdim=True) * inv ** 2 / len(CHANNELS)
    eq = Dx == Dx.min(dim=1, keepdim=True).values
    first = (eq & (eq.cumsum(dim=1) == 1)).to(x.dtype)
    gE = _box_T(gm - first * gm.sum(dim=1, keepdim=True), r)
    nb = _neighbours(x, d)
    Dd, H, Wd = x.shape[2:]
    gP = torch.zeros(x.shape[0], 1, Dd + 2 * d, H + 2 * d, Wd + 2 * d, dtype=x.dtype)
    views = _views(gP, d, (Dd, H, Wd))
    for c, (i, j) in enumerate(CHANNELS):
        term = 2 * gE[:, c:c + 1] * (nb[i] - nb[j])
        views[i].add_(term)
        views[j].sub_(term)
    return _pad_T(gP, d)


def closed_form(a, b, r=1, d=2, dtype=F64, bounds=None):
    """(da, db) of out.sum() by the closed form."""
    a, b = a.detach().cpu().to(dtype), b.detach().cpu().to(dtype)
    with torch.no_grad():
        bounds = (bounds_of(a, b, r, d) if bounds is None else bounds).to(dtype)
        return _side(a, b, bounds[:, 0], bounds[:, 1], r, d), _side(b, a, bounds[:, 1], bounds[:, 0], r, d)


# ---- the operator's cases ---------------------------------------------------------------------------------------------------
# name -> (shape, (r, d), seed).  The kernel's tile is 4 x 8 x 32 (z, y, x) voxels.
CASES = {
    "tiny_ragged": ((1, 1, 5, 6, 7), (2, 3), 1),       # the halo is larger than the volume; fewer voxels than one workgroup
    "batch": ((2, 1, 16, 16, 16), (1, 2), 2),          # sample 1 on another scale: per-sample bounds
    "ragged_r1d1": ((1, 1, 24, 20, 36), (1, 1), 3),    # tile remainders on all three axes (x: 32 + 4, y: 2 x 8 + 4)
    "ragged_r2d2": ((1, 1, 24, 20, 36), (2, 2), 3),
    "multi_tile": ((1, 1, 40, 36, 70), (1, 2), 4),     # two tiles and more plus a remainder per axis
    "masked": ((1, 1, 40, 36, 70), (1, 2), 4),         # multi_tile with the low-x half of a alone 0: the lower clamp active,
                                                       # 12-way ties of the minimum under a non-zero cotangent
    "r3d3": ((1, 1, 20, 20, 40), (3, 3), 5),           # the largest halo
}
TIED = ("masked",)                                     # exact ties: autograd's choice among them is not the definition's


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(a, b, r, d) of a case, float32 on the CPU."""
    from tests import mi_ref
    shape, (r, d), seed = CASES[name]
    a, b = mi_ref.smooth_pair(shape, seed)
    for n in range(1, shape[0]):                       # another range per sample, as tests/lncc_ref.py
        a[n] = a[n] * (3.0 * n) - 7.0
        b[n] = b[n] * 0.125 + 100.0 * n
    if name == "masked":
        a[..., :shape[4] // 2] = 0.0
    return a, b, r, d


# ---- the registration pair --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inverted_pair():
    """(fixed, moving), (1, 1, 32, 32, 32) float32: fixed = bspline_ref.recovery_pair()[0]; moving = the same normalised texture
    tex (as tests/lncc_ref.biased_pair) under an inverted, non-linear contrast, lncc_ref's smooth multiplicative bias field and
    its additive ramp: moving = (1 - tex)^2 (0.6 + 0.8 c_z c_x + 0.3 sin(3 c_y)) + 0.2 c_y, c = voxel index / (size - 1)."""
    size = B.SIZE
    fixed = B.recovery_pair()[0]
    ax = torch.arange(size, dtype=F64)
    v = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)
    raw = W._field_at(size, B.TEXTURE_SEED, v, dense=True)
    lo, hi = raw.min(), raw.max()
    tex = ((raw - lo) / (hi - lo)).clamp(0, 1)
    cz, cy, cx = (v[..., k] / (size - 1) for k in range(3))
    moving = (1 - tex) ** 2 * (0.6 + 0.8 * cz * cx + 0.3 * torch.sin(3 * cy)) + 0.2 * cy
    return fixed, moving[None, None].float()


# ---- the driver's schedule with this similarity -----------------------------------------------------------------------------
def mind_similarity(r=1, d=2):
    """-MIND-SSC for bspline_ref.register; the bounds are the level's own unwarped pair's, found once and kept in `level`."""
    def similarity(warped, f_l, level):
        if "mind_bounds" not in level:
            level["mind_bounds"] = bounds_of(level["moving"], f_l, r, d)
        return -mind_map(warped, f_l, r, d, level["mind_bounds"]).mean(dim=(1, 2, 3, 4))
    return similarity


def register(fixed, moving, mat, metric="mind", r=1, d=2, control_spacing=8, bending_weight=0.05, bins=32, shrink=(4, 2, 1),
             iters=60, lr=0.1, dtype=F64):
    """keymorph_amd.io.register_bspline(metric=...) with a given matrix, on the CPU in `dtype`."""
    if metric == "mi":
        return B.register(fixed, moving, mat, control_spacing, bending_weight, bins, shrink, iters, lr, dtype)
    assert metric == "mind"
    return B.register(fixed, moving, mat, control_spacing, bending_weight, bins, shrink, iters, lr, dtype,
                      similarity=mind_similarity(r, d))


# what inverted_run returns in fp64, as tests/test_mind_cpu.py measures and asserts it (voxels): for a GPU test to print beside
# its own
RESTATED = {"identity": 1.786, "mind": 0.859, "mi": 1.671}


@functools.lru_cache(maxsize=None)
def inverted_run(metric, dtype=F64):
    """(residual, identity error) in voxels of the restated driver on inverted_pair(), defaults, identity matrix."""
    fixed, moving = inverted_pair()
    dims = tuple(fixed.shape[2:])
    ctrl = register(fixed, moving, B.identity_mat(1, dims), metric=metric, dtype=dtype)
    truth = B.true_ctrl()
    return float(B.displacement_error(ctrl, truth, dims)[0]), float(B.displacement_error(torch.zeros_like(truth), truth, dims)[0])
