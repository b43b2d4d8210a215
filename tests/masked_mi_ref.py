"""The masked mutual information of keymorph_amd.ops (mutual_information(mask=), warp_mutual_information(fixed_mask=,
moving_mask=, inside=)) restated in plain torch on top of tests/mi_ref.py and tests/warp_mi_ref.py (dtype-generic: fp64 for the
yardstick, fp32 for the size of fp32's own error), and the stationary-structure recovery pair of the masked drivers' tests.

Per sample: voxel v has weight c_v in {0, 1}; h = sum_v c_v w_a(v) w_b(v)^T, M = sum_v c_v, p = h / M (all zero if M = 0),
MI = sum_{p > 0} p ln(p / (pa pb)).  The ranges are the caller's or the WHOLE volume's own, never the masked part's.
Fused: c = fixed_mask & (moving_mask read by the nearest sampler at the grid != 0) & (|grid| <= 1 on all three axes); c is data
(piecewise constant in the matrix), not differentiated."""
import torch
import torch.nn.functional as F

from tests import mi_ref
from tests import warp_mi_ref as W

F64 = torch.float64


def joint(a, b, weight, bins=32, range_a=None, range_b=None):
    """One sample (any shape, flattened), weight of 0s and 1s -> p (bins, bins) = the weighted table over the count."""
    a, b, c = a.reshape(-1), b.reshape(-1), weight.reshape(-1).to(a.dtype)
    rng = []
    for x, r in ((a, range_a), (b, range_b)):
        if r is None:
            rng.append((x.detach().min(), x.detach().max()))
        else:
            rng.append((torch.as_tensor(r[0], dtype=x.dtype), torch.as_tensor(r[1], dtype=x.dtype)))
    wa = mi_ref.window_matrix(a, rng[0][0], rng[0][1], bins)
    wb = mi_ref.window_matrix(b, rng[1][0], rng[1][1], bins)
    h = (wa * c[:, None]).t() @ wb
    M = c.sum()
    return h / M if float(M) > 0 else torch.zeros_like(h)


def mi_sample(a, b, weight, bins=32, range_a=None, range_b=None):
    p = joint(a, b, weight, bins, range_a, range_b)
    return (p * mi_ref.log_ratio(p)).sum()


def mutual_information(a, b, mask, bins=32, ranges=None):
    """(N, 1, D, H, W) pairs and mask -> (N,); ranges: per sample ((lo_a, hi_a), (lo_b, hi_b)) as warp_mi_ref.own_ranges returns
    them (None: the whole volumes' own)."""
    ranges = ranges or W.own_ranges(a.detach(), b.detach())
    return torch.stack([mi_sample(a[n], b[n], mask[n], bins, ranges[n][0], ranges[n][1]) for n in range(a.shape[0])])


def evaluate(a, b, mask, bins=32, ranges=None, dtype=F64):
    """(MI (N,), dMI.sum()/da, dMI.sum()/db) of float32 inputs evaluated in `dtype` on the CPU; the ranges are those of the float32
    volumes either way."""
    ranges = ranges or W.own_ranges(a.detach().cpu(), b.detach().cpu())
    a = a.detach().cpu().to(dtype).requires_grad_(True)
    b = b.detach().cpu().to(dtype).requires_grad_(True)
    mi = mutual_information(a, b, mask.detach().cpu(), bins, ranges)
    if not mi.requires_grad:                       # no sample counted a voxel: MI = 0 does not depend on the inputs
        return mi.detach(), torch.zeros_like(a), torch.zeros_like(b)
    da, db = torch.autograd.grad(mi.sum(), (a, b))
    return mi.detach(), da, db


def counted(grid, fixed_mask=None, moving_mask=None, inside=False):
    """The chain's counted set for a sampling grid (N, D, H, W, 3): (N, 1, D, H, W) bool."""
    c = torch.ones((grid.shape[0], 1, *grid.shape[1:4]), dtype=torch.bool) if fixed_mask is None else fixed_mask != 0
    if moving_mask is not None:
        near = F.grid_sample(moving_mask.to(grid.dtype), grid, mode="nearest", padding_mode="border", align_corners=False)
        c = c & (near != 0)
    if inside:
        c = c & (grid.abs() <= 1).all(-1)[:, None]
    return c


def warp_mi(moving, fixed, mat, bins=32, ranges=None, fixed_mask=None, moving_mask=None, inside=False, c=None):
    """(N,) in the inputs' dtype.  c: the counted set if the caller has it already (it is data), else built from mat's grid."""
    ranges = ranges or W.own_ranges(moving, fixed)
    if c is None:
        c = counted(W.grid_of(mat.detach(), moving.shape[2:]), fixed_mask, moving_mask, inside)
    return mutual_information(W.warp(moving, mat), fixed, c, bins, ranges)


def evaluate_warp(moving, fixed, mat, c, bins=32, dtype=F64, ranges=None):
    """(MI (N,), d MI.sum() / d mat (N, 3, 4)) with the counted set c held fixed, evaluated in `dtype` on the CPU."""
    ranges = ranges or W.own_ranges(moving, fixed)
    m = mat.detach().cpu().to(dtype).requires_grad_(True)
    mi = warp_mi(moving.detach().cpu().to(dtype), fixed.detach().cpu().to(dtype), m, bins, ranges, c=c.cpu())
    (g,) = torch.autograd.grad(mi.sum(), m)
    return mi.detach(), g


def dmat_floor(moving, fixed, mat, c, bins, ranges, grad64):
    """warp_mi_ref.dmat_floor over the counted voxels: bound_a of the compacted pair (its V is the count M), pushed through
    |da_v / dmat| of the counted voxels, over the norm of the fp64 gradient."""
    m64, f64 = moving.detach().cpu().to(F64), fixed.detach().cpu().to(F64)
    grid = W.grid_of(mat.detach().cpu().to(F64), m64.shape[2:]).requires_grad_(True)
    a = F.grid_sample(m64, grid, mode="bilinear", padding_mode="border", align_corners=False)
    (dgrid,) = torch.autograd.grad(a.sum(), grid)
    p = W.base_points(m64.shape[2:]).reshape(-1, 4).abs()
    out = []
    for n in range(m64.shape[0]):
        sel = c[n].cpu().reshape(-1)
        gn = float(grad64[n].norm())
        if int(sel.sum()) == 0 or gn == 0:
            out.append(0.0)
            continue
        ba = W.bound_a(a[n].detach().reshape(-1)[sel], f64[n].reshape(-1)[sel], bins, ranges[n][0], ranges[n][1])
        da = dgrid[n].reshape(-1, 3).flip(-1).abs()[sel]
        out.append(float(torch.einsum("v,vr,vk->rk", ba, da, p[sel]).norm()) / gn)
    return out


# ---- masks of the operator tests ---------------------------------------------------------------------------------------------
def ball(dims, centre=None, radius=None):
    """(D, H, W) bool: voxels within `radius` (default 0.4 of the smallest axis) of `centre` (default the middle), in voxels."""
    centre = [(n - 1) / 2 for n in dims] if centre is None else centre
    radius = 0.4 * min(dims) if radius is None else radius
    v = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=F64) for n in dims], indexing="ij"), dim=-1)
    return ((v - torch.tensor(centre, dtype=F64)) ** 2).sum(-1) <= radius * radius


def sparse(dims):
    """(D, H, W) bool whose counted voxels are one single voxel and one whole aligned run of 64 consecutive voxels (when the
    volume has 128 voxels or more: else the single voxel and the last 7): steps without a counted lane, a wave with one lane, and
    a full wave."""
    V = dims[0] * dims[1] * dims[2]
    m = torch.zeros(V, dtype=torch.bool)
    m[3] = True
    if V >= 256:
        start = (V // 2) // 64 * 64
        m[start:start + 64] = True
    else:
        m[-7:] = True
    return m.reshape(dims)


MASK_KINDS = ("ones", "ball", "sparse")


def mask_of(kind, shape):
    """(N, 1, D, H, W) uint8 of MASK_KINDS, the same for every sample."""
    dims = tuple(shape[2:])
    m = {"ones": lambda: torch.ones(dims, dtype=torch.bool), "ball": lambda: ball(dims), "sparse": lambda: sparse(dims)}[kind]()
    return m[None, None].expand(shape[0], 1, *dims).to(torch.uint8).contiguous()


# ---- the stationary-structure pair ----------------------------------------------------------------------------------------------
# warp_mi_ref.rigid_pair("rigid_a") with one bright textured slab added at the SAME voxel position in both volumes: a head holder
# that did not move with the anatomy.  Planes SLAB_Z of axis 0, value SLAB_AMP (1 + 0.5 checker), checker = +-1 by the parity of
# (y // 2 + x // 2): a texture that lines up with itself at the identity only.  Chosen on the CPU (tests/test_masked_mi_cpu.py
# holds both facts): with both masks = the slab's complement eroded by one voxel, the masked MI of the restatement peaks at the
# true motion; without masks it does not (the identity scores higher).
# Restatement, fp64, 32^3 (true motion / best of the twelve +-1 voxel-equivalent perturbations / identity):
#   masked 0.74306 / 0.73609 / 0.48725      unmasked 0.68425 / 0.71573 / 0.87326
# (planes 2..8 or amplitude 2 give the same two facts with a smaller masked margin.)
SLAB_Z = (2, 7)
SLAB_AMP = 1.0


def slab_mask(size=32):
    """(1, 1, size, size, size) uint8: 0 on the slab dilated by one voxel (the complement eroded by one voxel), else 1."""
    m = torch.ones((1, 1, size, size, size), dtype=torch.uint8)
    m[:, :, max(SLAB_Z[0] - 1, 0):SLAB_Z[1] + 1] = 0
    return m


def slab_pair(size=32):
    """(fixed, moving, L, t, mask): rigid_a's pair with the slab added to both, its motion, and the mask for both volumes."""
    fixed, moving, L, t = W.rigid_pair("rigid_a", size)
    y, x = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    checker = (((y // 2 + x // 2) % 2) * 2 - 1).float()
    slab = SLAB_AMP * (1 + 0.5 * checker)
    fixed, moving = fixed.clone(), moving.clone()
    fixed[0, 0, SLAB_Z[0]:SLAB_Z[1]] += slab
    moving[0, 0, SLAB_Z[0]:SLAB_Z[1]] += slab
    return fixed, moving, L, t, slab_mask(size)
