"""The definition of keymorph_amd.ops.local_ncc restated in plain torch (dtype-generic: fp64 for the yardstick, fp32 for the size
of fp32's own error), differentiated by autograd and by the closed form the kernel uses; a registration pair under a smooth
bias field; and tests/bspline_ref.py's driver schedule with either similarity.

a, b (N, 1, D, H, W); window w odd, r = w // 2.  box(x) = the sum of x over the in-bounds part of the w^3 cube around each voxel:
F.conv3d with a ones kernel and padding r (zeros add nothing; avg_pool3d refuses volumes smaller than the window), n = box(1).
  Sa, Sb, Saa, Sbb, Sab = box(a), box(b), box(a^2), box(b^2), box(ab)
  cross = Sab - Sa Sb / n    va = max(Saa - Sa^2 / n, 0)    vb = max(Sbb - Sb^2 / n, 0)
  cc = cross^2 / (va vb + eps)      out[n] = mean over the voxels of cc
The fp32 evaluation recentres each sample by its first voxel before anything is squared (exact, and nothing changes in real
arithmetic); the fp64 evaluation does not."""
import functools

import torch
import torch.nn.functional as F

from tests import bspline_ref as B
from tests import warp_mi_ref as W

F64 = torch.float64


def box(x, window):
    r = window // 2
    return F.conv3d(x, torch.ones(1, 1, window, window, window, dtype=x.dtype, device=x.device), padding=r)


def _sums(a, b, window):
    n = box(torch.ones_like(a[:1]), window)
    return n, box(a, window), box(b, window), box(a * a, window), box(b * b, window), box(a * b, window)


def lncc_map(a, b, window=9, eps=1e-5, recentre=None):
    """cc per voxel, (N, 1, D, H, W), in the inputs' dtype.  recentre: subtract each sample's first voxel first (None: in fp32
    only)."""
    if a.dtype == torch.float32 if recentre is None else recentre:
        a = a - a[:, :, :1, :1, :1].detach()
        b = b - b[:, :, :1, :1, :1].detach()
    n, Sa, Sb, Saa, Sbb, Sab = _sums(a, b, window)
    cross = Sab - Sa * Sb / n
    va = (Saa - Sa * Sa / n).clamp_min(0)
    vb = (Sbb - Sb * Sb / n).clamp_min(0)
    return cross * cross / (va * vb + eps)


def lncc(a, b, window=9, eps=1e-5, dtype=F64):
    """(N,) of (N, 1, D, H, W) inputs evaluated in `dtype`."""
    return lncc_map(a.to(dtype), b.to(dtype), window, eps).mean(dim=(1, 2, 3, 4))


def evaluate(a, b, window=9, eps=1e-5, dtype=F64):
    """(out (N,), d out.sum() / da, d out.sum() / db) of float32 inputs evaluated in `dtype` on the CPU, by autograd."""
    a = a.detach().cpu().to(dtype).requires_grad_(True)
    b = b.detach().cpu().to(dtype).requires_grad_(True)
    out = lncc_map(a, b, window, eps).mean(dim=(1, 2, 3, 4))
    da, db = torch.autograd.grad(out.sum(), (a, b))
    return out.detach(), da, db


def closed_form(a, b, window=9, eps=1e-5, dtype=F64):
    """(da, db) of out.sum() by the formulas the kernel uses: with D = va vb + eps, A = 2 cross / D, B = 2 cross^2 vb / D^2,
    C = 2 cross^2 va / D^2, ua = Sa / n, ub = Sb / n and V voxels per sample,
    da = [box(A) b - box(A ub) - box(B) a + box(B ua)] / V,  db = [box(A) a - box(A ua) - box(C) b + box(C ub)] / V."""
    a, b = a.detach().cpu().to(dtype), b.detach().cpu().to(dtype)
    if dtype == torch.float32:
        a = a - a[:, :, :1, :1, :1]
        b = b - b[:, :, :1, :1, :1]
    n, Sa, Sb, Saa, Sbb, Sab = _sums(a, b, window)
    cross = Sab - Sa * Sb / n
    va = (Saa - Sa * Sa / n).clamp_min(0)
    vb = (Sbb - Sb * Sb / n).clamp_min(0)
    den = va * vb + eps
    A, Bc, Cc = 2 * cross / den, 2 * cross * cross * vb / den ** 2, 2 * cross * cross * va / den ** 2
    ua, ub = Sa / n, Sb / n
    V = a[0].numel()

    def bx(x):
        return box(x, window)
    da = (bx(A) * b - bx(A * ub) - bx(Bc) * a + bx(Bc * ua)) / V
    db = (bx(A) * a - bx(A * ua) - bx(Cc) * b + bx(Cc * ub)) / V
    return da, db


# ---- the operator's cases ---------------------------------------------------------------------------------------------------
# name -> (shape, window, seed).  The kernel's tile is 16 x 8 x 32 (z, y, x) voxels.
CASES = {
    "tiny_ragged": ((1, 1, 5, 6, 7), 9, 1),        # the window is larger than the volume; fewer voxels than one workgroup
    "batch": ((2, 1, 16, 16, 16), 9, 2),           # per-sample pivots and outputs; sample 1 on another scale
    "odd_box_w5": ((1, 1, 24, 20, 36), 5, 3),      # ragged tile remainders on all three axes
    "odd_box_w3": ((1, 1, 24, 20, 36), 3, 3),
    "multi_tile": ((1, 1, 40, 36, 70), 9, 4),      # two tiles and a remainder per axis (four and a remainder along y)
    "offset": ((1, 1, 24, 20, 36), 5, 3),          # odd_box_w5 with a + 1000, 50 b + 300: the pivot
    "masked": ((1, 1, 40, 36, 70), 9, 4),          # multi_tile with the low-x half of both volumes 0: exactly constant windows
    "w15": ((1, 1, 20, 20, 40), 15, 5),            # the largest halo
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(a, b, window) of a case, float32 on the CPU."""
    from tests import mi_ref
    shape, window, seed = CASES[name]
    a, b = mi_ref.smooth_pair(shape, seed)
    for n in range(1, shape[0]):                   # another range per sample, as tests/test_mi_gpu.py's _pair
        a[n] = a[n] * (3.0 * n) - 7.0
        b[n] = b[n] * 0.125 + 100.0 * n
    if name == "offset":
        a, b = a + 1000.0, 50.0 * b + 300.0
    if name == "masked":
        a[..., :shape[4] // 2] = 0.0
        b[..., :shape[4] // 2] = 0.0
    return a, b, window


# ---- the registration pair --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def biased_pair():
    """(fixed, moving), (1, 1, 32, 32, 32) float32: fixed = bspline_ref.recovery_pair()[0]; moving = the same normalised texture
    before any remap, tex = clamp((raw - lo) / (hi - lo), 0, 1), under a smooth multiplicative bias field and an additive ramp:
    moving = tex (0.6 + 0.8 c_z c_x + 0.3 sin(3 c_y)) + 0.2 c_y with c = voxel index / (size - 1) per axis.
    apply_bspline(moving, bspline_ref.true_ctrl()) lines up with fixed up to the bias."""
    size = B.SIZE
    fixed = B.recovery_pair()[0]
    ax = torch.arange(size, dtype=F64)
    v = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)
    raw = W._field_at(size, B.TEXTURE_SEED, v, dense=True)
    lo, hi = raw.min(), raw.max()
    tex = ((raw - lo) / (hi - lo)).clamp(0, 1)
    cz, cy, cx = (v[..., k] / (size - 1) for k in range(3))
    moving = tex * (0.6 + 0.8 * cz * cx + 0.3 * torch.sin(3 * cy)) + 0.2 * cy
    return fixed, moving[None, None].float()


# ---- the driver's schedule with either similarity ---------------------------------------------------------------------------
def register(fixed, moving, mat, metric="lncc", window=9, control_spacing=8, bending_weight=0.05, bins=32, shrink=(4, 2, 1),
             iters=60, lr=0.1, dtype=F64):
    """keymorph_amd.io.register_bspline(metric=...) with a given matrix, on the CPU in `dtype`.  "mi" is bspline_ref.register
    itself; "lncc" is the same schedule with the similarity exchanged."""
    if metric == "mi":
        return B.register(fixed, moving, mat, control_spacing, bending_weight, bins, shrink, iters, lr, dtype)
    assert metric == "lncc"
    return B.register(fixed, moving, mat, control_spacing, bending_weight, bins, shrink, iters, lr, dtype,
                      similarity=lambda warped, f_l, level: lncc_map(warped, f_l, window).mean(dim=(1, 2, 3, 4)))


# what biased_run returns in fp64, as tests/test_lncc_cpu.py measures and asserts it (voxels): for a GPU test to print beside its own
RESTATED = {"identity": 1.786, "lncc": 0.621, "mi": 1.575}


@functools.lru_cache(maxsize=None)
def biased_run(metric, dtype=F64):
    """(residual, identity error) in voxels of the restated driver on biased_pair(), defaults, identity matrix."""
    fixed, moving = biased_pair()
    dims = tuple(fixed.shape[2:])
    ctrl = register(fixed, moving, B.identity_mat(1, dims), metric=metric, dtype=dtype)
    truth = B.true_ctrl()
    return float(B.displacement_error(ctrl, truth, dims)[0]), float(B.displacement_error(torch.zeros_like(truth), truth, dims)[0])
