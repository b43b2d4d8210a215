"""The dense displacement model (keymorph_amd.ops.displacement_grid, displacement_step_scale, displacement_update: csrc/dense.hip)
and the schedule of keymorph_amd.io.register_greedy restated in plain torch (dtype-generic: fp64 for the yardstick, fp32 for the
size of fp32's own error), from svf_ref.finish / interpolate, gauss_ref.smooth and bspline_ref.mi_similarity.

disp (N, 3, D, H, W): channels (z, y, x), voxels of its own lattice (fields_ref.to_displacement's convention).
    u            = disp over S / 2 per axis, reordered to (N, D, H, W, 3) xyz                         (normalised)
    grid         = Ids + u                       (mat None)   or   affine_grid(mat)[w] + L (s * u[w])  (svf_ref.finish)
    step_scale   = step / max_w |delta[n, :, w]|_2 over the voxels with a finite norm; 0 where that maximum is 0
    update       = delta' + U(Ids + delta' over S / 2),  delta' = delta * scale[n]  (delta when scale is None), U the trilinear,
                   border-clamped interpolant of disp (F.grid_sample(padding_mode="border", align_corners=False))
Per iteration of the driver at a level, with d the level's field:
    g = d similarity(grid_sample(m_l, grid(d, mat_l)), f_l) / d d;   g = smooth(g, sigma_update);   s = step_scale(g, step);
    d = smooth(update(d, g, s), sigma_total)
and between levels d is resized trilinearly, each channel times new size / old size of its axis."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import bspline_ref as R
from tests import gauss_ref
from tests import svf_ref as S
from tests import warp_mi_ref as W

F64 = torch.float64
STEP, SIGMA_UPDATE, SIGMA_TOTAL, ITERS = 0.5, 3 ** 0.5, 0.5 ** 0.5, 60
# recovery_run's fp64 answers with these defaults, amplitude -> (mean grid error in voxels, minimum Jacobian): the same to six digits
# on every host tried.  tests/test_dense_cpu.py recomputes them; tests/test_dense_gpu.py measures io.register_greedy against them.
RECOVERY_FP64 = {4.0: (0.559081, 0.557753), 8.0: (0.991471, 0.496337)}


def _half(dims, dtype):
    """S / 2 per channel (z, y, x), shaped for (N, 3, D, H, W)."""
    return torch.tensor([n / 2 for n in dims], dtype=dtype)[None, :, None, None, None]


def normalised(disp):
    """u (N, D, H, W, 3), xyz: disp over S / 2."""
    return (disp / _half(disp.shape[2:], disp.dtype)).permute(0, 2, 3, 4, 1).flip(-1)


def grid(disp, mat=None):
    dims = tuple(disp.shape[2:])
    return S.finish(normalised(disp), dims, mat)


def step_scale(delta, step):
    """(N,) in delta's dtype."""
    n2 = (delta * delta).sum(dim=1).flatten(1)
    n2 = torch.where(torch.isfinite(n2), n2, torch.zeros_like(n2))
    m = n2.amax(dim=1).sqrt()
    return torch.where(m > 0, step / m, torch.zeros_like(m))


def update(disp, delta, scale=None):
    dims = tuple(disp.shape[2:])
    if scale is not None:
        delta = delta * scale.to(delta.dtype)[:, None, None, None, None]
    pts = R.identity(dims, disp.dtype)[None] + normalised(delta)
    return delta + F.grid_sample(disp, pts, mode="bilinear", padding_mode="border", align_corners=False)


def smooth(x, sigma):
    dt = np.float64 if x.dtype == F64 else np.float32
    return torch.from_numpy(gauss_ref.smooth(x.detach().numpy(), sigma, dtype=dt))


def evaluate_grid(disp, mat, cot, dtype):
    """(grid, d (grid * cot).sum() / d disp) of float32 inputs evaluated in `dtype` on the CPU."""
    d = disp.detach().cpu().to(dtype).requires_grad_(True)
    g = grid(d, None if mat is None else mat.detach().cpu().to(dtype))
    (dd,) = torch.autograd.grad((g * cot.detach().cpu().to(dtype)).sum(), d)
    return g.detach(), dd


def resize_field(d, ldims):
    """d on another lattice: trilinear (align_corners=False), each channel times new size / old size of its axis."""
    old = tuple(d.shape[2:])
    if old == tuple(ldims):
        return d
    out = F.interpolate(d, size=tuple(ldims), mode="trilinear", align_corners=False)
    return out * torch.tensor([n / o for n, o in zip(ldims, old)], dtype=d.dtype)[None, :, None, None, None]


def register(fixed, moving, mat, step=STEP, sigma_update=SIGMA_UPDATE, sigma_total=SIGMA_TOTAL, shrink=(4, 2, 1), iters=ITERS,
             bins=32, dtype=F64, similarity=R.mi_similarity, trace=None):
    """keymorph_amd.io.register_greedy with a given matrix, on the CPU in `dtype`: bspline_ref.register's levels and per-level
    matrices around the greedy iteration.  trace: a list that receives the mean similarity of every iteration."""
    fixed, moving, mat = fixed.detach().to(dtype), moving.detach().to(dtype), mat.detach().to(F64)
    N, dims = fixed.shape[0], tuple(fixed.shape[2:])
    n = torch.tensor([float(d) for d in dims], dtype=F64)
    L = mat[:, :, :3] * n[None, :, None] / (n - 1)[None, None, :]
    t = mat[:, :, 3] * n[None, :] / 2
    per_level = list(iters) if isinstance(iters, (list, tuple)) else [iters] * len(shrink)
    d = None
    for sh, its in zip(shrink, per_level):
        ldims = tuple(x // int(sh) for x in dims)
        if min(ldims) < 16:
            continue
        if ldims == dims:
            f_l, m_l = fixed, moving
        else:
            f_l = F.interpolate(fixed, size=ldims, mode="trilinear", align_corners=False)
            m_l = F.interpolate(moving, size=ldims, mode="trilinear", align_corners=False)
        level = {"moving": m_l, "bins": bins}
        ratio = torch.tensor([a / b for a, b in zip(dims, ldims)], dtype=F64)
        mat_l = W.voxel_to_mat(L * ratio[None, None, :] / ratio[None, :, None], t / ratio[None, :], ldims).to(dtype)
        d = torch.zeros((N, 3, *ldims), dtype=dtype) if d is None else resize_field(d, ldims)
        for _ in range(int(its)):
            d = d.detach().requires_grad_(True)
            warped = F.grid_sample(m_l, grid(d, mat_l), mode="bilinear", padding_mode="border", align_corners=False)
            sim = similarity(warped, f_l, level)
            (g,) = torch.autograd.grad(sim.sum(), d)
            if trace is not None:
                trace.append(float(sim.mean()))
            g = smooth(g, sigma_update)
            d = smooth(update(d.detach(), g, step_scale(g, step)), sigma_total)
    return resize_field(d.detach(), dims)


def folded(disp):
    """(minimum, number of non-positive values) of the central-difference Jacobian determinant on the interior voxels."""
    from tests import fields_ref
    det = fields_ref.jacobian_det_central(disp.detach().cpu())
    return float(det.min()), int((det <= 0).sum())


@functools.lru_cache(maxsize=None)
def recovery_run(amplitude=R.AMPLITUDE, dtype=F64):
    """(disp, grid error in voxels, identity's grid error, minimum Jacobian, folded voxels) of the restated driver with its
    defaults on svf_ref.recovery_pair(amplitude) from the identity matrix.  Amplitude 4 is bspline_ref.recovery_pair()."""
    fixed, moving = S.recovery_pair(amplitude)
    dims = tuple(fixed.shape[2:])
    mat = R.identity_mat(1, dims)
    disp = register(fixed, moving, mat, dtype=dtype)
    err = float(S.grid_error(grid(disp.to(F64), mat), amplitude, dims)[0])
    ident = float(S.grid_error(grid(torch.zeros_like(disp, dtype=F64), mat), amplitude, dims)[0])
    return (disp, err, ident) + folded(disp)


def fp32_distance(amplitude=R.AMPLITUDE):
    """(distance, fp32 mean error): how far the restated driver's mean error moves when the whole schedule runs in fp32 instead of
    fp64, on the host that calls this.  It is MEASURED where it is used and not pinned: 120 greedy iterations amplify the order
    of torch's fp32 sums, which depends on the host's vector width -- 6.73e-4 (fp32 0.559754) on one x86 host, 1.93e-4 (0.559274)
    on another, each the same at any thread count, against an fp64 figure of 0.559081 on both."""
    e32 = recovery_run(amplitude, torch.float32)[1]
    return abs(e32 - RECOVERY_FP64[amplitude][0]), e32
