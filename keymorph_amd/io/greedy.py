"""Dense greedy diffeomorphic registration on the GPU: the transform is a voxel displacement field, one vector per voxel, instead of
a control lattice -- the model of ANTs SyN and of the `greedy` tool.  Per iteration the gradient of the similarity in the field
is smoothed by a Gaussian (the "fluid" regulariser), scaled so that its longest vector is `step` voxels, COMPOSED onto the field
(phi <- phi o (Id + update), not added), and the total field is smoothed by a second Gaussian (the "diffusion" regulariser).
Each composed map is within `step` < 1 voxel of the identity, so the field stays invertible without a bending penalty.

Conventions.  disp (N, 3, D, H, W) float32: channels (z, y, x), voxels of its own lattice -- fields.to_displacement's convention,
what loss_ops.jdstd / jdlessthan0 read and ops.gaussian_smooth works on as it is.  `mat` (N, 3, 4) is what ops.affine_grid takes;
the grid is the matrix applied to the deformed point (ops.displacement_grid)."""
import torch

from ._deformable import counted_voxels, metric_table
from ._pyramid import as_data, level_entries, levels, mask_levels, resolve_smoothing, scale_axes
from .intensity import _conjugate, mat_to_voxel, register_intensity, voxel_to_mat


def apply_greedy(x, disp, mat=None, mode="bilinear"):
    """align_img(ops.displacement_grid(disp, mat), x, mode): x (N, C, D, H, W) in moving space resampled into fixed space through
    the field; every mode of align_img ("bilinear", "nearest", "cubic", "label")."""
    from .. import ops
    from ..utils import align_img
    return align_img(ops.displacement_grid(disp, mat), x, mode)


def _resize_field(d, ldims):
    """d (N, 3, ...) on the lattice ldims: trilinear, each channel times new size / old size of its axis (a displacement is in
    voxels of its own lattice)."""
    from ..utils import resize_trilinear
    old = tuple(d.shape[2:])
    if old == tuple(ldims):
        return d
    return scale_axes(resize_trilinear(d, size=tuple(ldims)), [n / o for n, o in zip(ldims, old)])


def register_greedy(fixed, moving, mat=None, step=0.5, sigma_update=3 ** 0.5, sigma_total=0.5 ** 0.5, shrink=(4, 2, 1), iters=60,
                    bins=32, metric="mi", window=9, mind_radius=1, mind_dilation=2, fixed_mask=None, moving_mask=None, inside=False,
                    smoothing_sigmas=None):
    """disp (N, 3, D, H, W) at the full size such that apply_greedy(moving, disp, mat) lines up with fixed (both (N, 1, D, H, W)
    float32 on the GPU, of one shape).  mat None: register_intensity's affine answer, as the lattice drivers start.  The pyramid is
    theirs (shrink, levels with an axis under 16 skipped, smoothing_sigmas, per-level matrix), and so are the metrics "mi", "lncc"
    and "mind".  Per iteration at a level, with d the level's field in voxels of the level:
        g = d similarity(align_img(ops.displacement_grid(d, mat_l), moving_l), fixed_l) / d d
        g = ops.gaussian_smooth(g, sigma_update);   s = ops.displacement_step_scale(g, step)      (the longest update: `step` voxels)
        d = ops.gaussian_smooth(ops.displacement_update(d, g, s), sigma_total)
    and between levels d is resized trilinearly, each channel times the ratio of its axis.  iters: a number, or one per entry of
    `shrink`.  sigma_update, sigma_total: voxels of the level, a number or a (z, y, x) triple; 0 switches a smoothing off.  The
    defaults are those of the fp64 restatement (tests/dense_ref.py; DESIGN.md section 8m has its figures).

    fixed_mask, moving_mask, inside: which voxels the mutual information counts, as io.register_svf takes them; with "lncc" or
    "mind" any of them raises ValueError.

    Every sample is stepped on its own scale and every kernel sums in a fixed or order-independent way: a batch equals its
    samples, bit for bit.  Nothing inside the loop waits for the GPU."""
    from .. import ops
    from ..utils import align_img
    who = "register_greedy"
    table = metric_table(who, metric, bins, window, mind_radius, mind_dilation)
    if fixed.shape != moving.shape or fixed.dim() != 5 or fixed.shape[1] != 1:
        raise ValueError(f"{who}: expected two (N, 1, D, H, W) volumes of one shape, got {tuple(fixed.shape)} and "
                         f"{tuple(moving.shape)}")
    masked = fixed_mask is not None or moving_mask is not None or bool(inside)
    if masked and metric != "mi":
        raise ValueError(f"{who}: fixed_mask, moving_mask and inside work with metric='mi' only, got metric={metric!r}")
    resolve_smoothing(who, shrink, smoothing_sigmas)
    shrink = tuple(shrink)
    per_level = list(iters) if isinstance(iters, (list, tuple)) else [iters] * len(shrink)
    if len(per_level) != len(shrink) or any(isinstance(i, bool) or int(i) != i or i < 0 for i in per_level):
        raise ValueError(f"{who}: iters must be a non-negative integer or one per entry of shrink={shrink}, got {iters!r}")
    step = float(step)
    if not 0 < step < float("inf"):
        raise ValueError(f"{who}: step must be a positive number of voxels, got {step!r}")
    for name, s in (("sigma_update", sigma_update), ("sigma_total", sigma_total)):
        ops._gauss_sigmas(f"{who}: {name}", s, 4.0)
    N, dims = fixed.shape[0], tuple(fixed.shape[2:])
    if mat is not None and tuple(mat.shape) != (N, 3, 4):
        raise ValueError(f"{who}: mat must be ({N}, 3, 4), got {tuple(mat.shape)}")
    kept = [int(i) for i in level_entries(dims, shrink, per_level)]
    with torch.inference_mode(False), torch.enable_grad():
        fixed, moving = as_data(fixed), as_data(moving)
        fmasks = mask_levels(who, "fixed_mask", fixed_mask, fixed, shrink)
        mmasks = mask_levels(who, "moving_mask", moving_mask, moving, shrink)
        if mat is None:
            mat = register_intensity(fixed, moving, "affine", bins=bins, shrink=shrink, fixed_mask=fixed_mask,
                                     moving_mask=moving_mask, inside=inside, smoothing_sigmas=smoothing_sigmas)
        mat = as_data(mat)
        with torch.no_grad():
            L, t = mat_to_voxel(mat, dims)
        d = None
        for (ldims, f_l, m_l, ratio), fm_l, mm_l, its in zip(levels(fixed, moving, shrink, smoothing_sigmas, who), fmasks, mmasks,
                                                             kept):
            with torch.no_grad():
                state = table.per_level(m_l, f_l)
                mat_l = voxel_to_mat(_conjugate(L, ratio), scale_axes(t, ratio, divide=True), ldims)
                d = torch.zeros((N, 3, *ldims), dtype=torch.float32, device=fixed.device) if d is None else _resize_field(d, ldims)
            for _ in range(its):
                d = d.detach().requires_grad_(True)
                grid = ops.displacement_grid(d, mat_l)
                warped = align_img(grid, m_l)
                if masked:
                    sim = table.similarity(warped, f_l, state, counted_voxels(grid, fm_l, mm_l, inside))
                else:
                    sim = table.similarity(warped, f_l, state)
                (g,) = torch.autograd.grad(sim.sum(), d)
                with torch.no_grad():
                    g = ops.gaussian_smooth(g, sigma_update)
                    s = ops.displacement_step_scale(g, step)
                    d = ops.gaussian_smooth(ops.displacement_update(d.detach(), g, s), sigma_total)
        if d is None:
            raise ValueError(f"{who}: every level of shrink={shrink} has an axis under 16 voxels for {dims}")
        with torch.no_grad():
            return _resize_field(d.detach(), dims).contiguous()
