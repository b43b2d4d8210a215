"""What the deformable drivers share (io.register_bspline, io.register_svf; model.IntensityRegistration reads the metric table):
the fitting loop over a control lattice, and the one place that knows the similarity metrics by name.

A new transform model is a `grid_of` handed to fit_lattice; a new metric is one more arm of metric_table."""
import collections

import torch

from ._pyramid import as_data, levels, mask_levels, resolve_smoothing, scale_axes
from .intensity import _conjugate, mat_to_voxel, register_intensity, voxel_to_mat

# per_level(m_l, f_l) -> state: once per level, under no_grad, of the level's UNWARPED pair, without waiting for the GPU.
# similarity(warped, f_l, state, mask=None) -> (N,), higher is better: once per step.  mask: the step's counted voxels, given only
#     by a driver that was handed masks, and only "mi" takes one (fit_lattice refuses the others before it starts).
# reported(warped, img_f, img_m) -> (N,), or None: what model.IntensityRegistration stores under the metric's own name.
Metric = collections.namedtuple("Metric", "per_level similarity reported")


def metric_table(who, metric, bins=32, window=9, mind_radius=1, mind_dilation=2):
    """The Metric of a name; `who` goes in front of the refusal."""
    from .. import ops
    if metric not in ("mi", "lncc", "mind"):
        raise ValueError(f"{who}: metric must be 'mi', 'lncc' or 'mind', got {metric!r}")
    r, d = mind_radius, mind_dilation
    if metric == "mi":
        return Metric(lambda m_l, f_l: ops.mi_ranges(m_l, f_l, bins),
                      lambda warped, f_l, rng, mask=None: ops.mutual_information(warped, f_l, bins, ranges=rng, mask=mask),
                      None)
    if metric == "lncc":
        return Metric(lambda m_l, f_l: None,
                      lambda warped, f_l, _: ops.local_ncc(warped, f_l, window),
                      lambda warped, img_f, img_m: ops.local_ncc(warped, img_f, window))
    return Metric(lambda m_l, f_l: ops.mind_bounds(m_l, f_l, r, d),
                  lambda warped, f_l, bounds: -ops.mind_ssc_loss(warped, f_l, r, d, bounds),
                  lambda warped, img_f, img_m: ops.mind_ssc_loss(warped, img_f, r, d, ops.mind_bounds(img_m, img_f, r, d)))


def counted_voxels(grid, fixed_mask=None, moving_mask=None, inside=False):
    """(N, 1, D, H, W) bool, the voxels of the fixed lattice that a masked similarity counts for the sampling grid (N, D, H, W, 3):
    fixed_mask & (align_img(grid, moving_mask.float(), "nearest") != 0) & (grid.abs() <= 1).all(-1), each factor only if asked
    for -- ops.warp_mutual_information's definition, from the existing operators.  No graph."""
    from ..utils import align_img
    with torch.no_grad():
        grid = grid.detach()
        c = torch.ones((grid.shape[0], 1, *grid.shape[1:4]), dtype=torch.bool, device=grid.device) if fixed_mask is None \
            else fixed_mask != 0
        if moving_mask is not None:
            c = c & (align_img(grid, moving_mask.float(), "nearest") != 0)
        if inside:
            c = c & (grid.abs() <= 1).all(-1)[:, None]
        return c


def fit_lattice(who, fixed, moving, mat, grid_of, metric, control_spacing, bending, bins, shrink, iters, lr, fixed_mask=None,
                moving_mask=None, inside=False, metric_name="mi", smoothing_sigmas=None):
    """ctrl (N, 3, Cz, Cy, Cx) on ops.bspline_lattice_shape(dims, control_spacing), normalised, such that
    align_img(grid_of(ctrl, dims, mat), moving) lines up with fixed under `metric` (a Metric): the schedule the drivers' docstrings
    describe.  grid_of(ctrl_l, ldims, mat_l) -> grid (N, *ldims, 3) is the transform model, differentiable in ctrl_l.  mat None:
    register_intensity's affine answer.  fixed_mask, moving_mask, inside: register_intensity's; per step the counted set is
    counted_voxels of the step's grid (level masks as register_intensity builds them) and goes to the similarity as `mask`.  Only
    metric_name "mi" knows masks: ValueError with any other.  smoothing_sigmas: estimate_translation's, for this pyramid and for the
    affine start run here when mat is None; the metric's per-level state comes from the smoothed level pair.  Nothing inside the
    loop waits for the GPU."""
    from .. import ops
    from ..utils import align_img
    if fixed.shape != moving.shape or fixed.dim() != 5 or fixed.shape[1] != 1:
        raise ValueError(f"{who}: expected two (N, 1, D, H, W) volumes of one shape, got {tuple(fixed.shape)} and "
                         f"{tuple(moving.shape)}")
    masked = fixed_mask is not None or moving_mask is not None or bool(inside)
    if masked and metric_name != "mi":
        raise ValueError(f"{who}: fixed_mask, moving_mask and inside work with metric='mi' only, got metric={metric_name!r}")
    resolve_smoothing(who, shrink, smoothing_sigmas)
    N, dims = fixed.shape[0], tuple(fixed.shape[2:])
    if mat is not None and tuple(mat.shape) != (N, 3, 4):
        raise ValueError(f"{who}: mat must be ({N}, 3, 4), got {tuple(mat.shape)}")
    lattice = ops.bspline_lattice_shape(dims, control_spacing)
    with torch.inference_mode(False), torch.enable_grad():
        fixed, moving = as_data(fixed), as_data(moving)
        fmasks = mask_levels(who, "fixed_mask", fixed_mask, fixed, shrink)
        mmasks = mask_levels(who, "moving_mask", moving_mask, moving, shrink)
        if mat is None:
            mat = register_intensity(fixed, moving, "affine", bins=bins, shrink=shrink, fixed_mask=fixed_mask,
                                     moving_mask=moving_mask, inside=inside, smoothing_sigmas=smoothing_sigmas)
        mat = as_data(mat)
        q = torch.zeros((N, 3, *lattice), dtype=torch.float32, device=fixed.device)      # voxels of the full size, (x, y, z)
        with torch.no_grad():
            L, t = mat_to_voxel(mat, dims)
        for (ldims, f_l, m_l, ratio), fm_l, mm_l in zip(levels(fixed, moving, shrink, smoothing_sigmas, who), fmasks, mmasks):
            # ratio in (z, y, x), q's channels in (x, y, z)
            with torch.no_grad():
                state = metric.per_level(m_l, f_l)
                mat_l = voxel_to_mat(_conjugate(L, ratio), scale_axes(t, ratio, divide=True), ldims)
                q_l = scale_axes(q, [1.0 / r for r in reversed(ratio)])
            q_l.requires_grad_(True)
            to_norm = [2.0 / n for n in reversed(ldims)]
            opt = torch.optim.Adam([q_l], lr=lr)
            for _ in range(iters):
                opt.zero_grad(set_to_none=True)
                grid = grid_of(scale_axes(q_l, to_norm), ldims, mat_l)
                warped = align_img(grid, m_l)
                if masked:
                    sim = metric.similarity(warped, f_l, state, counted_voxels(grid, fm_l, mm_l, inside))
                else:
                    sim = metric.similarity(warped, f_l, state)
                loss = (bending * ops.bspline_bending(q_l) - sim).sum()
                loss.backward()
                opt.step()
            q = scale_axes(q_l.detach(), list(reversed(ratio)))
        return scale_axes(q, [2.0 / n for n in reversed(dims)])
