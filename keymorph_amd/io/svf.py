"""Diffeomorphic intensity registration on the GPU: register_bspline's schedule with the control lattice read as a stationary
VELOCITY field and exponentiated by scaling and squaring (ops.svf_grid) -- the transform model of ANTs SyN and VoxelMorph's
diffeomorphic variant.  Two things follow that a free-form lattice cannot give: the map does not fold however weak the bending
penalty is (each squaring step composes a near-identity map with itself), and its inverse costs nothing: exp(-v), the grid that
carries a FIXED-space volume or label map into moving space.

Conventions.  ctrl (N, 3, Cz, Cy, Cx) is what ops.svf_grid takes: register_bspline's lattice, units and channel order, read as
velocities.  `mat` (N, 3, 4) is what ops.affine_grid takes; the grid is the matrix applied to the deformed point."""
import torch

from ._deformable import fit_lattice, metric_table
from .intensity import mat_to_voxel, voxel_to_mat


def svf_grid(ctrl, dims, mat=None, steps=6, inverse=False):
    """ops.svf_grid(ctrl, dims, steps, mat), or with inverse=True the grid of the inverse map: P + U^-(P), U^- the displacement of
    -ctrl and P the identity lattice (mat None) or ops.affine_grid of the matrix inverted in voxel space -- align_img of it
    resamples a FIXED-space volume into moving space.  The inverse is not differentiable.  Content that the forward map moves out
    of the field of view has no inverse: near the border the two do not compose to the identity."""
    from .. import fields, ops
    if not inverse:
        return ops.svf_grid(ctrl, dims, steps, mat)
    if ctrl.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("svf_grid: inverse=True is not differentiable: pass ctrl.detach() or call it under torch.no_grad()")
    with torch.no_grad():
        if mat is None:
            return ops.svf_grid(-ctrl.detach(), dims, steps)
        dims = tuple(int(n) for n in dims)
        um = ops.svf_displacement(-ctrl.detach(), dims, steps)
        L, t = mat_to_voxel(mat.detach(), dims)
        inv = ops.affine_inverse(torch.cat([L, t[:, :, None]], dim=2))
        P = ops.affine_grid(voxel_to_mat(inv[:, :, :3].contiguous(), inv[:, :, 3].contiguous(), dims), dims)
        return ops.svf_compose(um, P)


def apply_svf(x, ctrl, mat=None, steps=6, inverse=False, mode="bilinear"):
    """align_img(svf_grid(ctrl, dims, mat, steps, inverse), x, mode): x (N, C, D, H, W) resampled through the diffeomorphism (a
    moving-space volume into fixed space) or, inverse=True, through its inverse (a fixed-space volume into moving space)."""
    from ..utils import align_img
    return align_img(svf_grid(ctrl, x.shape[2:], mat, steps, inverse), x, mode)


def register_svf(fixed, moving, mat=None, control_spacing=8, bending=0.05, steps=6, bins=32, shrink=(4, 2, 1), iters=60, lr=0.1,
                 metric="mi", window=9, mind_radius=1, mind_dilation=2, fixed_mask=None, moving_mask=None, inside=False,
                 smoothing_sigmas=None):
    """ctrl (N, 3, Cz, Cy, Cx), a lattice of velocities on ops.bspline_lattice_shape(dims, control_spacing), such that
    apply_svf(moving, ctrl, mat, steps) lines up with fixed (both (N, 1, D, H, W) float32 on the GPU, of one shape).  This is
    register_bspline's schedule with ops.svf_grid(., steps) in place of ops.bspline_grid: the same pyramid, per-level units (the
    lattice is stepped in voxels of the level), Adam, bending penalty on the lattice, the metrics "mi", "lncc" and "mind", and the same
    default affine start (register_intensity) when mat is None.  The loss is a sum, so every sample is optimised on its own, and
    every kernel under it sums in a fixed or order-independent way: a batch equals its samples, bit for bit.

    fixed_mask, moving_mask, inside: which voxels the mutual information counts, as io.register_intensity takes them (the default
    affine start gets them too).  Per step the counted set is fixed_mask & (align_img(grid, moving_mask, "nearest") != 0) &
    (|grid| <= 1), of the step's own grid, and the similarity is ops.mutual_information(..., mask=that set).  They work with
    metric="mi" only: with "lncc" or "mind" any of them raises ValueError (masked local metrics do not exist here).

    smoothing_sigmas: register_bspline's (None, "auto" or one Gaussian sigma per entry of `shrink`).

    Nothing inside the loop waits for the GPU."""
    from .. import ops
    table = metric_table("register_svf", metric, bins, window, mind_radius, mind_dilation)
    if isinstance(steps, bool) or int(steps) != steps or not 0 <= int(steps) <= ops.SVF_MAX_STEPS:
        raise ValueError(f"register_svf: steps must be an integer in 0 .. {ops.SVF_MAX_STEPS}, got {steps!r}")
    return fit_lattice("register_svf", fixed, moving, mat, lambda ctrl_l, ldims, mat_l: ops.svf_grid(ctrl_l, ldims, steps, mat_l),
                       table, control_spacing, bending, bins, shrink, iters, lr, fixed_mask, moving_mask, inside, metric,
                       smoothing_sigmas)
