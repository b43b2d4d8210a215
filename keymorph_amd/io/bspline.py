"""Deformable intensity registration on the GPU: a cubic B-spline free-form deformation (ops.bspline_grid) on top of an affine
matrix, fitted by multi-resolution Mattes mutual information under Adam with a bending penalty on the control lattice -- the
deformable counterpart of io.register_intensity, what elastix and ANTs are used for beside KeyMorph's thin-plate splines.

Conventions.  ctrl (N, 3, Cz, Cy, Cx) is what ops.bspline_grid takes: channel k is the displacement of grid component k, in the
grid's order (x, y, z) and normalised units, on the lattice ops.bspline_lattice_shape(dims, control_spacing).  Normalised
displacements on a normalised lattice mean the same thing at every pyramid level, so ONE parameter tensor serves all levels
without refitting; per level it is stepped in that level's voxels (q_l = ctrl (W_l, H_l, D_l) / 2), so that the learning rate and
the bending weight are in voxels as register_intensity's are.  `mat` (N, 3, 4) is what ops.affine_grid takes."""
from ._deformable import fit_lattice, metric_table


def apply_bspline(x, ctrl, mat=None, mode="bilinear"):
    """align_img(ops.bspline_grid(ctrl, dims, mat), x, mode): x (N, C, D, H, W) resampled through the free-form deformation."""
    from .. import ops
    from ..utils import align_img
    return align_img(ops.bspline_grid(ctrl, x.shape[2:], mat), x, mode)


def register_bspline(fixed, moving, mat=None, control_spacing=8, bending=0.05, bins=32, shrink=(4, 2, 1), iters=60, lr=0.1,
                     metric="mi", window=9, mind_radius=1, mind_dilation=2, fixed_mask=None, moving_mask=None,
                     inside=False, smoothing_sigmas=None):
    """ctrl (N, 3, Cz, Cy, Cx) on the lattice ops.bspline_lattice_shape(dims, control_spacing) such that
    apply_bspline(moving, ctrl, mat) lines up with fixed (both (N, 1, D, H, W) float32 on the GPU, of one shape) under mutual
    information.  mat (N, 3, 4): the affine part, data; None: register_intensity(fixed, moving, "affine", bins=bins,
    shrink=shrink) is run first (read it back from there if you need it, or pass your own).

    Over the trilinear pyramid (size // shrink per level; a level with an axis shorter than 16 is skipped) `iters` Adam steps per
    level, `lr` in voxels of the level, on
        sum_n [ -mutual_information(align_img(bspline_grid(ctrl_l, ldims, mat_l), m_l), f_l, bins, ranges)
                + bending * bspline_bending(q_l) ],
    q_l the control displacements in voxels of the level (it starts at the previous level's answer), ctrl_l = q_l (2 / W_l,
    2 / H_l, 2 / D_l), mat_l the matrix of the same voxel-space map at the level's size, and the intensity ranges from
    ops.mi_ranges once per level.  The loss is a sum, so every sample is optimised on its own.  The penalty is what keeps the
    border control points, which see few voxels, from chasing interpolation blur.

    metric="lncc": the similarity is ops.local_ncc(warped, f_l, window) instead of the mutual information (no ranges are
    computed): the local metric of ANTs and VoxelMorph, for one modality under a smooth bias field, which a global histogram
    cannot see.  The default affine start stays register_intensity's.

    metric="mind": the similarity is -ops.mind_ssc_loss(warped, f_l, mind_radius, mind_dilation, bounds), the MIND-SSC
    self-similarity context distance: a local metric for two modalities (MR to CT, T1 to T2 under a coil bias).  `bounds`, the
    clamp of the descriptor's variance, is ops.mind_bounds(m_l, f_l, ...) of the level's unwarped pair, once per level, where the
    mutual information has its ranges.

    fixed_mask, moving_mask, inside: which voxels the mutual information counts, as io.register_intensity takes them (the default
    affine start gets them too).  Per step the counted set is fixed_mask & (align_img(grid, moving_mask, "nearest") != 0) &
    (|grid| <= 1), of the step's own grid, and the similarity is ops.mutual_information(..., mask=that set).  They work with
    metric="mi" only: with "lncc" or "mind" any of them raises ValueError (masked local metrics do not exist here).

    smoothing_sigmas: None, "auto" or one Gaussian sigma per entry of `shrink`, as io.estimate_translation takes it: every level
    pair is smoothed at the full size before it is resized (the default affine start gets it too), and the ranges / bounds come
    from the smoothed pair.

    Nothing inside the loop waits for the GPU."""
    from .. import ops
    table = metric_table("register_bspline", metric, bins, window, mind_radius, mind_dilation)
    return fit_lattice("register_bspline", fixed, moving, mat, ops.bspline_grid, table, control_spacing, bending, bins, shrink,
                       iters, lr, fixed_mask, moving_mask, inside, metric, smoothing_sigmas)
