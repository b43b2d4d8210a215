"""The centering step of the reference's README ([C], notebooks/[C] Centering.ipynb) on the GPU: a subject's T1 / PD is
translated onto the same subject's T2 by a mutual-information translation registration of the masked volumes, and the
translation is applied to the unmasked image (linear) and to the mask (nearest).  The notebook does this with ANTs and
SimpleITK; here it is ops.mutual_information under Adam, over a trilinear pyramid."""
import torch

from ._pyramid import levels, resolve_smoothing, scale_axes


def translate(x, t, mode="bilinear"):
    """x (N, C, D, H, W) shifted by t (N, 3) voxels in (z, y, x) order: out[v] = x[v + t], border values outside; differentiable in
    t (and in x for "bilinear"; "cubic" is the cubic B-spline of ops.cubic_sample, for the image that is kept; "label" is
    ops.warp_labels on an integer label map, no gradient).  A pure voxel shift
    through ops.affine_grid and align_img: the matrix diag((n - 1) / n) cancels the linspace(-1, 1) base grid against
    align_corners=False sampling (a translation alone would also zoom by (n - 1) / n), and the offsets are 2 t / n."""
    from .. import ops
    from ..utils import align_img
    if x.dim() != 5 or t.dim() != 2 or tuple(t.shape) != (x.shape[0], 3):
        raise ValueError(f"translate: expected x (N, C, D, H, W) and t (N, 3), got {tuple(x.shape)} and {tuple(t.shape)}")
    if mode not in ("bilinear", "nearest", "cubic", "label"):
        raise ValueError(f"translate: mode must be 'bilinear', 'nearest', 'cubic' or 'label', got {mode!r}")
    # the matrix from Python scalars only (scale_axes says why): this runs on every step of estimate_translation's loop
    t = t.float()
    lin = t.new_zeros((x.shape[0], 3, 3))
    for k, n in enumerate(x.shape[2:]):
        lin[:, k, k] = (n - 1) / n
    off = scale_axes(t, [2.0 / n for n in x.shape[2:]])
    mat = torch.cat([lin, off.unsqueeze(-1)], dim=2)
    return align_img(ops.affine_grid(mat, x.shape[2:]), x, mode)


def _centroid(x):
    """Intensity centroid of (N, 1, D, H, W) in voxels, (N, 3) in (z, y, x) order (ops.com3d: negative values count as 0)."""
    from .. import ops
    c = ops.com3d(x)[:, 0]
    return torch.stack([(c[:, k] + 1.0) * (0.5 * (n - 1)) for k, n in enumerate(x.shape[2:])], dim=1)


def estimate_translation(fixed, moving, bins=32, shrink=(4, 2, 1), iters=30, lr=0.25, smoothing_sigmas=None):
    """t (N, 3) voxels, (z, y, x), such that translate(moving, t) lines up with fixed (both (N, 1, D, H, W) float32 on the GPU, of
    one shape) under mutual information.  Start: the difference of the two intensity centroids.  Then, per pyramid level
    (size // shrink by trilinear resize; a level with an axis shorter than 16 is skipped), `iters` Adam steps of size `lr` voxels
    of that level on -MI(translate(moving_l, t_l), fixed_l); t is carried from level to level in full-resolution voxels.  Every
    sample is optimised on its own (the loss is the sum over the batch); nothing inside the loop waits for the GPU.
    smoothing_sigmas: None (the plain trilinear pyramid), "auto" (shrink / 2 per level, 0 at shrink 1) or one Gaussian sigma per
    entry of `shrink`, a number or a (z, y, x) triple in full-resolution voxels: each level is ops.gaussian_smooth'ed at the full
    size before it is resized (io/_pyramid.py), as ANTs' --smoothing-sigmas and elastix' pyramid schedules do -- what noisy
    volumes need at shrink 4, where the trilinear resize alone reads two voxels in four."""
    from .. import ops
    if fixed.shape != moving.shape or fixed.dim() != 5 or fixed.shape[1] != 1:
        raise ValueError(f"estimate_translation: expected two (N, 1, D, H, W) volumes of one shape, got {tuple(fixed.shape)} and "
                         f"{tuple(moving.shape)}")
    resolve_smoothing("estimate_translation", shrink, smoothing_sigmas)      # refused before any work
    fixed, moving = fixed.detach(), moving.detach()
    with torch.no_grad():
        t = _centroid(moving) - _centroid(fixed)
    for _, f_l, m_l, ratio in levels(fixed, moving, shrink, smoothing_sigmas, "estimate_translation"):
        t_l = scale_axes(t, ratio, divide=True).requires_grad_(True)
        opt = torch.optim.Adam([t_l], lr=lr)
        for _ in range(iters):
            opt.zero_grad(set_to_none=True)
            loss = -ops.mutual_information(translate(m_l, t_l), f_l, bins).sum()
            loss.backward()
            opt.step()
        t = scale_axes(t_l.detach(), ratio)
    return t


def center_to(fixed, fixed_mask, moving, moving_mask, **kwargs):
    """The notebook's cell: the translation is estimated on fixed * fixed_mask and moving * moving_mask, then applied to the
    unmasked moving image ("bilinear") and to its mask ("nearest") -> (aligned_moving, aligned_mask, t); the mask comes back in
    its input dtype.  kwargs go to estimate_translation."""
    t = estimate_translation(fixed.float() * fixed_mask.to(torch.float32), moving.float() * moving_mask.to(torch.float32),
                             **kwargs)
    with torch.no_grad():
        aligned = translate(moving.float(), t, "bilinear")
        mask = translate(moving_mask.to(torch.float32), t, "nearest").to(moving_mask.dtype)
    return aligned, mask, t
