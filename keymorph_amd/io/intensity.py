"""Intensity-based translation / rigid / affine registration on the GPU: multi-resolution Mattes mutual information under Adam,
the baseline that the reference's scripts/register.py names `--registration_model itkelastix|ants`.  Every step is one fused
pass over the pair (ops.warp_mutual_information: neither the sampling grid nor the warped volume is stored) and a 12-number
gradient; the parameterisations below turn it into a gradient for a shift, a rotation vector or a 3 x 3 matrix.

Conventions.  A voxel-space transform (L, t) means "output voxel v reads the moving volume at c + L (v - c) + t", c = (n - 1) / 2
the volume's centre, L (N, 3, 3), t (N, 3) voxels, rows and columns in (z, y, x) order.  `mat` (N, 3, 4) is what ops.affine_grid
takes.  translate(x, t) of io.centering is the case L = I."""
import torch

from ._pyramid import as_data, levels, mask_levels, resolve_smoothing, scale_axes


def _dims3(dims):
    d = tuple(int(n) for n in dims)
    if len(d) != 3 or min(d) < 1:
        raise ValueError(f"expected three positive sizes (D, H, W), got {tuple(dims)}")
    return d


def voxel_to_mat(L, t, dims):
    """The voxel-space transform (L (N, 3, 3), t (N, 3)) as the (N, 3, 4) matrix ops.affine_grid takes for a volume of `dims`:
    mat[k][j] = L[k][j] (n_j - 1) / n_k, mat[k][3] = 2 t_k / n_k -- the linspace(-1, 1, n) base grid is (v - c) 2 / (n - 1) per
    axis and align_corners=False sampling reads at g n / 2 + c.  Plain torch on the inputs' device and dtype, differentiable, and
    built from Python scalars only (a tensor made from a host list would be a copy that waits for the stream)."""
    dims = _dims3(dims)
    if L.dim() != 3 or tuple(L.shape[1:]) != (3, 3) or tuple(t.shape) != (L.shape[0], 3):
        raise ValueError(f"voxel_to_mat: expected L (N, 3, 3) and t (N, 3), got {tuple(L.shape)} and {tuple(t.shape)}")
    rows = []
    for k, nk in enumerate(dims):
        rows.append(torch.stack([L[:, k, j] * ((nj - 1) / nk) for j, nj in enumerate(dims)] + [t[:, k] * (2.0 / nk)], dim=1))
    return torch.stack(rows, dim=1)


def mat_to_voxel(mat, dims):
    """The inverse of voxel_to_mat: (L (N, 3, 3), t (N, 3)).  Every axis needs at least two voxels."""
    dims = _dims3(dims)
    if min(dims) < 2:
        raise ValueError(f"mat_to_voxel: every axis needs at least two voxels, got {dims}")
    if mat.dim() != 3 or tuple(mat.shape[1:]) != (3, 4):
        raise ValueError(f"mat_to_voxel: expected mat (N, 3, 4), got {tuple(mat.shape)}")
    L = torch.stack([torch.stack([mat[:, k, j] * (nk / (nj - 1)) for j, nj in enumerate(dims)], dim=1)
                     for k, nk in enumerate(dims)], dim=1)
    t = torch.stack([mat[:, k, 3] * (nk / 2.0) for k, nk in enumerate(dims)], dim=1)
    return L, t


def rotation_matrix(omega):
    """R = exp([omega]x), omega (N, 3) a rotation vector (axis times angle in radians) -> (N, 3, 3), by Rodrigues' formula
    R = I + A K + B K^2, A = sin(th) / th, B = (sin(th / 2) / (th / 2))^2 / 2 (th^2 is kept above 1e-12: exact to rounding, and the
    derivative at omega = 0 is the generators')."""
    if omega.dim() != 2 or omega.shape[1] != 3:
        raise ValueError(f"rotation_matrix: expected omega (N, 3), got {tuple(omega.shape)}")
    th = (omega * omega).sum(1).clamp_min(1e-12).sqrt()
    A = torch.sin(th) / th
    B = 0.5 * (torch.sin(0.5 * th) / (0.5 * th)) ** 2
    z = torch.zeros_like(th)
    a, b, c = omega[:, 0], omega[:, 1], omega[:, 2]
    K = torch.stack([torch.stack([z, -c, b], dim=1), torch.stack([c, z, -a], dim=1), torch.stack([-b, a, z], dim=1)], dim=1)
    eye = torch.diag_embed(torch.ones_like(omega))
    return eye + A[:, None, None] * K + B[:, None, None] * (K @ K)


def _conjugate(A, spacing):
    """S^-1 A S, S = diag(spacing), from Python scalars."""
    return torch.stack([torch.stack([A[:, k, j] * (float(spacing[j]) / float(spacing[k])) for j in range(3)], dim=1)
                        for k in range(3)], dim=1)


def rigid_params_to_voxel(omega, t, spacing=(1.0, 1.0, 1.0)):
    """(L, t) of the rigid motion with rotation vector omega (N, 3) and shift t (N, 3) voxels: L = S^-1 R S, R = exp([omega]x),
    S = diag(spacing) in (z, y, x) order -- so that the motion is a rotation in millimetres also for anisotropic voxels."""
    return _conjugate(rotation_matrix(omega), spacing), t


def apply_mat(x, mat, mode="bilinear"):
    """align_img(ops.affine_grid(mat, dims), x, mode): x (N, C, D, H, W) resampled through the (N, 3, 4) matrix; mode "bilinear",
    "nearest", "cubic" or, for an integer label map, "label" (align_img)."""
    from .. import ops
    from ..utils import align_img
    return align_img(ops.affine_grid(mat, x.shape[2:]), x, mode)


_STAGES = {"translation": ("translation",), "rigid": ("translation", "rigid"), "affine": ("translation", "rigid", "affine")}


def register_intensity(fixed, moving, transform="rigid", bins=32, shrink=(4, 2, 1), iters=30, lr=0.25, spacing=(1.0, 1.0, 1.0),
                       fixed_mask=None, moving_mask=None, inside=False, smoothing_sigmas=None):
    """mat (N, 3, 4), the argument ops.affine_grid takes, such that apply_mat(moving, mat) lines up with fixed (both
    (N, 1, D, H, W) float32 on the GPU, of one shape) under mutual information; transform = "translation" | "rigid" | "affine",
    spacing = voxel size in (z, y, x) order.

    Stages, as in elastix / ANTs, each started from the previous one's answer: the difference of the intensity centroids (as
    estimate_translation), then translation, then (if asked) rigid, then (if asked) affine.  Every stage runs over the trilinear
    pyramid (size // shrink per level; a level with an axis shorter than 16 is skipped) with `iters` Adam steps per level on
    -sum_n ops.warp_mutual_information(moving_l, fixed_l, mat_l): the loss is a sum, so every sample is optimised on its own.
    The intensity ranges come from ops.mi_ranges once per level.

    Scaling of the parameters: the shift is stepped in voxels of the level.  The rotation vector and, in the affine stage, the
    entries of the physical matrix A (L = S^-1 A S) are stepped as omega * h and A * h, h = the level's largest half-extent
    max_k spacing_k (n_k - 1) / 2 in units of its smallest spacing: a unit step of such a parameter moves the farthest face of
    the volume by about one voxel, like a unit step of the shift, so the one learning rate `lr` (voxels per step) serves all.

    fixed_mask, moving_mask ((N, 1, D, H, W) uint8 or bool on the GPU, non-zero = counted), inside: which voxels the mutual
    information counts, as ops.warp_mutual_information defines it (elastix' FixedMask / MovingMask, ANTs' -x; inside=True drops
    samples that the transform sends outside the moving volume, as ITK does).  The centroid start is that of fixed * fixed_mask
    and moving * moving_mask.  A mask's pyramid is the mask itself at the full size and resize_trilinear(mask.float()) >= 0.5
    below, built once per level; the intensity ranges stay those of the whole level volumes.  A sample whose level mask is empty
    does not move at that level.

    smoothing_sigmas: None, "auto" or one Gaussian sigma per entry of `shrink` (full-resolution voxels), as
    estimate_translation takes it: the level pair is smoothed before it is resized, and the intensity ranges are those of the
    smoothed level pair.  The masks' pyramids do not change.

    Nothing inside the loop waits for the GPU."""
    from .. import ops
    from .centering import _centroid
    if transform not in _STAGES:
        raise ValueError(f"register_intensity: transform must be one of {sorted(_STAGES)}, got {transform!r}")
    if fixed.shape != moving.shape or fixed.dim() != 5 or fixed.shape[1] != 1:
        raise ValueError(f"register_intensity: expected two (N, 1, D, H, W) volumes of one shape, got {tuple(fixed.shape)} and "
                         f"{tuple(moving.shape)}")
    spacing = tuple(float(s) for s in spacing)
    if len(spacing) != 3 or min(spacing) <= 0:
        raise ValueError(f"register_intensity: spacing must be three positive numbers, got {spacing}")
    resolve_smoothing("register_intensity", shrink, smoothing_sigmas)
    dims = tuple(fixed.shape[2:])
    with torch.inference_mode(False), torch.enable_grad():
        fixed, moving = as_data(fixed), as_data(moving)
        fmasks = mask_levels("register_intensity", "fixed_mask", fixed_mask, fixed, shrink)
        mmasks = mask_levels("register_intensity", "moving_mask", moving_mask, moving, shrink)
        pyramid = []
        with torch.no_grad():
            if fixed_mask is None and moving_mask is None:
                t = _centroid(moving) - _centroid(fixed)
            else:                                              # an empty mask has no centroid: that sample starts at 0
                t = _centroid(moving if moving_mask is None else moving * moving_mask) \
                    - _centroid(fixed if fixed_mask is None else fixed * fixed_mask)
                for mask in (fixed_mask, moving_mask):
                    if mask is not None:
                        t = torch.where((mask != 0).flatten(1).any(1, keepdim=True), t, torch.zeros_like(t))
            pairs = levels(fixed, moving, shrink, smoothing_sigmas, "register_intensity")
            for (ldims, f_l, m_l, ratio), fm_l, mm_l in zip(pairs, fmasks, mmasks):
                sp = [s * r for s, r in zip(spacing, ratio)]
                h = max(s * (n - 1) / 2 for s, n in zip(sp, ldims)) / min(sp)
                pyramid.append((ldims, f_l, m_l, ops.mi_ranges(m_l, f_l, bins), ratio, sp, h, fm_l, mm_l))
        omega = torch.zeros_like(t)
        A = None
        for stage in _STAGES[transform]:
            if stage == "affine":
                A = rotation_matrix(omega).detach()
            for ldims, f_l, m_l, rng, ratio, sp, h, fm_l, mm_l in pyramid:
                t_l = scale_axes(t, ratio, divide=True).requires_grad_(True)
                params = [t_l]
                if stage == "translation":                     # L does not move in this stage: once per level, no graph
                    with torch.no_grad():
                        L_fixed = _conjugate(rotation_matrix(omega), sp)
                elif stage == "rigid":
                    q = (omega * h).requires_grad_(True)
                    params.append(q)
                elif stage == "affine":
                    q = (A * h).requires_grad_(True)
                    params.append(q)

                def level_mat():
                    if stage == "translation":
                        L = L_fixed
                    elif stage == "rigid":
                        L = _conjugate(rotation_matrix(q / h), sp)
                    else:
                        L = _conjugate(q / h, sp)
                    return voxel_to_mat(L, t_l, ldims)
                opt = torch.optim.Adam(params, lr=lr)
                for _ in range(iters):
                    opt.zero_grad(set_to_none=True)
                    loss = -ops.warp_mutual_information(m_l, f_l, level_mat(), bins, rng, fm_l, mm_l, inside).sum()
                    loss.backward()
                    opt.step()
                t = scale_axes(t_l.detach(), ratio)
                if stage == "rigid":
                    omega = q.detach() / h
                elif stage == "affine":
                    A = q.detach() / h
        with torch.no_grad():
            L = _conjugate(rotation_matrix(omega) if A is None else A, spacing)
            return voxel_to_mat(L, t, dims)


def estimate_rigid(fixed, moving, **kwargs):
    """register_intensity(fixed, moving, "rigid", ...)."""
    return register_intensity(fixed, moving, "rigid", **kwargs)


def estimate_affine(fixed, moving, **kwargs):
    """register_intensity(fixed, moving, "affine", ...)."""
    return register_intensity(fixed, moving, "affine", **kwargs)
