"""What the multi-resolution drivers share (io.estimate_translation, io.register_intensity, and io.register_bspline and
io.register_svf through io/_deformable.py's fit_lattice, io.register_greedy): the levels of the trilinear pyramid, and how parameters
are carried between them."""
import torch

MIN_AXIS = 16      # a level with a shorter axis is skipped


def level_dims(dims, shrink):
    """The sizes of the pyramid's levels, in the order of `shrink`: size // shrink per axis, levels with an axis under MIN_AXIS
    dropped."""
    out = []
    for sh in shrink:
        ldims = tuple(int(n) // int(sh) for n in dims)
        if min(ldims) >= MIN_AXIS:
            out.append(ldims)
    return out


def resolve_smoothing(who, shrink, smoothing):
    """The per-level Gaussian sigmas of a pyramid, one entry per entry of `shrink`, or None.  smoothing: None (no smoothing: the
    pyramid of before), "auto" (sigma = shrink / 2 per level, 0 at shrink 1 -- the ANTs / elastix habit), or a sequence of
    len(shrink) entries, each a number or a (z, y, x) triple >= 0 in voxels of the FULL-resolution volume.  ValueError naming
    `who` for anything else."""
    from .. import ops
    if smoothing is None:
        return None
    shrink = tuple(shrink)
    if isinstance(smoothing, str):
        if smoothing != "auto":
            raise ValueError(f"{who}: smoothing_sigmas must be None, 'auto' or one entry per pyramid level, got {smoothing!r}")
        return tuple(0.0 if int(sh) <= 1 else int(sh) / 2.0 for sh in shrink)
    try:
        entries = tuple(smoothing)
    except TypeError:
        raise ValueError(f"{who}: smoothing_sigmas must be None, 'auto' or one entry per pyramid level, got {smoothing!r}") from None
    if len(entries) != len(shrink):
        raise ValueError(f"{who}: smoothing_sigmas has {len(entries)} entries for the {len(shrink)} levels of shrink={shrink}")
    out = []
    for e in entries:
        sig = ops._gauss_sigmas(who, e, 4.0)
        out.append(float(e) if isinstance(e, (int, float)) else sig)
    return tuple(out)


def level_entries(dims, shrink, entries):
    """Of one entry per entry of `shrink`, those of the levels level_dims(dims, shrink) keeps (a dropped level drops its entry)."""
    return [e for sh, e in zip(shrink, entries) if min(int(n) // int(sh) for n in dims) >= MIN_AXIS]


def level_smoothing(who, dims, shrink, smoothing):
    """resolve_smoothing's entries for the levels level_dims(dims, shrink) keeps (a dropped level drops its entry); None: None."""
    sig = resolve_smoothing(who, shrink, smoothing)
    if sig is None:
        return None
    return level_entries(dims, shrink, sig)


def levels(fixed, moving, shrink, smoothing=None, who="levels"):
    """Per level (ldims, fixed_l, moving_l, ratio) of two (N, 1, D, H, W) volumes of one shape: the pair resized (trilinear, no
    graph) to ldims -- the inputs themselves, no copy, at the full size -- and ratio[k] = dims[k] / ldims[k], (z, y, x).
    smoothing (resolve_smoothing; `who` is named in its errors): level l is resize_trilinear(ops.gaussian_smooth(v, sigma_l),
    ldims), smoothed at the full resolution before it shrinks; with sigma_l = 0 at the full size it is still the input itself."""
    from ..utils import resize_trilinear
    dims = tuple(fixed.shape[2:])
    if smoothing is not None:
        from .. import ops
        sigmas = level_smoothing(who, dims, shrink, smoothing)
        for ldims, sigma in zip(level_dims(dims, shrink), sigmas):
            with torch.no_grad():
                f_l, m_l = ops.gaussian_smooth(fixed, sigma), ops.gaussian_smooth(moving, sigma)
                if ldims != dims:
                    f_l, m_l = resize_trilinear(f_l, size=ldims), resize_trilinear(m_l, size=ldims)
            yield ldims, f_l, m_l, [n / l for n, l in zip(dims, ldims)]
        return
    for ldims in level_dims(dims, shrink):
        if ldims == dims:
            f_l, m_l = fixed, moving
        else:
            with torch.no_grad():
                f_l, m_l = resize_trilinear(fixed, size=ldims), resize_trilinear(moving, size=ldims)
        yield ldims, f_l, m_l, [n / l for n, l in zip(dims, ldims)]


def mask_levels(who, name, mask, like, shrink):
    """The pyramid of a mask of `like`'s shape (uint8 or bool on the GPU, non-zero = counted; else ValueError), one uint8 tensor per
    level of levels(like, ., shrink): the mask itself at the full size, resize_trilinear(mask.float(), ldims) >= 0.5 below.  None
    for every level when mask is None.  Built once, under no_grad, without waiting for the GPU."""
    from .. import ops
    from ..utils import resize_trilinear
    dims = tuple(like.shape[2:])
    sizes = level_dims(dims, shrink)
    if mask is None:
        return [None] * len(sizes)
    mask = ops._need_mask(who, name, mask, like)
    with torch.no_grad():
        soft = mask.float() if any(ldims != dims for ldims in sizes) else None
        return [mask if ldims == dims else (resize_trilinear(soft, size=ldims) >= 0.5).to(torch.uint8) for ldims in sizes]


def scale_axes(t, factors, divide=False):
    """t (N, 3, ...) with channel k times factors[k] (divide: over factors[k]).  From Python scalars only: a tensor made from a
    host list would be a host-to-device copy, which waits for the stream, on every step of a driver's loop."""
    if divide:
        return torch.stack([t[:, k] / float(factors[k]) for k in range(3)], dim=1)
    return torch.stack([t[:, k] * float(factors[k]) for k in range(3)], dim=1)


def as_data(x):
    """x without its graph, usable under autograd also when it was made in inference mode (then: a copy)."""
    return x.clone() if x.is_inference() else x.detach()
