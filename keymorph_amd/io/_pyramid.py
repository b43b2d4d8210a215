"""What the multi-resolution drivers share (io.estimate_translation, io.register_intensity, and io.register_bspline and
io.register_svf through io/_deformable.py's fit_lattice): the levels of the trilinear pyramid, and how parameters are carried
between them."""
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


def levels(fixed, moving, shrink):
    """Per level (ldims, fixed_l, moving_l, ratio) of two (N, 1, D, H, W) volumes of one shape: the pair resized (trilinear, no
    graph) to ldims -- the inputs themselves, no copy, at the full size -- and ratio[k] = dims[k] / ldims[k], (z, y, x)."""
    from ..utils import resize_trilinear
    dims = tuple(fixed.shape[2:])
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
