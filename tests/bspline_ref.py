"""The definitions of keymorph_amd.ops.bspline_grid and ops.bspline_bending restated in plain torch (dtype-generic: fp64 for the
yardstick, fp32 for the size of fp32's own error), a pair deformed by a known smooth lattice, and the schedule of
keymorph_amd.io.register_bspline rebuilt from F.grid_sample, F.interpolate and tests/mi_ref.py.

Per axis of S voxels and C control points: voxel centre g = (2 i + 1) / S - 1, u = (g + 1) (C - 3) / 2,
cell = clamp(floor(u), 0, C - 4), t = u - cell, weights B0 = (1 - t)^3 / 6, B1 = (3 t^3 - 6 t^2 + 4) / 6,
B2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6, B3 = t^3 / 6 on control points cell .. cell + 3: a basis matrix (S, C).
grid[n, z, y, x, k] = base[n, z, y, x, k] + sum_{c,b,a} Bz[z, c] By[y, b] Bx[x, a] ctrl[n, k, c, b, a], k in the grid's order
(x, y, z); base = the voxel-centre lattice, or ops.affine_grid's formula (tests/warp_mi_ref.py::grid_of) for a matrix."""
import functools

import torch
import torch.nn.functional as F

from tests import mi_ref
from tests import warp_mi_ref as W

F64 = torch.float64


def lattice_shape(shape, spacing):
    return tuple(-(-int(n) // int(spacing)) + 3 for n in shape)


def basis(S, C, dtype=F64):
    """(S, C): row i holds the four weights of voxel i."""
    i = torch.arange(S, dtype=dtype)
    g = (2 * i + 1) / S - 1
    u = (g + 1) * (C - 3) / 2
    cell = torch.floor(u).clamp(0, C - 4)
    t = u - cell
    w = torch.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6],
                    dim=1)
    k = cell.long()[:, None] + torch.arange(4)[None, :]
    return torch.zeros(S, C, dtype=dtype).scatter(1, k, w)


def basis_at(S, C, i, cell, dtype=F64):
    """The four weights of voxel i taken in a GIVEN cell (C2 continuity: on a knot either neighbour gives the same value)."""
    u = torch.tensor(((2 * i + 1) / S - 1 + 1) * (C - 3) / 2, dtype=dtype)
    t = u - cell
    w = torch.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6])
    return torch.zeros(C, dtype=dtype).scatter(0, cell + torch.arange(4), w)


def identity(dims, dtype=F64):
    """(D, H, W, 3) in (x, y, z): the voxel centres, fields.identity_grid."""
    ax = [(2 * torch.arange(n, dtype=dtype) + 1) / n - 1 for n in dims]
    z, y, x = torch.meshgrid(*ax, indexing="ij")
    return torch.stack([x, y, z], dim=-1)


def displacement(ctrl, dims):
    """(N, D, H, W, 3): the spline alone, in ctrl's dtype."""
    Bz, By, Bx = (basis(S, C, ctrl.dtype) for S, C in zip(dims, ctrl.shape[2:]))
    return torch.einsum("zc,yb,xa,nkcba->nzyxk", Bz, By, Bx, ctrl)


def bspline_grid(ctrl, dims, mat=None):
    dims = tuple(int(n) for n in dims)
    base = identity(dims, ctrl.dtype)[None] if mat is None else W.grid_of(mat.to(ctrl.dtype), dims)
    return base + displacement(ctrl, dims)


def bending(q):
    """(N,): sum over the lattice axes of the mean of the squared second differences."""
    out = 0
    for a in (2, 3, 4):
        n = q.shape[a] - 2
        d = q.narrow(a, 0, n) - 2 * q.narrow(a, 1, n) + q.narrow(a, 2, n)
        out = out + d.pow(2).mean(dim=(1, 2, 3, 4))
    return out


def evaluate_grid(ctrl, dims, mat, cot, dtype):
    """(grid, d (grid * cot).sum() / d ctrl) of float32 inputs evaluated in `dtype` on the CPU."""
    c = ctrl.detach().cpu().to(dtype).requires_grad_(True)
    g = bspline_grid(c, dims, None if mat is None else mat.detach().cpu().to(dtype))
    (dc,) = torch.autograd.grad((g * cot.detach().cpu().to(dtype)).sum(), c)
    return g.detach(), dc


def evaluate_bending(q, cot, dtype):
    x = q.detach().cpu().to(dtype).requires_grad_(True)
    b = bending(x)
    (dq,) = torch.autograd.grad((b * cot.detach().cpu().to(dtype)).sum(), x)
    return b.detach(), dq


# ---- the recovery pair ------------------------------------------------------------------------------------------------------------
SIZE, SPACING, SEED, TEXTURE_SEED, AMPLITUDE = 32, 8, 3, 5, 4.0


@functools.lru_cache(maxsize=None)
def true_ctrl(seed=SEED, size=SIZE):
    """(1, 3, 7, 7, 7) fp64, normalised: a 3^3 random lattice in [-1, 1] interpolated to 7^3, times AMPLITUDE voxels."""
    c = 2 * torch.rand(1, 3, 3, 3, 3, dtype=F64, generator=torch.Generator().manual_seed(seed)) - 1
    lat = lattice_shape((size,) * 3, SPACING)
    return F.interpolate(c, lat, mode="trilinear", align_corners=True) * AMPLITUDE * 2 / size


@functools.lru_cache(maxsize=None)
def recovery_pair(seed=SEED, size=SIZE):
    """(fixed, moving), (1, 1, size, size, size) float32: moving(v) = remap(texture(v)), fixed(v) = texture(T(v)) with T(v) the voxel
    bspline_grid(true_ctrl) points at -- so apply_bspline(moving, true_ctrl) lines up with fixed.  texture = the dense Gaussians of
    warp_mi_ref._field_at rescaled by their range on the voxel centres, remap = the non-monotone map of warp_mi_ref.moved_pair."""
    dims = (size,) * 3
    v = torch.stack(torch.meshgrid(*[torch.arange(d, dtype=F64) for d in dims], indexing="ij"), dim=-1)
    raw = W._field_at(size, TEXTURE_SEED, v, dense=True)
    lo, hi = raw.min(), raw.max()
    g = bspline_grid(true_ctrl(seed, size), dims)[0].flip(-1)              # (z, y, x)
    T = ((g + 1) * size - 1) / 2
    fixed = ((W._field_at(size, TEXTURE_SEED, T, dense=True) - lo) / (hi - lo)).clamp(0, 1)

    def remap(x):
        return 0.8 * (1 - x) ** 2 + 0.2 * torch.sin(6 * x) ** 2
    table = remap(torch.linspace(0, 1, 4097, dtype=F64))
    rlo, rhi = table.min(), table.max()
    moving = ((remap((raw - lo) / (hi - lo)) - rlo) / (rhi - rlo)).clamp(0, 1)
    return fixed[None, None].float(), moving[None, None].float()


def identity_mat(n, dims):
    return W.voxel_to_mat(torch.eye(3, dtype=F64)[None].expand(n, 3, 3), torch.zeros(n, 3, dtype=F64), dims)


def displacement_error(ctrl, truth, dims):
    """Per sample, the mean over the voxel lattice of |estimated - true| displacement, in voxels."""
    d = displacement(ctrl.detach().cpu().to(F64) - truth.to(F64), dims)
    half = torch.tensor([dims[2] / 2, dims[1] / 2, dims[0] / 2], dtype=F64)
    return (d * half).norm(dim=-1).mean(dim=(1, 2, 3))


# ---- the driver's schedule ------------------------------------------------------------------------------------------------------
def mi_similarity(warped, f_l, level):
    """The mutual information of register_bspline's default metric; the ranges are the level's own pair's, found once."""
    if "ranges" not in level:
        level["ranges"] = W.own_ranges(level["moving"], f_l)
    return torch.stack([mi_ref.mi_sample(warped[k], f_l[k], level["bins"], *level["ranges"][k]) for k in range(len(warped))])


def register(fixed, moving, mat, control_spacing=8, bending_weight=0.05, bins=32, shrink=(4, 2, 1), iters=60, lr=0.1,
             dtype=F64, similarity=mi_similarity, grid_of=bspline_grid):
    """keymorph_amd.io.register_bspline with a given matrix, on the CPU in `dtype`: the same levels, parameters, loss and Adam.
    similarity(warped, f_l, level) -> (N,), higher is better; level = {"moving": m_l, "bins": bins}, a dict of the level's own
    that the callable may keep things in.  grid_of(ctrl_l, ldims, mat_l) -> grid: the transform model (svf_ref.register's differs)."""
    fixed, moving, mat = fixed.detach().to(dtype), moving.detach().to(dtype), mat.detach().to(F64)
    N, dims = fixed.shape[0], tuple(fixed.shape[2:])
    n = torch.tensor([float(d) for d in dims], dtype=F64)
    L = mat[:, :, :3] * n[None, :, None] / (n - 1)[None, None, :]
    t = mat[:, :, 3] * n[None, :] / 2
    q = torch.zeros((N, 3, *lattice_shape(dims, control_spacing)), dtype=dtype)
    for sh in shrink:
        ldims = tuple(d // int(sh) for d in dims)
        if min(ldims) < 16:
            continue
        if ldims == dims:
            f_l, m_l = fixed, moving
        else:
            f_l = F.interpolate(fixed, size=ldims, mode="trilinear", align_corners=False)
            m_l = F.interpolate(moving, size=ldims, mode="trilinear", align_corners=False)
        level = {"moving": m_l, "bins": bins}
        ratio = torch.tensor([d / l for d, l in zip(dims, ldims)], dtype=F64)
        mat_l = W.voxel_to_mat(L * ratio[None, None, :] / ratio[None, :, None], t / ratio[None, :], ldims).to(dtype)
        rx = ratio.flip(0).to(dtype)[None, :, None, None, None]
        to_norm = torch.tensor([2.0 / ldims[2], 2.0 / ldims[1], 2.0 / ldims[0]], dtype=dtype)[None, :, None, None, None]
        q_l = (q / rx).requires_grad_(True)
        opt = torch.optim.Adam([q_l], lr=lr)
        for _ in range(iters):
            opt.zero_grad(set_to_none=True)
            warped = F.grid_sample(m_l, grid_of(q_l * to_norm, ldims, mat_l), mode="bilinear", padding_mode="border",
                                   align_corners=False)
            (bending_weight * bending(q_l) - similarity(warped, f_l, level)).sum().backward()
            opt.step()
        q = q_l.detach() * rx
    return q * torch.tensor([2.0 / dims[2], 2.0 / dims[1], 2.0 / dims[0]], dtype=dtype)[None, :, None, None, None]


@functools.lru_cache(maxsize=None)
def recovery_run(dtype=F64):
    """(residual, identity error) in voxels of the restated driver on the recovery pair, defaults, identity matrix."""
    fixed, moving = recovery_pair()
    dims = tuple(fixed.shape[2:])
    ctrl = register(fixed, moving, identity_mat(1, dims), dtype=dtype)
    truth = true_ctrl()
    return float(displacement_error(ctrl, truth, dims)[0]), float(displacement_error(torch.zeros_like(truth), truth, dims)[0])
