"""The definition of keymorph_amd.ops.warp_mutual_information restated in plain torch (dtype-generic: fp64 for the yardstick,
fp32 for the size of fp32's own error): the matrix -> grid formula of ops.affine_grid, F.grid_sample(bilinear, border,
align_corners=False), then tests/mi_ref.py's mutual information with both ranges FIXED to the volumes' own minima and maxima.
Also: voxel_to_mat restated, the accumulation format's floor for the matrix gradient, and recovery pairs moved by a known
rigid / affine motion.

Per sample:  grid[z, y, x] = flip(mat [lin_z, lin_y, lin_x, 1]), lin_k = linspace(-1, 1, n_k), rows of mat = (z, y, x) outputs,
flipped to the (x, y, z) order of grid_sample;  a = grid_sample(moving, grid);  MI(a, fixed) with range_a = (min, max) of moving
and range_b = (min, max) of fixed."""
import math

import torch
import torch.nn.functional as F

from tests import mi_ref

F64 = torch.float64
Q = 2.0 ** -24                      # half a quantum of one fixed-point window product (csrc/mi.hip)


def base_points(dims, dtype=F64):
    """(D, H, W, 4): (lin_z, lin_y, lin_x, 1) per voxel."""
    axes = [torch.linspace(-1, 1, n, dtype=dtype) if n > 1 else torch.ones(1, dtype=dtype) for n in dims]
    z, y, x = torch.meshgrid(*axes, indexing="ij")
    return torch.stack([z, y, x, torch.ones_like(z)], dim=-1)


def grid_of(mat, dims):
    """mat (N, 3, 4) -> (N, D, H, W, 3) in (x, y, z) order, in mat's dtype."""
    p = base_points(dims, mat.dtype)
    return torch.einsum("nrk,dhwk->ndhwr", mat, p).flip(-1)


def warp(moving, mat):
    return F.grid_sample(moving, grid_of(mat, moving.shape[2:]), mode="bilinear", padding_mode="border", align_corners=False)


def own_ranges(moving, fixed):
    """Per sample ((lo_a, hi_a), (lo_b, hi_b)) as Python floats: the volumes' own minima and maxima."""
    return [((float(moving[n].min()), float(moving[n].max())), (float(fixed[n].min()), float(fixed[n].max())))
            for n in range(moving.shape[0])]


def warp_mi(moving, fixed, mat, bins=32, ranges=None):
    """(N,) in the inputs' dtype; ranges as own_ranges returns them (None: computed from the inputs)."""
    ranges = ranges or own_ranges(moving, fixed)
    a = warp(moving, mat)
    return torch.stack([mi_ref.mi_sample(a[n], fixed[n], bins, ranges[n][0], ranges[n][1]) for n in range(a.shape[0])])


def evaluate(moving, fixed, mat, bins=32, dtype=F64, ranges=None):
    """(MI (N,), d MI.sum() / d mat (N, 3, 4)) of float32 inputs evaluated in `dtype` on the CPU; the ranges are those of the
    float32 volumes either way."""
    ranges = ranges or own_ranges(moving, fixed)
    m = mat.detach().cpu().to(dtype).requires_grad_(True)
    mi = warp_mi(moving.detach().cpu().to(dtype), fixed.detach().cpu().to(dtype), m, bins, ranges)
    (g,) = torch.autograd.grad(mi.sum(), m)
    return mi.detach(), g


def voxel_to_mat(L, t, dims):
    """mat[k][j] = L[k][j] (n_j - 1) / n_k, mat[k][3] = 2 t_k / n_k in fp64."""
    n = torch.tensor([float(d) for d in dims], dtype=F64)
    lin = L.to(F64) * (n - 1)[None, None, :] / n[None, :, None]
    return torch.cat([lin, (2 * t.to(F64) / n[None, :])[:, :, None]], dim=2)


def voxel_map(L, t, dims):
    """Where output voxel v reads: c + L (v - c) + t, (N, D, H, W, 3) in (z, y, x), fp64."""
    c = torch.tensor([(d - 1) / 2 for d in dims], dtype=F64)
    v = torch.stack(torch.meshgrid(*[torch.arange(d, dtype=F64) for d in dims], indexing="ij"), dim=-1)
    return torch.einsum("nkj,dhwj->ndhwk", L.to(F64), v - c) + c + t.to(F64)[:, None, None, None, :]


def mat_voxel_map(mat, dims):
    """The voxel map of an ops.affine_grid matrix: ix_k = (g_k + 1) n_k / 2 - 1 / 2 of the grid, (N, D, H, W, 3) in (z, y, x)."""
    g = grid_of(mat.detach().cpu().to(F64), dims).flip(-1)
    n = torch.tensor([float(d) for d in dims], dtype=F64)
    return ((g + 1) * n - 1) / 2


def mean_displacement(mat, L, t, dims):
    """Mean over the fixed lattice of |estimated - true| voxel map, per sample."""
    return (mat_voxel_map(mat, dims) - voxel_map(L, t, dims)).norm(dim=-1).mean(dim=(1, 2, 3))


def rotation(omega):
    """exp([omega]x) in fp64 through the matrix exponential (NOT Rodrigues' formula, which the package uses)."""
    a, b, c = (float(v) for v in omega)
    K = torch.tensor([[0.0, -c, b], [c, 0.0, -a], [-b, a, 0.0]], dtype=F64)
    return torch.linalg.matrix_exp(K)


# ---- the accumulation format's floor for d MI / d mat ------------------------------------------------------------------------
def _derivative_matrix(x, lo, hi, bins):
    s = (bins - 3) / (hi - lo) if hi > lo else torch.zeros((), dtype=x.dtype)
    u = ((x - lo) * s + 1).clamp(1, bins - 2)
    k0 = (torch.floor(u).long() - 1).clamp(0, bins - 4)
    t = u - (k0 + 1)
    d = torch.stack([-0.5 * (1 - t) ** 2, 1.5 * t * t - 2 * t, -1.5 * t * t + t + 0.5, 0.5 * t * t], dim=1)
    k = k0[:, None] + torch.arange(4)[None, :]
    return (torch.zeros(x.numel(), bins, dtype=x.dtype).scatter(1, k, d),
            torch.zeros(x.numel(), bins, dtype=x.dtype).scatter(1, k, torch.ones_like(d)), s)


def bound_a(a, b, bins, range_a, range_b):
    """Per voxel, the bound on |d(dMI/da_v)| that the fixed-point table costs by construction: tests/test_mi_gpu.py::_floors'
    bound_a, recomputed here (fp64 tensors, one sample)."""
    a, b = a.reshape(-1), b.reshape(-1)
    V = a.numel()
    lo_a, hi_a, lo_b, hi_b = (torch.tensor(v, dtype=F64) for v in (*range_a, *range_b))
    wa, wb = mi_ref.window_matrix(a, lo_a, hi_a, bins), mi_ref.window_matrix(b, lo_b, hi_b, bins)
    dwa, ca, sa = _derivative_matrix(a, lo_a, hi_a, bins)
    _, cb, _ = _derivative_matrix(b, lo_b, hi_b, bins)
    h, n = wa.t() @ wb, ca.t() @ cb
    G = mi_ref.log_ratio(h / V)
    r = torch.where(h > 0, n * Q / h.clamp_min(1e-300), torch.zeros_like(h))
    rough = G.abs() + torch.log(h.clamp_min(2.0 ** -23) * 2.0 ** 23).abs() + math.log(2)
    e = torch.where(r < 0.5, -torch.log1p(-r.clamp_max(0.5)), rough)
    e = torch.where((h == 0) & (n > 0), torch.zeros_like(e), e)
    ha, hb = h.sum(1), h.sum(0)
    ea = -torch.log1p(-(n.sum(1) * Q / ha.clamp_min(1e-300)).clamp_max(0.5))
    eb = -torch.log1p(-(n.sum(0) * Q / hb.clamp_min(1e-300)).clamp_max(0.5))
    E = e + ea[:, None] + eb[None, :]
    return float(sa) / V * ((dwa.abs() @ E) * wb).sum(1)


def dmat_floor(moving, fixed, mat, bins, ranges, grad64):
    """Per sample: bound_a pushed through |da_v / dmat| of the fp64 restatement -- |da_v / dmat[r][k]| = |da_v / dgrid_v[r]| |p_k|,
    p = (lin_z, lin_y, lin_x, 1) -- over the norm of the fp64 gradient."""
    m64, f64 = moving.detach().cpu().to(F64), fixed.detach().cpu().to(F64)
    grid = grid_of(mat.detach().cpu().to(F64), m64.shape[2:]).requires_grad_(True)
    a = F.grid_sample(m64, grid, mode="bilinear", padding_mode="border", align_corners=False)
    (dgrid,) = torch.autograd.grad(a.sum(), grid)            # every a_v depends on its own grid row only
    p = base_points(m64.shape[2:]).reshape(-1, 4).abs()
    out = []
    for n in range(m64.shape[0]):
        ba = bound_a(a[n].detach(), f64[n], bins, ranges[n][0], ranges[n][1])
        da = dgrid[n].reshape(-1, 3).flip(-1).abs()          # (V, 3) in (z, y, x) rows
        bound = torch.einsum("v,vr,vk->rk", ba, da, p)
        gn = float(grad64[n].norm())
        out.append(float(bound.norm()) / gn if gn > 0 else 0.0)
    return out


def lattice_term_sums(moving, fixed, bins, ranges):
    """For a matrix that puts every coordinate ON a lattice point (voxel_to_mat(I, 0)), per sample an upper bound S (3, 4) on
    sum_v |term_v| of each entry of dmat, term_v[r][k] = dMI/da_v * da_v/dgrid_v[r] * p_k: |dMI/da_v| from the fp64 restatement at
    a = moving (what the identity warp returns), |da_v/dgrid_v[r]| <= (n_r / 2) max(|forward|, |backward| difference of moving
    along axis r) whichever cell a rounding puts the coordinate in (the clamp mask can only remove terms), |p_k| <= 1.  And X
    (3, 4), the same sums with max |moving| in place of the difference: the scale of the corner values that the blend's derivative
    subtracts, hence of its own rounding.  Returns (S, X), each (N, 3, 4)."""
    m64 = moving.detach().cpu().to(F64)
    out, outx = [], []
    for n in range(m64.shape[0]):
        _, da, _ = mi_ref.evaluate(moving[n:n + 1], fixed[n:n + 1], bins, ranges[n][0], ranges[n][1], F64)
        g = da[0, 0].abs()
        x = m64[n, 0]
        slopes = []
        for ax, size in enumerate(x.shape):
            d = x.diff(dim=ax).abs()
            pad = torch.zeros_like(x.narrow(ax, 0, 1))
            slopes.append(torch.maximum(torch.cat([d, pad], dim=ax), torch.cat([pad, d], dim=ax)) * (size / 2))
        p = base_points(x.shape).abs()
        out.append(torch.stack([torch.stack([(g * slopes[r] * p[..., k]).sum() for k in range(4)]) for r in range(3)]))
        top = float(x.abs().max())
        outx.append(torch.stack([torch.stack([(g * p[..., k]).sum() * (x.shape[r] / 2) * top for k in range(4)])
                                 for r in range(3)]))
    return torch.stack(out), torch.stack(outx)


# ---- recovery pairs moved by a known linear map --------------------------------------------------------------------------
RIGID_CASES = {                      # name -> (rotation vector in degrees (z, y, x), shift in voxels (z, y, x), seed)
    "rigid_a": ((4.0, -3.0, 5.0), (1.8, -1.2, 0.9), 5),
    "rigid_b": ((-5.0, 2.5, 3.0), (-1.1, 1.6, 1.4), 9),
}
AFFINE_SCALE = (1.05, 1.0, 0.95)     # the extra anisotropic scale of the affine pair: L = R diag(scale)


def _field_at(size, seed, pts, dense=False):
    """tests/mi_ref.py::_blobs' 12 Gaussians (same generator sequence) evaluated at pts (..., 3) voxels (z, y, x), fp64.
    dense: 48 narrower Gaussians whose centres reach past the volume on every side instead -- a texture without a background,
    so that the entropy of a zoomed view of it does not depend on the zoom (over a large background mutual information rewards
    zooming in on the structure, and the optimum of a scale sits away from the true one)."""
    g = torch.Generator().manual_seed(seed)
    if dense:
        centres = (-0.2 + 1.4 * torch.rand(48, 3, generator=g, dtype=F64)) * (size - 1)
        sigma = (0.07 + 0.06 * torch.rand(48, generator=g, dtype=F64)) * size
        amp = 0.5 + torch.rand(48, generator=g, dtype=F64)
    else:
        centres = (0.2 + 0.6 * torch.rand(12, 3, generator=g, dtype=F64)) * (size - 1)
        sigma = (0.08 + 0.10 * torch.rand(12, generator=g, dtype=F64)) * size
        amp = 0.5 + torch.rand(12, generator=g, dtype=F64)
    out = torch.zeros(pts.shape[:-1], dtype=F64)
    for c, s, a in zip(centres, sigma, amp):
        out += a * torch.exp(-((pts - c) ** 2).sum(-1) / (2 * s * s))
    return out


def moved_pair(size, L, t, seed, dense=False):
    """(fixed, moving), each (1, 1, size, size, size) float32, as mi_ref.recovery_pair but with moving displaced by the voxel-space
    map (L (3, 3), t (3,)): moving[c + L (v - c) + t] = remap(fixed[v]), so voxel_to_mat(L, t) lines moving up with fixed."""
    dims = (size,) * 3
    c = (size - 1) / 2
    v = torch.stack(torch.meshgrid(*[torch.arange(d, dtype=F64) for d in dims], indexing="ij"), dim=-1)
    f0 = _field_at(size, seed, v, dense)
    lo, hi = f0.min(), f0.max()
    # moving(u) = field(c + L^-1 (u - c - t))
    src = torch.einsum("kj,dhwj->dhwk", torch.linalg.inv(L.to(F64)), v - c - t.to(F64)) + c
    fs = ((_field_at(size, seed, src, dense) - lo) / (hi - lo)).clamp(0, 1)

    def remap(x):
        return 0.8 * (1 - x) ** 2 + 0.2 * torch.sin(6 * x) ** 2
    table = remap(torch.linspace(0, 1, 4097, dtype=F64))
    rlo, rhi = table.min(), table.max()
    m = ((remap(fs) - rlo) / (rhi - rlo)).clamp(0, 1)
    return ((f0 - lo) / (hi - lo))[None, None].float(), m[None, None].float()


def rigid_pair(name, size=32):
    """(fixed, moving, L (1, 3, 3), t (1, 3)) of RIGID_CASES[name]."""
    deg, shift, seed = RIGID_CASES[name]
    L = rotation([math.radians(d) for d in deg])
    t = torch.tensor(shift, dtype=F64)
    f, m = moved_pair(size, L, t, seed)
    return f, m, L[None], t[None]


def affine_pair(size=32):
    """rigid_a's motion with AFFINE_SCALE in addition, on the dense texture (see _field_at)."""
    deg, shift, seed = RIGID_CASES["rigid_a"]
    L = rotation([math.radians(d) for d in deg]) @ torch.diag(torch.tensor(AFFINE_SCALE, dtype=F64))
    t = torch.tensor(shift, dtype=F64)
    f, m = moved_pair(size, L, t, seed, dense=True)
    return f, m, L[None], t[None]
