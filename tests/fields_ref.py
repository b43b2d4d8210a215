"""fp64 restatement of keymorph_amd.fields on the CPU (plain torch): the yardstick of tests/test_fields_*.py.

A grid (n, D, H, W, 3) is xyz, normalised, align_corners=False; as a function of space it is its own trilinear interpolant
with border clamping (`interp`).  Nothing here imports the package under test."""
import math

import torch

F64 = torch.float64


def identity_grid(dims, n=1):
    """Ids (n, D, H, W, 3): ((2i+1)/W - 1, (2j+1)/H - 1, (2k+1)/D - 1)."""
    D, H, W = (int(s) for s in dims)
    ax = [(2 * torch.arange(s, dtype=F64) + 1) / s - 1 for s in (D, H, W)]
    z, y, x = torch.meshgrid(*ax, indexing="ij")
    return torch.stack([x, y, z], dim=-1).unsqueeze(0).expand(n, D, H, W, 3).clone()


def _taps(pts, dims):
    """Sampler coordinates of pts (..., 3) xyz on a (D, H, W) lattice: floor corners, +1 corners (clamped), fractions and
    d(voxel coordinate)/d(normalised coordinate) including the clamp mask.  NaN goes to the far border, as the sampler does."""
    out = []
    for a, S in enumerate((dims[2], dims[1], dims[0])):       # x, y, z
        v = ((pts[..., a] + 1) * S - 1) / 2
        lo, hi = v <= 0, ~(v < S - 1)
        m = torch.where(lo | hi, torch.zeros_like(v), torch.full_like(v, S / 2))
        v = torch.where(lo, torch.zeros_like(v), torch.where(hi, torch.full_like(v, S - 1), v))
        i0 = v.floor()
        f = v - i0
        i0 = i0.long()
        out.append((i0, (i0 + 1).clamp(max=S - 1), f, m))
    return out


def interp(G, pts, jac=False):
    """G (n, D, H, W, 3) evaluated at pts (n, ..., 3): (n, ..., 3) in fp64, and with jac=True also d G / d pts (n, ..., 3, 3)."""
    G, pts = G.to(F64), pts.to(F64)
    n, D, H, W, _ = G.shape
    (x0, x1, fx, mx), (y0, y1, fy, my), (z0, z1, fz, mz) = _taps(pts, (D, H, W))
    b = torch.arange(n).view(n, *([1] * (pts.dim() - 2))).expand(pts.shape[:-1])
    val = torch.zeros(*pts.shape[:-1], 3, dtype=F64)
    J = torch.zeros(*pts.shape[:-1], 3, 3, dtype=F64)
    for zi, wz, dz in ((z0, 1 - fz, -1.0), (z1, fz, 1.0)):
        for yi, wy, dy in ((y0, 1 - fy, -1.0), (y1, fy, 1.0)):
            for xi, wx, dx in ((x0, 1 - fx, -1.0), (x1, fx, 1.0)):
                g = G[b, zi, yi, xi]
                val = val + g * (wx * wy * wz).unsqueeze(-1)
                if jac:
                    J[..., 0] += g * (dx * wy * wz * mx).unsqueeze(-1)
                    J[..., 1] += g * (wx * dy * wz * my).unsqueeze(-1)
                    J[..., 2] += g * (wx * wy * dz * mz).unsqueeze(-1)
    return (val, J) if jac else val


def compose(first, then):
    """then interpolated at first: a grid on the lattice of first."""
    return interp(then, first)


def affine_start(G, ids):
    """(n, 3, 4) least-squares affine map from grid values to the lattice points they sit on."""
    n = G.shape[0]
    X = torch.cat([G.reshape(n, -1, 3), torch.ones(n, G[0, ..., 0].numel(), 1, dtype=F64)], dim=-1)
    return torch.linalg.lstsq(X, ids.reshape(n, -1, 3)).solution.transpose(1, 2)


def invert(G, tol=1e-5, max_iters=20, dtype=F64):
    """The Newton scheme of fields.invert restated: -> H, converged (bool), iterations (long), residual (max-norm at the end).
    dtype=float32 runs the same arithmetic in single precision (the fp32 residual floor)."""
    G = G.to(F64)
    n, D, H, W, _ = G.shape
    ids = identity_grid((D, H, W), n)
    A = affine_start(G, ids)
    G, ids, A = G.to(dtype), ids.to(dtype), A.to(dtype)
    L = A[:, :, :3]
    detL = torch.linalg.det(L.to(F64)).to(dtype).view(n, 1, 1, 1)
    c = (torch.einsum("nab,ndhwb->ndhwa", L, ids) + A[:, :, 3].view(n, 1, 1, 1, 3)).clamp(-1, 1)
    lim = torch.tensor([2.0 / W, 2.0 / H, 2.0 / D], dtype=dtype)
    active = torch.ones(n, D, H, W, dtype=torch.bool)
    ok = torch.zeros_like(active)
    its = torch.zeros(n, D, H, W, dtype=torch.long)
    res = torch.zeros(n, D, H, W, dtype=dtype)
    for it in range(max_iters + 1):
        val, J = interp(G, c, jac=True)
        val, J = val.to(dtype), J.to(dtype)
        r = ids - val
        rmax = r.abs().amax(dim=-1)
        res = torch.where(active, rmax, res)
        bad = ~torch.isfinite(r).all(dim=-1)
        done = active & ~bad & (rmax <= tol)
        ok |= done
        active = active & ~bad & ~done
        if it == max_iters or not bool(active.any()):
            break
        det = torch.linalg.det(J.to(F64)).to(dtype)
        newton = det * detL > 0.05
        Jsafe = torch.where(newton[..., None, None], J, torch.eye(3, dtype=dtype).expand_as(J))
        d = torch.where(newton.unsqueeze(-1), torch.linalg.solve(Jsafe.to(F64), r.to(F64).unsqueeze(-1)).squeeze(-1).to(dtype),
                        torch.einsum("nab,ndhwb->ndhwa", L, r))
        d = torch.maximum(torch.minimum(d, lim), -lim)
        c = torch.where(active.unsqueeze(-1), (c + d).clamp(-1, 1), c)
        its += active.long()
    return c, ok, its, res


def to_displacement(G):
    """(n, 3, D, H, W), channels (z, y, x), voxels: (g - Ids) * S / 2."""
    G = G.to(F64)
    n, D, H, W, _ = G.shape
    d = (G - identity_grid((D, H, W), n)) * torch.tensor([W / 2, H / 2, D / 2], dtype=F64)
    return d.flip(-1).permute(0, 4, 1, 2, 3).contiguous()


def from_displacement(disp):
    disp = disp.to(F64)
    n, _, D, H, W = disp.shape
    g = disp.permute(0, 2, 3, 4, 1).flip(-1) / torch.tensor([W / 2, H / 2, D / 2], dtype=F64)
    return g + identity_grid((D, H, W), n)


def jacobian_det_central(disp):
    """det(d(disp)/d(z, y, x) + I) by central differences on the interior voxels: (n, D-2, H-2, W-2)."""
    disp = disp.to(F64)
    grads = []
    for ax in (2, 3, 4):                      # d/dz, d/dy, d/dx
        hi = disp.narrow(ax, 2, disp.shape[ax] - 2)
        lo = disp.narrow(ax, 0, disp.shape[ax] - 2)
        g = (hi - lo) / 2
        for other in (2, 3, 4):
            if other != ax:
                g = g.narrow(other, 1, g.shape[other] - 2)
        grads.append(g)
    J = torch.stack(grads, dim=-1).permute(0, 2, 3, 4, 1, 5) + torch.eye(3, dtype=F64)      # (n, d, h, w, component, axis)
    return torch.linalg.det(J)


# ---- the test field ------------------------------------------------------------------------------------------------
CASES = {
    "A": dict(a=0.0, rot=10.0, sc=1.3, b=(0.03, -0.02, 0.02)),
    "B": dict(a=0.04, rot=10.0, sc=1.3, b=(0.03, -0.02, 0.02)),
    "C": dict(a=0.06, rot=15.0, sc=1.45, b=(0.0, 0.02, 0.0)),
    "D": dict(a=0.04, rot=25.0, sc=0.9, b=(0.03, -0.02, 0.02)),      # part of the targets is unreachable
}


def matrix(rot_deg, sc):
    """M = sc * Rz(rot) * Rx(0.6 rot), acting on (x, y, z)."""
    r, q = math.radians(rot_deg), math.radians(0.6 * rot_deg)
    Rz = torch.tensor([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]], dtype=F64)
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(q), -math.sin(q)], [0, math.sin(q), math.cos(q)]], dtype=F64)
    return sc * Rz @ Rx


def sample_params(case, s):
    """Sample 0 is the case as the table states it; sample 1 turns the other way by 0.8 of the angle with the offset negated,
    so that the two samples of a batch carry different transforms."""
    p = CASES[case]
    if s == 0:
        return p["a"], p["rot"], p["sc"], torch.tensor(p["b"], dtype=F64)
    return p["a"], -0.8 * p["rot"], p["sc"], -torch.tensor(p["b"], dtype=F64)


def field(dims, a, M, b):
    """(D, H, W, 3) fp64: Ids M^T + b + a (sin(3y+1)cos(2z), sin(2.5z)cos(3x+.5), sin(3x)cos(2y+.3)) on its own lattice."""
    ids = identity_grid(dims)[0]
    x, y, z = ids.unbind(-1)
    wob = torch.stack([torch.sin(3 * y + 1) * torch.cos(2 * z), torch.sin(2.5 * z) * torch.cos(3 * x + 0.5),
                       torch.sin(3 * x) * torch.cos(2 * y + 0.3)], dim=-1)
    return ids @ M.T + b + a * wob


def case_grid(case, dims, n=2):
    """(n, D, H, W, 3) fp64 and the per-sample (M, b)."""
    gs, mb = [], []
    for s in range(n):
        a, rot, sc, b = sample_params(case, s)
        M = matrix(rot, sc)
        gs.append(field(dims, a, M, b))
        mb.append((M, b))
    return torch.stack(gs), mb
