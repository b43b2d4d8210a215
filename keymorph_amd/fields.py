"""Sampling grids as transforms: compose two grids, invert one, hand one over as a displacement field.

Conventions (the ones ``align_img`` samples with, so every function here agrees with it):

* a grid ``G`` is ``(n, D, H, W, 3)``, float32, xyz, normalised; ``align_img(G, x)[v] = x(G[v])`` with
  ``align_corners=False``: coordinate ``g`` along an axis of size ``S`` is voxel ``((g + 1) * S - 1) / 2``;
* as a function of space a grid is its own trilinear interpolant on that lattice with border clamping -- what the sampler
  does to any volume;
* the lattice identity is ``Ids[k, j, i] = ((2i+1)/W - 1, (2j+1)/H - 1, (2k+1)/D - 1)`` (voxel centres).  It is NOT
  ``utils.uniform_norm_grid`` (``linspace(-1, 1)``), the base grid the grid generators evaluate on; nothing here depends on
  that difference, every definition goes through the sampler alone.

Everything runs in csrc/fields.hip on the current stream, batched over ``n``; inputs are float32 on the GPU (anything else
raises ``KeymorphHipError``, there is no CPU fallback) and nothing here is differentiable: an input that requires grad while
grad mode is on raises instead of cutting the graph silently.

Worked example -- interpolate the original moving image ONCE although it is first centred and then registered::

    from keymorph_amd import fields, ops
    from keymorph_amd.utils import align_img

    # 1. io.centering.translate(moving, t) samples the moving image with this grid (t in voxels, (z, y, x)):
    n, _, D, H, W = moving.shape
    mat = torch.zeros(n, 3, 4, device=moving.device)
    for k, s in enumerate((D, H, W)):
        mat[:, k, k] = (s - 1) / s
        mat[:, k, 3] = t[:, k] * (2.0 / s)
    g_center = ops.affine_grid(mat, (D, H, W))           # centred = align_img(g_center, moving)
    # 2. KeyMorph registers the CENTRED image: aligned = align_img(g_reg, centred), two interpolations of `moving`
    g_reg = model(fixed, align_img(g_center, moving), transform_type="tps_0")["tps_0"]["grid"].detach()
    # 3. one grid from fixed space into the original moving image: look g_center up where g_reg points
    g_total = fields.compose(g_reg, g_center)
    aligned = align_img(g_total, moving)                 # one interpolation
    # a fixed-space label map carried into moving space through the same transform, and its folding statistics
    h = fields.invert(g_total)                           # compose(h, g_total) = identity
    labels_in_moving = align_img(h, fixed_labels, mode="nearest")
    loss_ops.jdstd(fields.to_displacement(g_total[:1]))

(The upstream helpers ``utils.pytorchflow2displacement`` / ``displacement2pytorchflow`` stay placeholders: they work on the
``align_corners=True`` lattice, which is not the one ``align_img`` samples on.  Use ``to_displacement`` / ``from_displacement``.)
"""
from __future__ import annotations

import functools

import torch

from . import _lib, ops
from ._lib import check
from .ops import _p, _stream

Tensor = torch.Tensor

_START_POINTS = 16      # invert(): the affine start is fitted on at most this many lattice points per axis


def _check(t: Tensor, name: str, shape_doc: str, ok) -> Tensor:
    """float32, on the GPU, not part of an autograd graph, the documented shape -> contiguous (ops._prep)."""
    if not isinstance(t, torch.Tensor):
        raise _lib.KeymorphHipError(f"{name}: expected a torch tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise _lib.KeymorphHipError(f"{name} is {t.dtype}: keymorph_amd.fields takes float32 tensors on the GPU")
    if t.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{name} requires grad, and keymorph_amd.fields is not differentiable: pass {name}.detach() "
                           "or call it under torch.no_grad()")
    if not ok(t):
        raise ValueError(f"{name}: expected {shape_doc}, got {tuple(t.shape)}")
    return ops._prep(t.detach(), name)


def _grid(t: Tensor, name: str) -> Tensor:
    return _check(t, name, "a grid (n, D, H, W, 3)", lambda g: g.dim() == 5 and g.shape[-1] == 3 and g.numel() > 0)


def identity_grid(shape, device) -> Tensor:
    """``Ids`` for ``shape`` = (n, ., D, H, W) or (D, H, W) (then n = 1): (n, D, H, W, 3), the grid with
    ``align_img(Ids, x) == x``."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 3:
        n, dims = 1, shape
    elif len(shape) == 5:
        n, dims = shape[0], shape[2:]
    else:
        raise ValueError(f"identity_grid: shape must be (n, C, D, H, W) or (D, H, W), got {shape}")
    if n < 1 or min(dims) < 1:
        raise ValueError(f"identity_grid: empty shape {shape}")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.KeymorphHipError(f"identity_grid on {device}: keymorph_amd ops run only on an AMD GPU (no CPU fallback)")
    out = torch.empty((n, *dims, 3), dtype=torch.float32, device=device)
    ops._prep(out, "identity_grid")      # (the current-device rule of every op)
    check(_lib.load().kmh_field_identity(_p(out), n, *dims, _stream()), "kmh_field_identity")
    return out


def compose(first: Tensor, then: Tensor) -> Tensor:
    """``G12[w] = then(first[w])``: the grid on the lattice of ``first`` with
    ``align_img(compose(G1, G2), x) ~ align_img(G1, align_img(G2, x))`` (equal up to the blend of ``x`` being applied once
    instead of twice; border behaviour identical).  The two grids may have different spatial sizes.  One kernel, ``then`` is
    read channels-last; bit-identical to ``align_img(first, then.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)``."""
    first, then = _grid(first, "first"), _grid(then, "then")
    if first.shape[0] != then.shape[0]:
        raise ValueError(f"compose: batch sizes differ, {tuple(first.shape)} and {tuple(then.shape)}")
    n, Do, Ho, Wo, _ = first.shape
    _, D, H, W, _ = then.shape
    out = torch.empty_like(first)
    if _lib.profiler.enabled:      # first 12 B + out 12 B per output voxel, `then` once
        _lib.profiler.meta = {"bytes": 24.0 * n * Do * Ho * Wo + 12.0 * n * D * H * W}
    check(_lib.load().kmh_field_compose(_p(first), _p(then), _p(out), n, Do, Ho, Wo, D, H, W, _stream()), "kmh_field_compose")
    return out


@functools.lru_cache(maxsize=16)
def _start_lattice(dims, strides, device):
    """Ids on every strides-th lattice point, (1, d, h, w, 3): a few thousand points, built once per shape and device."""
    ax = [(2.0 * torch.arange(0, s, k, dtype=torch.float32, device=device) + 1.0) / s - 1.0 for s, k in zip(dims, strides)]
    z, y, x = torch.meshgrid(*ax, indexing="ij")
    return torch.stack([x, y, z], dim=-1).unsqueeze(0)


def _affine_start(grid: Tensor) -> Tensor:
    """(n, 3, 4): the affine map that takes grid VALUES back to the lattice points they sit on, fitted in closed form
    (ops.affine_fit) on a strided subsample of the lattice; non-finite grid rows get weight 0.  No host synchronisation."""
    n, D, H, W, _ = grid.shape
    st = tuple(max(1, -(-s // _START_POINTS)) for s in (D, H, W))
    sub = grid[:, ::st[0], ::st[1], ::st[2]]
    ids = _start_lattice((D, H, W), st, grid.device).expand_as(sub)
    x, y = sub.reshape(n, -1, 3), ids.reshape(n, -1, 3)
    w = torch.isfinite(x).all(dim=-1)
    x = torch.where(w.unsqueeze(-1), x, torch.zeros_like(x))
    return ops.affine_fit(x, y, w.to(torch.float32))


def _invert(grid: Tensor, tol: float, max_iters: int):
    grid = _grid(grid, "grid")
    n, D, H, W, _ = grid.shape
    if min(D, H, W) < 2:
        raise ValueError(f"invert: every axis of the grid must be at least 2, got {(D, H, W)}")
    if not (tol >= 0.0) or int(max_iters) < 0:
        raise ValueError(f"invert: tol must be >= 0 and max_iters >= 0, got {tol} and {max_iters}")
    lib = _lib.load()
    start = _affine_start(grid)
    dev = grid.device
    out = torch.empty_like(grid)
    conv = torch.empty((n, D, H, W), dtype=torch.uint8, device=dev)
    unconv = torch.empty(n, dtype=torch.int64, device=dev)
    iters = torch.empty(n, dtype=torch.int64, device=dev)
    maxres = torch.empty(n, dtype=torch.float32, device=dev)
    ws = ops.workspace(int(lib.kmh_field_invert_ws_bytes(n, D, H, W)), dev, "fields")
    check(lib.kmh_field_invert(_p(grid), _p(start), _p(out), _p(conv), _p(unconv), _p(maxres), _p(iters), n, D, H, W,
                               float(tol), int(max_iters), _p(ws), _stream()), "kmh_field_invert")
    return out, conv, unconv, maxres, iters


def invert(grid: Tensor, tol: float = 1e-5, max_iters: int = 20, return_info: bool = False):
    """``H`` on the lattice of ``grid`` with ``compose(H, grid) = Ids``: for every voxel ``w`` the point ``c`` with
    ``grid(c) = Ids[w]``, by per-voxel Newton steps (each limited to one voxel per axis, ``c`` kept inside [-1, 1]) from a
    closed-form affine start, until ``max |residual| <= tol`` or ``max_iters`` steps.  Where the Jacobian is near-singular (a
    fold, or the flat band between the border and the first voxel centre) the step goes through the start's linear part.

    ``return_info=True`` -> ``(H, converged, unconverged, max_residual)``: ``converged`` (n, D, H, W) uint8, ``unconverged``
    (n,) int64, ``max_residual`` (n,) float32 over the converged voxels -- device tensors, nothing is read back.  A target
    outside the image of ``grid`` has no solution: its voxel ends finite, inside [-1, 1] and flagged (``converged == 0``), and
    so does a voxel whose iteration met a non-finite grid value."""
    out, conv, unconv, maxres, _ = _invert(grid, tol, max_iters)
    return (out, conv, unconv, maxres) if return_info else out


def to_displacement(grid: Tensor) -> Tensor:
    """(n, 3, D, H, W), channels (z, y, x), in voxels: the voxel the grid points at minus the voxel's own index,
    ``(g - Ids) * S / 2`` -- what ``loss_ops.jdstd`` / ``jdlessthan0`` / ``_jacobian_determinant`` expect."""
    grid = _grid(grid, "grid")
    n, D, H, W, _ = grid.shape
    out = torch.empty((n, 3, D, H, W), dtype=torch.float32, device=grid.device)
    check(_lib.load().kmh_field_to_displacement(_p(grid), _p(out), n, D, H, W, _stream()), "kmh_field_to_displacement")
    return out


def from_displacement(disp: Tensor) -> Tensor:
    """The inverse of ``to_displacement``: (n, 3, D, H, W) voxels, channels (z, y, x) -> the grid (n, D, H, W, 3)."""
    disp = _check(disp, "disp", "a displacement field (n, 3, D, H, W)",
                  lambda d: d.dim() == 5 and d.shape[1] == 3 and d.numel() > 0)
    n, _, D, H, W = disp.shape
    out = torch.empty((n, D, H, W, 3), dtype=torch.float32, device=disp.device)
    check(_lib.load().kmh_field_from_displacement(_p(disp), _p(out), n, D, H, W, _stream()), "kmh_field_from_displacement")
    return out


class _SmoothGrid(torch.autograd.Function):
    """smooth(): the chain of three kernels forward; backward, the smoothing's transpose on each component of the cotangent -- the
    two displacement maps scale a component by S / 2 and by 2 / S, which cancel around an operator that works per channel."""

    @staticmethod
    def forward(ctx, grid, sigma, plan):
        ctx.plan = plan
        return from_displacement(ops.gaussian_smooth(to_displacement(grid.detach()), sigma))

    @staticmethod
    def backward(ctx, gout):
        if ctx.plan is None:
            return gout, None, None
        g = ops._prep(gout, "gout").permute(0, 4, 1, 2, 3).contiguous()
        return ops._gauss_call(g, ctx.plan, True).permute(0, 2, 3, 4, 1).contiguous(), None, None


def smooth(grid: Tensor, sigma) -> Tensor:
    """The grid (n, D, H, W, 3) whose voxel displacement is ``grid``'s, smoothed by a Gaussian of ``sigma`` voxels (a number or a
    (z, y, x) triple): ``from_displacement(ops.gaussian_smooth(to_displacement(grid), sigma))`` -- the regulariser of demons and
    SyN.  The DISPLACEMENT is smoothed, not the grid: the smoothing replicates its border, which would flatten the identity's
    ramp near the faces, while a zero displacement stays zero (``smooth(identity_grid(...), sigma)`` is the identity, bit for bit).
    Unlike the rest of this module it is differentiable in ``grid``."""
    if not isinstance(grid, torch.Tensor):
        raise _lib.KeymorphHipError(f"grid: expected a torch tensor, got {type(grid).__name__}")
    ops._need_gpu_f32("smooth", "grid", grid)
    if grid.dim() != 5 or grid.shape[-1] != 3 or grid.numel() == 0:
        raise ValueError(f"grid: expected a grid (n, D, H, W, 3), got {tuple(grid.shape)}")
    n, D, H, W, _ = grid.shape
    # the displacement's shape as a view of one element: sigma and the limits are checked before anything is allocated
    plan = ops._gauss_plan("smooth", grid.detach().reshape(-1)[:1].expand(n, 3, D, H, W), sigma, 4.0)
    return _SmoothGrid.apply(grid, sigma, plan)
