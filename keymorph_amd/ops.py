"""torch.autograd.Function wrappers over the C ABI (include/keymorph_hip.h).

PyTorch is plumbing here: it owns device memory, the current HIP stream and autograd
bookkeeping.  Every FLOP of the hot path runs in libkeymorph_hip.so; there is no
eager/PyTorch fallback -- a CPU tensor or a missing library raises.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os

from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check

Tensor = torch.Tensor


# --------------------------------------------------------------------------
# plumbing
# --------------------------------------------------------------------------
def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _need_gpu(who: Optional[str], name: str, t) -> None:
    """t is a tensor on the current GPU, or KeymorphHipError.  who: the public function named in the message (None: none)."""
    if not isinstance(t, Tensor) or not t.is_cuda:
        what = f"{who}: {name}" if who else name
        raise _lib.KeymorphHipError(f"{what} is not on the GPU: keymorph_amd ops run only on an AMD GPU (no CPU fallback)")
    if t.device.index != torch.cuda.current_device():
        # the C ABI launches on the CURRENT device's stream and never calls hipSetDevice: a tensor that lives on
        # another GPU would be touched by kernels queued on the wrong device
        raise _lib.KeymorphHipError(
            f"{who + ': ' if who else ''}{name} is on {t.device} but the current device is cuda:{torch.cuda.current_device()}: "
            "call torch.cuda.set_device(...) (one process per GPU) before using keymorph_amd ops")


def _need_gpu_f32(who: str, name: str, t) -> None:
    """_need_gpu, then float32 or ValueError: for the ops that state their dtype instead of converting (_prep converts)."""
    _need_gpu(who, name, t)
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: {name} must be float32, got {t.dtype}")


def _need_volume_pair(who: str, a: Tensor, b: Tensor, max_voxels: Optional[int] = None, min_w: int = 1) -> None:
    """a, b: two non-empty (N, 1, D, H, W) tensors of one shape, W >= min_w, fewer than max_voxels voxels per sample, or
    ValueError."""
    if a.shape != b.shape:
        raise ValueError(f"{who}: shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    if a.dim() != 5 or a.shape[1] != 1 or a.numel() == 0:
        raise ValueError(f"{who}: expected two non-empty (N, 1, D, H, W) volumes, got {tuple(a.shape)}")
    if a.shape[4] < min_w or (max_voxels is not None and a.numel() // a.shape[0] >= max_voxels):
        raise ValueError(f"{who}: needs W >= {min_w} and fewer than {max_voxels} voxels per sample, got {tuple(a.shape)}")


def _prep(t: Tensor, name: str = "tensor") -> Tensor:
    _need_gpu(None, name, t)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


_WS = {}


def workspace(nbytes: int, device: torch.device, slot: str = "reduce") -> Tensor:
    """Stream-ordered scratch (grown on demand, reused by consecutive launches)."""
    key = (device.index, slot)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _reduce_ws(device) -> Tensor:
    return workspace(int(_lib.load().kmh_reduce_ws_bytes()), device, "reduce")


# --------------------------------------------------------------------------
# a11  sampler
# --------------------------------------------------------------------------
class _GridSample3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, grid, mode):
        lib = _lib.load()
        x, grid = _prep(x, "x"), _prep(grid, "grid")
        N, C, D, H, W = x.shape
        n2, Do, Ho, Wo, three = grid.shape
        assert n2 == N and three == 3, "grid must be (N, Do, Ho, Wo, 3)"
        out = torch.empty((N, C, Do, Ho, Wo), dtype=torch.float32, device=x.device)
        if _lib.profiler.enabled:  # grid 12 B + C*(volume 4 B + out 4 B) per output voxel
            _lib.profiler.meta = {"bytes": float(N * Do * Ho * Wo) * (12 + 8 * C)}
        check(lib.kmh_grid_sample3d_fwd(_p(x), _p(grid), _p(out), N, C, D, H, W, Do, Ho, Wo, mode, _stream()),
              "kmh_grid_sample3d_fwd")
        ctx.save_for_backward(x, grid)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        x, grid = ctx.saved_tensors
        gout = _prep(gout)
        N, C, D, H, W = x.shape
        _, Do, Ho, Wo, _ = grid.shape
        dx = dgrid = None
        if ctx.needs_input_grad[1]:
            if ctx.mode != 0:
                dgrid = torch.zeros_like(grid)
            else:
                dgrid = torch.empty_like(grid)
                if _lib.profiler.enabled:  # gout 4C + grid 12 + volume 4C + dgrid 12 B per voxel
                    _lib.profiler.meta = {"bytes": float(N * Do * Ho * Wo) * (24 + 8 * C)}
                check(lib.kmh_grid_sample3d_bwd_grid(_p(x), _p(grid), _p(gout), _p(dgrid), N, C, D, H, W, Do, Ho,
                                                     Wo, _stream()), "kmh_grid_sample3d_bwd_grid")
        if ctx.needs_input_grad[0]:
            if ctx.mode != 0:
                raise NotImplementedError("gradient wrt the volume is implemented for bilinear mode only")
            dx = torch.zeros_like(x)
            check(lib.kmh_grid_sample3d_bwd_input(_p(grid), _p(gout), _p(dx), N, C, D, H, W, Do, Ho, Wo,
                                                  _stream()), "kmh_grid_sample3d_bwd_input")
        return dx, dgrid, None


def grid_sample3d(x: Tensor, grid: Tensor, mode: str = "bilinear") -> Tensor:
    """mode "cubic": cubic_sample(cubic_coefficients(x), grid), differentiable in the grid only.  mode "label": warp_labels(x,
    grid), x an integer label map; no gradient."""
    if mode == "cubic":
        return _GridSampleCubic.apply(x, grid)
    if mode == "label":
        return warp_labels(x, grid)
    return _GridSample3d.apply(x, grid, {"bilinear": 0, "nearest": 1}[mode])


# label maps through a grid by trilinear vote (csrc/label_warp.hip): its element types as (bytes, signed), and its limits
LABEL_DTYPES = {torch.uint8: (1, 0), torch.bool: (1, 0), torch.int16: (2, 1), torch.int32: (4, 1), torch.int64: (8, 1)}
LABEL_MAX_PLANE = 1 << 29      # voxels of one channel plane (an int64 plane inside a 32-bit byte range)
LABEL_MAX_PLANES = 65535       # N * C (gridDim.y)


def warp_labels(labels: Tensor, grid: Tensor, return_weight: bool = False):
    """Integer label maps labels (N, C, D, H, W) -- uint8, bool, int16, int32 or int64 on the current GPU, every channel a map of
    its own -- resampled at grid (N, Do, Ho, Wo, 3) -> (N, C, Do, Ho, Wo) of the same dtype: per output voxel the label whose
    one-hot channel align_img's bilinear sampler would give the largest value, the smallest such label on a tie.  For labels in
    [0, L) that is torch.argmax(align_img(grid, one_hot(labels).float()), 1) bit for bit (the same corners, the same float32
    weights, the same order of additions), in one pass over 8 corner labels per voxel and without the L channels; label ids
    enter only through == and <, so any ids do (signed order for the signed dtypes, False < True).  return_weight: also the
    winner's summed weight (float32, the .max(1) of that chain).  Neither output carries a gradient; labels and grid may be part
    of a graph, which is left alone."""
    who = "warp_labels"
    _need_gpu(who, "labels", labels)
    _need_gpu(who, "grid", grid)
    if labels.dtype not in LABEL_DTYPES:
        if labels.dtype.is_floating_point:
            raise TypeError(f"{who}: labels is {labels.dtype}; pass the integer label map itself (uint8, bool, int16, int32 or "
                            "int64), not a float copy or a one-hot encoding of it")
        raise TypeError(f"{who}: labels must be uint8, bool, int16, int32 or int64, got {labels.dtype}")
    if labels.dim() != 5 or labels.numel() == 0:
        raise ValueError(f"{who}: expected non-empty (N, C, D, H, W) label maps, got {tuple(labels.shape)}")
    N, C, D, H, W = labels.shape
    if D * H * W >= LABEL_MAX_PLANE or N * C > LABEL_MAX_PLANES:
        raise ValueError(f"{who}: a channel plane must have fewer than 2^29 voxels and N * C be at most {LABEL_MAX_PLANES}, got "
                         f"{tuple(labels.shape)}")
    if grid.dim() != 5 or grid.shape[0] != N or grid.shape[4] != 3 or grid.numel() == 0:
        raise ValueError(f"{who}: expected a non-empty grid ({N}, Do, Ho, Wo, 3), got {tuple(grid.shape)}")
    nbytes, signed = LABEL_DTYPES[labels.dtype]
    lab = labels.detach().contiguous()
    if lab.dtype == torch.bool:
        lab = lab.view(torch.uint8)
    grid = _prep(grid.detach(), "grid")
    _, Do, Ho, Wo, _ = grid.shape
    out = torch.empty((N, C, Do, Ho, Wo), dtype=lab.dtype, device=lab.device)
    weight = torch.empty((N, C, Do, Ho, Wo), dtype=torch.float32, device=lab.device) if return_weight else None
    if _lib.profiler.enabled:  # grid 12 B, 8 corner labels of which a smooth grid shares all but ~1, one label (+ 4 B) out
        _lib.profiler.meta = {"bytes": float(N * C * Do * Ho * Wo) * (12 + 2 * nbytes + (4 if return_weight else 0))}
    check(_lib.load().kmh_warp_labels(_p(lab), nbytes, signed, _p(grid), _p(out), _p(weight), N, C, D, H, W, Do, Ho, Wo,
                                      _stream()), "kmh_warp_labels")
    if labels.dtype == torch.bool:
        out = out.view(torch.bool)
    return (out, weight) if return_weight else out


# cubic B-spline resampling (csrc/cubic.hip): the limits of its kernels
CUBIC_MAX_PLANE = 1 << 29      # voxels of one channel plane (32-bit byte offsets inside it)
CUBIC_MAX_BATCH = 65535


def _cubic_check(who: str, x, grid=None) -> None:
    """x: a non-empty (N, C, D, H, W) volume on the GPU within the kernels' limits; grid: (N, Do, Ho, Wo, 3), non-empty.
    KeymorphHipError for a tensor that is not on the GPU, ValueError for the rest -- before anything is allocated or copied."""
    _need_gpu(who, "the volume", x)
    if grid is not None:
        _need_gpu(who, "grid", grid)
    if x.dim() != 5 or x.numel() == 0:
        raise ValueError(f"{who}: expected a non-empty (N, C, D, H, W) volume, got {tuple(x.shape)}")
    N, _, D, H, W = x.shape
    if D * H * W >= CUBIC_MAX_PLANE or N > CUBIC_MAX_BATCH:
        raise ValueError(f"{who}: a channel plane must have fewer than 2^29 voxels and the batch at most {CUBIC_MAX_BATCH} "
                         f"samples, got {tuple(x.shape)}")
    if grid is not None and (grid.dim() != 5 or grid.shape[0] != N or grid.shape[4] != 3 or grid.numel() == 0):
        raise ValueError(f"{who}: expected a non-empty grid ({N}, Do, Ho, Wo, 3), got {tuple(grid.shape)}")


def _cubic_prefilter(x: Tensor) -> Tensor:
    x = _prep(x.detach(), "x")
    coef = torch.empty_like(x)
    N, C, D, H, W = x.shape
    if _lib.profiler.enabled:  # the floor: every pass reads and writes each voxel once
        _lib.profiler.meta = {"bytes": 8.0 * x.numel() * sum(1 for n in (D, H, W) if n > 1)}
    check(_lib.load().kmh_cubic_prefilter(_p(x), _p(coef), N, C, D, H, W, _stream()), "kmh_cubic_prefilter")
    return coef


def _cubic_fwd(coef: Tensor, grid: Tensor) -> Tensor:
    N, C, D, H, W = coef.shape
    _, Do, Ho, Wo, _ = grid.shape
    out = torch.empty((N, C, Do, Ho, Wo), dtype=torch.float32, device=coef.device)
    if _lib.profiler.enabled:  # grid 12 B + C * out 4 B per output voxel, the coefficients once
        _lib.profiler.meta = {"bytes": float(N * Do * Ho * Wo) * (12 + 4 * C) + 4.0 * coef.numel()}
    check(_lib.load().kmh_cubic_sample_fwd(_p(coef), _p(grid), _p(out), N, C, D, H, W, Do, Ho, Wo, _stream()),
          "kmh_cubic_sample_fwd")
    return out


def _cubic_bwd(ctx, gout):
    """the shared backward of the two cubic Functions: saved (coef, grid); input 0 is the volume / the coefficients"""
    if ctx.needs_input_grad[0]:
        raise NotImplementedError("cubic resampling has no gradient with respect to the volume (only to the grid)")
    if not ctx.needs_input_grad[1]:
        return None, None
    coef, grid = ctx.saved_tensors
    gout = _prep(gout)
    N, C, D, H, W = coef.shape
    _, Do, Ho, Wo, _ = grid.shape
    dgrid = torch.empty_like(grid)
    if _lib.profiler.enabled:  # gout 4C + grid 12 + dgrid 12 B per output voxel, the coefficients once
        _lib.profiler.meta = {"bytes": float(N * Do * Ho * Wo) * (24 + 4 * C) + 4.0 * coef.numel()}
    check(_lib.load().kmh_cubic_sample_bwd_grid(_p(coef), _p(grid), _p(gout), _p(dgrid), N, C, D, H, W, Do, Ho, Wo,
                                                _stream()), "kmh_cubic_sample_bwd_grid")
    return None, dgrid


class _CubicSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coef, grid):
        coef, grid = _prep(coef, "coef"), _prep(grid, "grid")
        ctx.save_for_backward(coef, grid)
        return _cubic_fwd(coef, grid)

    backward = staticmethod(_cubic_bwd)


class _GridSampleCubic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, grid):
        _cubic_check("grid_sample3d", x, grid)
        coef, grid = _cubic_prefilter(x), _prep(grid, "grid")
        ctx.save_for_backward(coef, grid)
        return _cubic_fwd(coef, grid)

    backward = staticmethod(_cubic_bwd)


def cubic_coefficients(x: Tensor) -> Tensor:
    """The cubic B-spline coefficients of x (N, C, D, H, W) -> (N, C, D, H, W) float32: the separable recursive prefilter along
    W, H and D with whole-sample mirror ends (scipy.ndimage.spline_filter(order=3, mode="mirror") per channel); an axis of
    length 1 is left alone.  No graph through it: the volumes are data.  For callers that sample one volume many times:
    cubic_sample(cubic_coefficients(x), grid) is grid_sample3d(x, grid, "cubic")."""
    _cubic_check("cubic_coefficients", x)
    return _cubic_prefilter(x)


def cubic_sample(coef: Tensor, grid: Tensor) -> Tensor:
    """The cubic B-spline with coefficients coef (N, C, D, H, W) at grid (N, Do, Ho, Wo, 3) -> (N, C, Do, Ho, Wo), in align_img's
    convention (border, align_corners=False: the trilinear sampler's source coordinate, clamped to the voxel centres, with a zero
    grid gradient where clamped).  64 taps, mirrored at the ends like the coefficients.  The spline interpolates the data at the
    voxel centres and overshoots between them: data in [0, 1] can leave [0, 1], and nothing is clamped -- label maps stay on
    "nearest".  Differentiable in grid only; a coef that requires a gradient raises NotImplementedError in backward."""
    _cubic_check("cubic_sample", coef, grid)
    return _CubicSample.apply(coef, grid)


# Gaussian smoothing (csrc/gauss.hip): the limits of its kernels
GAUSS_MAX_RADIUS = 32          # taps on either side of the centre (sigma <= 8 at truncate = 4)
GAUSS_MAX_PLANE = 1 << 29      # voxels of one channel plane
GAUSS_MAX_PLANES = 65535       # N * C (gridDim.y)


def _gauss_sigmas(who: str, sigma, truncate) -> Tuple[float, float, float]:
    """sigma, a number or a (z, y, x) triple, as three finite floats >= 0, and truncate finite and > 0, or ValueError"""
    if isinstance(sigma, (int, float)) and not isinstance(sigma, bool):
        sigma = (sigma,) * 3
    try:
        s = tuple(float(v) for v in sigma)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: sigma must be a number or a (z, y, x) triple of numbers, got {sigma!r}") from None
    if len(s) != 3 or any(isinstance(v, bool) for v in sigma) or not all(math.isfinite(v) and v >= 0.0 for v in s):
        raise ValueError(f"{who}: sigma must be a finite number >= 0 or a (z, y, x) triple of them, got {sigma!r}")
    if isinstance(truncate, bool) or not isinstance(truncate, (int, float)) or not math.isfinite(truncate) or truncate <= 0:
        raise ValueError(f"{who}: truncate must be a finite number > 0, got {truncate!r}")
    return s


def gaussian_radius(sigma: float, truncate: float = 4.0) -> int:
    """R = int(truncate * sigma + 0.5), scipy.ndimage.gaussian_filter's radius: the kernel has the taps k = -R .. R."""
    return int(float(truncate) * float(sigma) + 0.5)


@functools.lru_cache(maxsize=64)
def _gauss_taps(sigma: float, truncate: float):
    """(R, the half-kernel w[0 .. R], the tail sums T[i] = sum_{k >= i} w[k]): fp64 lists, w normalised over k = -R .. R in fp64"""
    R = gaussian_radius(sigma, truncate)
    if R == 0:
        return 0, [1.0], [1.0]
    e = [math.exp(-0.5 * k * k / (sigma * sigma)) for k in range(R + 1)]
    total = math.fsum(e + e[1:])
    w = [v / total for v in e]
    return R, w, [math.fsum(w[i:]) for i in range(R + 1)]


@functools.lru_cache(maxsize=64)
def _gauss_host(sigma: float, truncate: float):
    """(R, w, T) as host float arrays for the C ABI: rounded to fp32 once, here"""
    R, w, t = _gauss_taps(sigma, truncate)
    return R, (ctypes.c_float * (R + 1))(*w), (ctypes.c_float * (R + 1))(*t)


def gaussian_kernel1d(sigma: float, truncate: float = 4.0) -> Tensor:
    """The 2 R + 1 weights gaussian_smooth uses along an axis with this sigma, a float32 tensor on the host: R =
    int(truncate * sigma + 0.5), w[k] = exp(-k^2 / 2 sigma^2) / sum_k exp(-k^2 / 2 sigma^2) for k = -R .. R, computed and
    normalised in fp64 and rounded to fp32 once.  sigma = 0 (or any R = 0): the single weight 1."""
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)):
        raise ValueError(f"gaussian_kernel1d: sigma must be one number, got {sigma!r}")
    s = _gauss_sigmas("gaussian_kernel1d", sigma, truncate)[0]
    if float(truncate) * s > GAUSS_MAX_RADIUS:
        raise ValueError(f"gaussian_kernel1d: truncate * sigma must be at most {GAUSS_MAX_RADIUS} (sigma <= 8 at truncate = 4), got "
                         f"sigma {sigma} with truncate {truncate}")
    R, w, _ = _gauss_host(s, float(truncate))
    half = list(w)
    return torch.tensor(half[:0:-1] + half, dtype=torch.float32)


def _gauss_plan(who: str, x, sigma, truncate):
    """The checks of gaussian_smooth -> None (nothing to do) or ((rz, ry, rx), [w_z, w_y, w_x], [t_z, t_y, t_x]).
    KeymorphHipError for a tensor that is not on the GPU, ValueError for the rest -- before anything is allocated."""
    _need_gpu_f32(who, "x", x)
    sig = _gauss_sigmas(who, sigma, truncate)
    if x.dim() != 5 or x.numel() == 0:
        raise ValueError(f"{who}: expected a non-empty (N, C, D, H, W) volume, got {tuple(x.shape)}")
    N, C, D, H, W = x.shape
    radii = tuple(gaussian_radius(s, truncate) for s in sig)
    if float(truncate) * max(sig) > GAUSS_MAX_RADIUS:              # so R = int(truncate * sigma + 0.5) <= 32 as well
        raise ValueError(f"{who}: truncate * sigma must be at most {GAUSS_MAX_RADIUS} per axis (sigma <= 8 at truncate = 4), got "
                         f"sigma {sig} with truncate {truncate}")
    if D * H * W >= GAUSS_MAX_PLANE or N * C > GAUSS_MAX_PLANES:
        raise ValueError(f"{who}: a channel plane must have fewer than 2^29 voxels and N * C be at most {GAUSS_MAX_PLANES}, got "
                         f"{tuple(x.shape)}")
    if max(radii) == 0:
        return None
    host = [_gauss_host(s, float(truncate)) for s in sig]
    return radii, [h[1] for h in host], [h[2] for h in host]


def _gauss_call(x: Tensor, plan, transpose: bool) -> Tensor:
    lib = _lib.load()
    radii, w, t = plan
    N, C, D, H, W = x.shape
    out = torch.empty_like(x)
    nbytes = int(lib.kmh_gauss_ws_bytes(N, C, D, H, W, *radii))
    ws = workspace(nbytes, x.device, "gauss") if nbytes else None
    if _lib.profiler.enabled:  # every active axis reads and writes each voxel once
        _lib.profiler.meta = {"bytes": 8.0 * x.numel() * sum(1 for r in radii if r)}
    host = [ctypes.addressof(a) for a in w]
    if transpose:
        check(lib.kmh_gauss_bwd(_p(x), _p(out), _p(ws), N, C, D, H, W, *radii, *host, *[ctypes.addressof(a) for a in t],
                                _stream()), "kmh_gauss_bwd")
    else:
        check(lib.kmh_gauss_fwd(_p(x), _p(out), _p(ws), N, C, D, H, W, *radii, *host, _stream()), "kmh_gauss_fwd")
    return out


class _GaussianSmooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        ctx.plan = plan
        return _gauss_call(x.contiguous(), plan, False)

    @staticmethod
    def backward(ctx, gout):
        return _gauss_call(_prep(gout, "gout"), ctx.plan, True), None


def gaussian_smooth(x: Tensor, sigma, truncate: float = 4.0) -> Tensor:
    """x (N, C, D, H, W) float32 on the GPU smoothed by a Gaussian of `sigma` voxels, a number or a (z, y, x) triple:
    scipy.ndimage.gaussian_filter(x, sigma, mode="nearest", truncate=truncate) on the three spatial axes.  Per axis with
    R = int(truncate * sigma + 0.5) > 0:  out[i] = sum_{k=-R..R} w[k] x[clamp(i + k, 0, n - 1)]  with gaussian_kernel1d's weights,
    along W, then H, then D; an axis with R = 0 is not touched, and when that is every axis the result is x itself (no copy).
    Differentiable in x: the backward is the exact transpose, a gather without atomics.  Runs repeat bit for bit and a batch
    equals its samples.  ValueError: sigma negative or not finite, truncate * sigma > 32 on an axis (sigma <= 8 at truncate = 4;
    the kernels hold at most 32 taps on either side of the centre), a channel
    plane of 2^29 voxels or more, N * C > 65535."""
    plan = _gauss_plan("gaussian_smooth", x, sigma, truncate)
    if plan is None:
        return x
    return _GaussianSmooth.apply(x, plan)


class _WarpMSE(torch.autograd.Function):
    """Fused align_img + MSELoss (one pass; the warped volume is still returned).  When the grid needs a gradient the
    same pass also writes d(loss)/d(grid) -- the MSE cotangent is known inside the warp -- so the backward is a no-op
    for the default cotangent 1 (a device-side check) instead of an MSE-backward pass plus a grid-backward pass."""

    @staticmethod
    def forward(ctx, x, grid, fixed):
        lib = _lib.load()
        x, grid, fixed = _prep(x), _prep(grid), _prep(fixed)
        N, C, D, H, W = x.shape
        _, Do, Ho, Wo, _ = grid.shape
        out = torch.empty((N, C, Do, Ho, Wo), dtype=torch.float32, device=x.device)
        assert fixed.shape == out.shape
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ctx.dgrid = None
        if ctx.needs_input_grad[1] and (grid.numel() & 3) == 0:
            dgrid = torch.empty_like(grid)
            if _lib.profiler.enabled:  # grid 12 + dgrid 12 + C * (volume 4 + fixed 4 + out 4) B per output voxel
                _lib.profiler.meta = {"bytes": float(N * Do * Ho * Wo) * (24 + 12 * C)}
            rc = lib.kmh_warp_mse_fwd_grad(_p(x), _p(grid), _p(fixed), _p(out), _p(loss), _p(dgrid), N, C, D, H, W, Do,
                                           Ho, Wo, _p(_reduce_ws(x.device)), _stream())
            if rc == 0:
                ctx.dgrid = dgrid
            elif rc != -22:
                check(rc, "kmh_warp_mse_fwd_grad")
        if ctx.dgrid is None:
            if _lib.profiler.enabled:  # grid 12 B + C*(volume 4 + fixed 4 + out 4) B per output voxel
                _lib.profiler.meta = {"bytes": float(N * Do * Ho * Wo) * (12 + 12 * C)}
            check(lib.kmh_warp_mse_fwd(_p(x), _p(grid), _p(fixed), _p(out), _p(loss), N, C, D, H, W, Do, Ho, Wo,
                                       _p(_reduce_ws(x.device)), _stream()), "kmh_warp_mse_fwd")
        # always saved (inputs and the returned output: no extra memory): the plain three-launch backward serves a
        # grid that needed the non-fused route and every backward after the first one
        ctx.save_for_backward(x, grid, fixed, out)
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    def backward(ctx, gloss, _gout):
        lib = _lib.load()
        if ctx.dgrid is not None:
            # d(loss)/d(grid) was written by the forward pass: the first backward hands that buffer out, scaled in place
            # by the cotangent (a device-side check makes the usual cotangent 1 a no-op: no pass over 200 MB, no host
            # synchronisation).  A second backward over a retained graph recomputes it from the saved tensors below.
            dgrid, ctx.dgrid = ctx.dgrid, None
            gl = _prep(gloss).reshape(1)
            check(lib.kmh_scale_unless_one(_p(dgrid), dgrid.numel(), _p(gl), _stream()), "kmh_scale_unless_one")
            return None, dgrid, None
        x, grid, fixed, out = ctx.saved_tensors
        N, C, D, H, W = x.shape
        _, Do, Ho, Wo, _ = grid.shape
        gout = torch.empty_like(out)
        gl = _prep(gloss).reshape(1)
        check(lib.kmh_mse_bwd(_p(out), _p(fixed), _p(gl), out.numel(), _p(gout), _stream()), "kmh_mse_bwd")
        dgrid = torch.empty_like(grid)
        if _lib.profiler.enabled:
            _lib.profiler.meta = {"bytes": float(N * Do * Ho * Wo) * (24 + 8 * C)}
        check(lib.kmh_grid_sample3d_bwd_grid(_p(x), _p(grid), _p(gout), _p(dgrid), N, C, D, H, W, Do, Ho, Wo,
                                             _stream()), "kmh_grid_sample3d_bwd_grid")
        return None, dgrid, None


def warp_mse(x: Tensor, grid: Tensor, fixed: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (mse(fixed, warp(x, grid)), warp(x, grid)); gradient flows to ``grid`` only."""
    return _WarpMSE.apply(x, grid, fixed)


# --------------------------------------------------------------------------
# a12 / a13  losses
# --------------------------------------------------------------------------
class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        lib = _lib.load()
        a, b = _prep(a), _prep(b)
        assert a.shape == b.shape
        out = torch.empty((), dtype=torch.float32, device=a.device)
        check(lib.kmh_mse_fwd(_p(a), _p(b), a.numel(), _p(out), _p(_reduce_ws(a.device)), _stream()), "kmh_mse_fwd")
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        a, b = ctx.saved_tensors
        g = _prep(g).reshape(1)
        da = torch.empty_like(a)
        check(lib.kmh_mse_bwd(_p(a), _p(b), _p(g), a.numel(), _p(da), _stream()), "kmh_mse_bwd")
        return (da if ctx.needs_input_grad[0] else None), (-da if ctx.needs_input_grad[1] else None)


def mse_loss(a: Tensor, b: Tensor) -> Tensor:
    return _MSE.apply(a, b)


# rows per launch of kmh_dice_sums / kmh_rows_axpby: the sums' block partials (rows, blocks, 3) must fit the 65536 x 3
# reduction workspace and the launch grid has one row of blocks per row
_DICE_ROWS = 32768


class _DiceRows(torch.autograd.Function):
    """per-row Dice loss 1 - (2 sum tp + 1)/(sum p^2 + sum t^2 + 1); rows = n*c."""

    @staticmethod
    def forward(ctx, pred, target):
        lib = _lib.load()
        pred, target = _prep(pred), _prep(target)
        R, V = pred.shape
        sums = torch.empty((R, 3), dtype=torch.float32, device=pred.device)
        for r0 in range(0, R, _DICE_ROWS):
            r = min(_DICE_ROWS, R - r0)
            check(lib.kmh_dice_sums(_p(pred[r0:]), _p(target[r0:]), r, V, _p(sums[r0:]), _p(_reduce_ws(pred.device)),
                                    _stream()), "kmh_dice_sums")
        num = 2 * sums[:, 0] + 1
        den = sums[:, 1] + sums[:, 2] + 1
        ctx.save_for_backward(pred, target, num, den)
        return 1 - num / den

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        pred, target, num, den = ctx.saved_tensors
        R, V = pred.shape
        g = _prep(g)
        ca = (-2.0 * g / den).contiguous()
        cb = (2.0 * g * num / (den * den)).contiguous()
        dpred = torch.empty_like(pred)
        for r0 in range(0, R, _DICE_ROWS):
            r = min(_DICE_ROWS, R - r0)
            check(lib.kmh_rows_axpby(_p(target[r0:]), _p(pred[r0:]), _p(ca[r0:]), _p(cb[r0:]), r, V, _p(dpred[r0:]),
                                     _stream()), "kmh_rows_axpby")
        return dpred, None


def dice_rows(pred: Tensor, target: Tensor) -> Tensor:
    return _DiceRows.apply(pred, target)


class _WarpDiceRows(torch.autograd.Function):
    """Dice rows of align_img(grid, x) against `fixed` WITHOUT the warped tensor: one pass for the three sums per (n, c)
    (kmh_warp_dice_sums), one pass for d/d(grid) (kmh_warp_dice_bwd_grid; the warp is recomputed, nothing is stored).
    scripts/train.py:146-164 with loss_fn == "dice"; keymorph/utils.py:14-21 + keymorph/loss_ops.py:16-63.
    Both segmentations are first checked for being exactly one-hot ON THE DEVICE (kmh_onehot_to_labels: one streaming
    read each, writes byte label maps + a flag); when they are -- one_hot() of a label map, nearest-sampled augmentation --
    the two passes read one byte per voxel instead of 4 C; a soft segmentation clears the flag and the same launches read
    the float tensors.  No host synchronisation decides; the results are bit-identical either way."""

    @staticmethod
    def forward(ctx, x, grid, fixed):
        lib = _lib.load()
        x, grid, fixed = _prep(x), _prep(grid), _prep(fixed)
        N, C, D, H, W = x.shape
        _, Do, Ho, Wo, _ = grid.shape
        assert fixed.shape == (N, C, Do, Ho, Wo), "the fixed segmentation must have the warped tensor's shape"
        sums = torch.empty((N * C, 3), dtype=torch.float32, device=x.device)
        labx = labf = gate = None
        # (label maps pay from ~4 channels on: at C = 1 the class loop costs more than the one gather it saves -- 0.175 vs 0.102 ms)
        if 4 <= C <= 255 and not os.environ.get("KEYMORPH_DICE_NO_LABELS"):
            labx = torch.empty((N, D * H * W), dtype=torch.uint8, device=x.device)
            labf = torch.empty((N, Do * Ho * Wo), dtype=torch.uint8, device=x.device)
            gate = torch.ones(1, dtype=torch.int32, device=x.device)
            check(lib.kmh_onehot_to_labels(_p(x), N, C, D * H * W, _p(labx), _p(gate), _stream()), "kmh_onehot_to_labels")
            check(lib.kmh_onehot_to_labels(_p(fixed), N, C, Do * Ho * Wo, _p(labf), _p(gate), _stream()),
                  "kmh_onehot_to_labels")
        if _lib.profiler.enabled:      # grid 12 B + C * (gathered volume 4 + fixed 4) per output voxel
            _lib.profiler.meta = {"bytes": float(N * Do * Ho * Wo) * (12 + 8 * C)}
        check(lib.kmh_warp_dice_sums(_p(x), _p(grid), _p(fixed), _p(sums), N, C, D, H, W, Do, Ho, Wo, _p(labx), _p(labf),
                                     _p(gate), _p(_reduce_ws(x.device)), _stream()), "kmh_warp_dice_sums")
        num = 2 * sums[:, 0] + 1
        den = sums[:, 1] + sums[:, 2] + 1
        ctx.labels = (labx, labf, gate)
        ctx.save_for_backward(x, grid, fixed, num, den)
        return (1 - num / den).view(N, C)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, grid, fixed, num, den = ctx.saved_tensors
        labx, labf, gate = ctx.labels
        N, C, D, H, W = x.shape
        _, Do, Ho, Wo, _ = grid.shape
        g = _prep(g).reshape(-1)
        ca = (-2.0 * g / den).contiguous()
        cb = (2.0 * g * num / (den * den)).contiguous()
        dgrid = torch.empty_like(grid)
        if _lib.profiler.enabled:      # the same reads + 12 B of grid gradient
            _lib.profiler.meta = {"bytes": float(N * Do * Ho * Wo) * (24 + 8 * C)}
        check(lib.kmh_warp_dice_bwd_grid(_p(x), _p(grid), _p(fixed), _p(ca), _p(cb), _p(dgrid), N, C, D, H, W, Do, Ho, Wo,
                                         _p(labx), _p(labf), _p(gate), _stream()), "kmh_warp_dice_bwd_grid")
        return None, dgrid, None


def warp_dice_ok(x: Tensor, grid: Tensor) -> bool:
    """does the fused warp + Dice pass apply?  The size conditions are the library's own (`kmh_warp_dice_ok`, the same
    predicate its two entry points return -22 on: W >= 2, < 2^30 voxels per channel plane, <= 128 channels, N * C <= 65536
    rows, the lane-contiguous sampler not switched off by KMH_SAMPLER_OLD); on top of them the grid must be the only input
    that needs a gradient (`fixed.requires_grad` is the caller's check: loss_ops.warp_dice_loss)."""
    if not (x.dim() == 5 and grid.dim() == 5 and not x.requires_grad):
        return False
    N, C, D, H, W = (int(v) for v in x.shape)
    return bool(_lib.load().kmh_warp_dice_ok(N, C, D, H, W))


def warp_dice_rows(x: Tensor, grid: Tensor, fixed: Tensor) -> Tensor:
    """-> (N, C) rows 1 - (2 sum t p + 1) / (sum p^2 + sum t^2 + 1) with p = align_img(grid, x), t = fixed; the gradient
    flows to ``grid`` only."""
    return _WarpDiceRows.apply(x, grid, fixed)


def argmax_onehot(pred: Tensor) -> Tensor:
    """(N, C, V) -> the one-hot of torch.argmax over the channels, float32: the first NaN if a voxel has one (in whichever
    channel), otherwise the first maximum (+0 == -0)."""
    lib = _lib.load()
    pred = _prep(pred)
    N, C, V = pred.shape
    out = torch.empty_like(pred)
    check(lib.kmh_argmax_onehot(_p(pred), N, C, V, _p(out), _stream()), "kmh_argmax_onehot")
    return out


# --------------------------------------------------------------------------
# a9 / a8  grid generators
# --------------------------------------------------------------------------
class _AffineGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mat, D, H, W):
        lib = _lib.load()
        mat = _prep(mat)
        N = mat.shape[0]
        assert mat.shape[1:] == (3, 4)
        out = torch.empty((N, D, H, W, 3), dtype=torch.float32, device=mat.device)
        check(lib.kmh_affine_grid_fwd(_p(mat), _p(out), N, D, H, W, _stream()), "kmh_affine_grid_fwd")
        ctx.dims = (N, D, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        N, D, H, W = ctx.dims
        g = _prep(g)
        dmat = torch.empty((N, 3, 4), dtype=torch.float32, device=g.device)
        check(lib.kmh_affine_grid_bwd(_p(g), _p(dmat), N, D, H, W, _p(_reduce_ws(g.device)), _stream()),
              "kmh_affine_grid_bwd")
        return dmat, None, None, None


def affine_grid(mat34: Tensor, shape: Sequence[int]) -> Tensor:
    D, H, W = (int(s) for s in shape)
    return _AffineGrid.apply(mat34, D, H, W)


class _TpsGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, ctrl, D, H, W):
        lib = _lib.load()
        theta, ctrl = _prep(theta), _prep(ctrl)
        N, T, _ = ctrl.shape
        assert theta.shape == (N, T + 4, 3)
        out = torch.empty((N, D, H, W, 3), dtype=torch.float32, device=ctrl.device)
        check(lib.kmh_tps_grid_fwd(_p(theta), _p(ctrl), _p(out), N, T, D, H, W, _stream()), "kmh_tps_grid_fwd")
        ctx.save_for_backward(theta, ctrl)
        ctx.dims = (N, T, D, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        theta, ctrl = ctx.saved_tensors
        N, T, D, H, W = ctx.dims
        g = _prep(g)
        dtheta = torch.empty_like(theta)
        dctrl = torch.empty_like(ctrl)
        ws = workspace(int(lib.kmh_tps_grid_bwd_ws_bytes(N, T, D, H, W)), g.device, "tps_bwd")
        check(lib.kmh_tps_grid_bwd(_p(g), _p(theta), _p(ctrl), _p(dtheta), _p(dctrl), N, T, D, H, W, _p(ws),
                                   _stream()), "kmh_tps_grid_bwd")
        return dtheta, dctrl, None, None, None


def tps_grid(theta: Tensor, ctrl: Tensor, shape: Sequence[int]) -> Tensor:
    D, H, W = (int(s) for s in shape)
    return _TpsGrid.apply(theta, ctrl, D, H, W)


# --------------------------------------------------------------------------
# free-form deformation: cubic B-spline control lattice -> grid, and the lattice's bending penalty (csrc/bspline.hip)
# --------------------------------------------------------------------------
def bspline_lattice_shape(shape: Sequence[int], spacing: int) -> Tuple[int, int, int]:
    """(Cz, Cy, Cx) of the control lattice with one cell per `spacing` voxels: ceil(n / spacing) + 3 per axis."""
    spacing = int(spacing)
    dims = tuple(int(n) for n in shape)
    if len(dims) != 3 or min(dims) < 1 or spacing < 1:
        raise ValueError(f"bspline_lattice_shape: expected three positive sizes and a positive spacing, got {tuple(shape)}, {spacing}")
    return tuple(-(-n // spacing) + 3 for n in dims)


def _lattice_check(t, name, who):
    _need_gpu_f32(who, name, t)
    if t.dim() != 5 or t.shape[0] < 1 or t.shape[1] != 3 or min(t.shape[2:]) < 4:
        raise ValueError(f"{who}: {name} must be (N, 3, Cz, Cy, Cx) with every C >= 4, got {tuple(t.shape)}")


class _BsplineGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctrl, mat, D, H, W):
        lib = _lib.load()
        N, _, Cz, Cy, Cx = ctrl.shape
        out = torch.empty((N, D, H, W, 3), dtype=torch.float32, device=ctrl.device)
        if _lib.profiler.enabled:  # 12 B written per voxel
            _lib.profiler.meta = {"bytes": 12.0 * N * D * H * W}
        check(lib.kmh_bspline_grid_fwd(_p(ctrl), _p(mat), _p(out), N, D, H, W, Cz, Cy, Cx, _stream()), "kmh_bspline_grid_fwd")
        ctx.dims = (N, D, H, W, Cz, Cy, Cx)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        N, D, H, W, Cz, Cy, Cx = ctx.dims
        g = _prep(g)
        dctrl = torch.empty((N, 3, Cz, Cy, Cx), dtype=torch.float32, device=g.device)
        ws = workspace(int(lib.kmh_bspline_grid_ws_bytes(*ctx.dims)), g.device, "bspline_bwd")
        if _lib.profiler.enabled:  # 12 B read per voxel
            _lib.profiler.meta = {"bytes": 12.0 * N * D * H * W}
        check(lib.kmh_bspline_grid_bwd(_p(g), _p(dctrl), *ctx.dims, _p(ws), _stream()), "kmh_bspline_grid_bwd")
        return dctrl, None, None, None, None


def bspline_grid(ctrl: Tensor, shape: Sequence[int], mat: Optional[Tensor] = None) -> Tensor:
    """The sampling grid (N, D, H, W, 3) of a free-form deformation: ctrl (N, 3, Cz, Cy, Cx) float32 on the current GPU, every
    C >= 4, channel k = the displacement of grid component k, in the grid's own order (x, y, z) and normalised units, at the
    control points of a uniform cubic B-spline lattice with C - 3 cells over [-1, 1] per axis:
    voxel centre g = (2 i + 1) / S - 1, u = (g + 1) (C - 3) / 2, cell = floor(u), t = u - cell, weights B0..B3(t) on control points
    cell .. cell + 3, and out = base + sum_{c,b,a} Bz_c By_b Bx_a ctrl[:, :, cz + c, cy + b, cx + a].
    base = fields.identity_grid (mat None) or exactly ops.affine_grid(mat, shape) for mat (N, 3, 4).  Differentiable in ctrl only
    (mat is data: one that requires grad raises); two calls give bit-identical grids and gradients, a batch equals its samples."""
    _lattice_check(ctrl, "ctrl", "bspline_grid")
    dims = tuple(int(s) for s in shape)
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 1 << 31:
        raise ValueError(f"bspline_grid: shape must be three positive sizes (D, H, W) with fewer than 2^31 voxels, got {tuple(shape)}")
    if mat is not None:
        _need_gpu("bspline_grid", "mat", mat)
        if mat.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("bspline_grid: mat requires grad, and bspline_grid is differentiable in ctrl only: pass mat.detach()")
        if mat.dtype != torch.float32 or tuple(mat.shape) != (ctrl.shape[0], 3, 4):
            raise ValueError(f"bspline_grid: mat must be float32 ({ctrl.shape[0]}, 3, 4), got {mat.dtype} {tuple(mat.shape)}")
        mat = mat.detach().contiguous()
    return _BsplineGrid.apply(ctrl.contiguous(), mat, *dims)


class _BsplineBending(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q):
        N, _, Cz, Cy, Cx = q.shape
        out = torch.empty((N,), dtype=torch.float32, device=q.device)
        lib = _lib.load()
        ws = workspace(int(lib.kmh_bspline_bending_ws_bytes(N)), q.device, "bspline_bending")
        check(lib.kmh_bspline_bending_fwd(_p(q), _p(out), N, Cz, Cy, Cx, _p(ws), _stream()), "kmh_bspline_bending_fwd")
        ctx.save_for_backward(q)
        return out

    @staticmethod
    def backward(ctx, g):
        (q,) = ctx.saved_tensors
        N, _, Cz, Cy, Cx = q.shape
        g = _prep(g)
        dq = torch.empty_like(q)
        check(_lib.load().kmh_bspline_bending_bwd(_p(q), _p(g), _p(dq), N, Cz, Cy, Cx, _stream()), "kmh_bspline_bending_bwd")
        return dq


def bspline_bending(q: Tensor) -> Tensor:
    """(N,): per sample, the sum over the three lattice axes of the mean of (q[i - 1] - 2 q[i] + q[i + 1])^2 over that axis'
    differenced tensor; q (N, 3, Cz, Cy, Cx) float32 on the current GPU, every C >= 4, any units.  0 for a lattice that is linear
    in its indices.  Differentiable; fixed-order sums (bit-identical runs, a batch equals its samples)."""
    _lattice_check(q, "q", "bspline_bending")
    return _BsplineBending.apply(q.contiguous())


# --------------------------------------------------------------------------
# diffeomorphic grids: a lattice of velocities exponentiated by scaling and squaring (csrc/svf.hip)
# --------------------------------------------------------------------------
SVF_MAX_STEPS = 12


def _svf_forward(ctrl, mat, dims, steps, keep):
    """(grid or u_K, [u_0 .. u_{K-1}] if keep).  mat False: the displacement u_K is returned as it is (no finish)."""
    lib = _lib.load()
    N, _, Cz, Cy, Cx = ctrl.shape
    D, H, W = dims
    small = ctrl * (2.0 ** -steps) if steps else ctrl                 # a power of two: exact
    u = torch.empty((N, D, H, W, 3), dtype=torch.float32, device=ctrl.device)
    check(lib.kmh_bspline_disp_fwd(_p(small), _p(u), N, D, H, W, Cz, Cy, Cx, _stream()), "kmh_bspline_disp_fwd")
    us = []
    for _ in range(steps):
        nxt = torch.empty_like(u)
        if _lib.profiler.enabled:  # 12 B read + 12 B written per voxel, the gathers from cache
            _lib.profiler.meta = {"bytes": 24.0 * N * D * H * W}
        check(lib.kmh_svf_compose(_p(u), None, None, _p(nxt), N, D, H, W, _stream()), "kmh_svf_compose")
        if keep:
            us.append(u)
        u = nxt
    if mat is not False:
        check(lib.kmh_svf_finish_fwd(_p(u), _p(mat), _p(u), N, D, H, W, _stream()), "kmh_svf_finish_fwd")
    return u, us


class _SvfGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctrl, mat, steps, D, H, W):
        grid, us = _svf_forward(ctrl, mat, (D, H, W), steps, True)
        ctx.save_for_backward(*us)
        ctx.mat, ctx.steps, ctx.dims = mat, steps, (ctrl.shape[0], D, H, W, *ctrl.shape[2:])
        return grid

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        us, steps, mat = ctx.saved_tensors, ctx.steps, ctx.mat
        N, D, H, W, Cz, Cy, Cx = ctx.dims
        g = _prep(g)
        du = torch.empty_like(g)
        amax = torch.zeros((steps + 1, N), dtype=torch.int32, device=g.device)      # float bits of the largest finite |cotangent|
        check(lib.kmh_svf_finish_bwd(_p(g), _p(mat), _p(du), _p(amax[steps]), N, D, H, W, _stream()), "kmh_svf_finish_bwd")
        if steps:
            ws = workspace(int(lib.kmh_svf_square_bwd_ws_bytes(N, D, H, W)), g.device, "svf_bwd")
            for k in range(steps - 1, -1, -1):
                if _lib.profiler.enabled:  # 32 cleared + 36 + 32 + 24 B per voxel, and 24 eight-byte atomics
                    _lib.profiler.meta = {"bytes": 124.0 * N * D * H * W}
                check(lib.kmh_svf_square_bwd(_p(us[k]), _p(du), _p(du), _p(amax[k + 1]), _p(amax[k]) if k else None, N, D, H, W,
                                             _p(ws), _stream()), "kmh_svf_square_bwd")
        dctrl = torch.empty((N, 3, Cz, Cy, Cx), dtype=torch.float32, device=g.device)
        ws = workspace(int(lib.kmh_bspline_grid_ws_bytes(N, D, H, W, Cz, Cy, Cx)), g.device, "bspline_bwd")
        check(lib.kmh_bspline_grid_bwd(_p(du), _p(dctrl), N, D, H, W, Cz, Cy, Cx, _p(ws), _stream()), "kmh_bspline_grid_bwd")
        if steps:
            dctrl = dctrl * (2.0 ** -steps)
        return dctrl, None, None, None, None, None


def _svf_check(who, ctrl, shape, steps, mat):
    _lattice_check(ctrl, "ctrl", who)
    dims = tuple(int(s) for s in shape)
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] * 3 >= 1 << 30:
        raise ValueError(f"{who}: shape must be three positive sizes (D, H, W) with D * H * W * 3 < 2^30, got {tuple(shape)}")
    if isinstance(steps, bool) or int(steps) != steps or not 0 <= int(steps) <= SVF_MAX_STEPS:
        raise ValueError(f"{who}: steps must be an integer in 0 .. {SVF_MAX_STEPS}, got {steps!r}")
    if mat is not None:
        _need_gpu(who, "mat", mat)
        if mat.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{who}: mat requires grad, and {who} is differentiable in ctrl only: pass mat.detach()")
        if mat.dtype != torch.float32 or tuple(mat.shape) != (ctrl.shape[0], 3, 4):
            raise ValueError(f"{who}: mat must be float32 ({ctrl.shape[0]}, 3, 4), got {mat.dtype} {tuple(mat.shape)}")
        if min(dims) < 2:
            raise ValueError(f"{who}: with a matrix every axis needs at least two voxels, got {dims}")
        mat = mat.detach().contiguous()
    return dims, int(steps), mat


def svf_grid(ctrl: Tensor, shape: Sequence[int], steps: int = 6, mat: Optional[Tensor] = None) -> Tensor:
    """The sampling grid (N, D, H, W, 3) of a diffeomorphism: ctrl (N, 3, Cz, Cy, Cx) float32 on the current GPU is a cubic B-spline
    lattice of VELOCITIES in bspline_grid's units and order, and the grid is the exponential of that stationary velocity field by
    scaling and squaring, in displacement form:
        u_0 = the spline of ctrl 2^-steps (no base),   u_{k+1}[w] = u_k[w] + U_k(Ids[w] + u_k[w])   `steps` times,
    U_k the trilinear interpolant of u_k with border clamping (the sampler's), Ids = fields.identity_grid; then
        grid = Ids + u_K   (mat None)   or   grid = ops.affine_grid(mat, shape) + L (s * u_K),  L = mat[:, :, :3], s = S / (S - 1) per axis
    -- the matrix applied to the deformed point.  A zero lattice gives exactly the base; steps = 0 is bspline_grid (with the matrix
    applied analytically instead of added to).  The inverse map is svf_grid(-ctrl, ...): see io.svf_grid(inverse=True).
    steps in 0 .. 12; D * H * W * 3 < 2^30.  Differentiable in ctrl only (mat is data: one that requires grad raises); the backward
    keeps u_0 .. u_{K-1} (12 B per voxel each) and sums its scatter in 64-bit fixed point, so two calls give bit-identical grids and
    gradients and a batch equals its samples."""
    dims, steps, mat = _svf_check("svf_grid", ctrl, shape, steps, mat)
    return _SvfGrid.apply(ctrl.contiguous(), mat, steps, *dims)


def svf_displacement(ctrl: Tensor, shape: Sequence[int], steps: int = 6) -> Tensor:
    """u_K of svf_grid (N, D, H, W, 3), normalised, on the voxel-centre lattice: svf_grid(ctrl, shape, steps) is
    fields.identity_grid + this, bit for bit.  Not differentiable (ctrl is detached)."""
    dims, steps, _ = _svf_check("svf_displacement", ctrl, shape, steps, None)
    return _svf_forward(ctrl.detach().contiguous(), False, dims, steps, False)[0]


def svf_compose(u: Tensor, first: Tensor, add: Optional[Tensor] = None) -> Tensor:
    """add + U(first): the displacement u (N, D, H, W, 3) interpolated (trilinear, border-clamped) at the grid `first` of the same
    shape, plus `add` (None: first itself, which gives the grid first + U(first)).  Not differentiable: inputs are detached."""
    for name, t in (("u", u), ("first", first), ("add", first if add is None else add)):
        _need_gpu_f32("svf_compose", name, t)
        if t.dim() != 5 or t.shape[-1] != 3 or t.shape != u.shape or t.numel() == 0:
            raise ValueError(f"svf_compose: {name} must be (N, D, H, W, 3) like u, got {tuple(t.shape)} and {tuple(u.shape)}")
        if t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"svf_compose: {name} requires grad, and svf_compose is not differentiable: pass {name}.detach()")
    u, first = u.detach().contiguous(), first.detach().contiguous()
    add = first if add is None else add.detach().contiguous()
    N, D, H, W, _ = u.shape
    out = torch.empty_like(u)
    check(_lib.load().kmh_svf_compose(_p(u), _p(first), _p(add), _p(out), N, D, H, W, _stream()), "kmh_svf_compose")
    return out


# --------------------------------------------------------------------------
# dense displacement fields as a transform model: the grid of a planar voxel displacement, its step scale and the greedy
# composition (csrc/dense.hip)
# --------------------------------------------------------------------------
def _disp_check(who, name, t, like=None):
    """t: a non-empty float32 (N, 3, D, H, W) field on the GPU with D * H * W * 3 < 2^30 (and of like's shape), or an error."""
    _need_gpu_f32(who, name, t)
    if t.dim() != 5 or t.shape[1] != 3 or t.numel() == 0:
        raise ValueError(f"{who}: {name} must be a non-empty displacement field (N, 3, D, H, W), got {tuple(t.shape)}")
    if t.shape[2] * t.shape[3] * t.shape[4] * 3 >= 1 << 30 or t.shape[0] > 65535:
        raise ValueError(f"{who}: {name} needs D * H * W * 3 < 2^30 and N <= 65535, got {tuple(t.shape)}")
    if like is not None and t.shape != like.shape:
        raise ValueError(f"{who}: {name} must have the field's shape {tuple(like.shape)}, got {tuple(t.shape)}")


class _DisplacementGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, mat):
        N, _, D, H, W = disp.shape
        ctx.mat = mat
        grid = torch.empty((N, D, H, W, 3), dtype=torch.float32, device=disp.device)
        if _lib.profiler.enabled:  # 12 B read + 12 B written per voxel
            _lib.profiler.meta = {"bytes": 24.0 * N * D * H * W}
        check(_lib.load().kmh_disp_grid_fwd(_p(disp), _p(mat), _p(grid), N, D, H, W, _stream()), "kmh_disp_grid_fwd")
        return grid

    @staticmethod
    def backward(ctx, g):
        g = _prep(g)
        N, D, H, W, _ = g.shape
        ddisp = torch.empty((N, 3, D, H, W), dtype=torch.float32, device=g.device)
        if _lib.profiler.enabled:
            _lib.profiler.meta = {"bytes": 24.0 * N * D * H * W}
        check(_lib.load().kmh_disp_grid_bwd(_p(g), _p(ctx.mat), _p(ddisp), N, D, H, W, _stream()), "kmh_disp_grid_bwd")
        return ddisp, None


def displacement_grid(disp: Tensor, mat: Optional[Tensor] = None) -> Tensor:
    """The sampling grid (N, D, H, W, 3) of a dense displacement field: disp (N, 3, D, H, W) float32 on the current GPU, channels
    (z, y, x), in voxels of its own lattice (fields.to_displacement's convention), planar so that gaussian_smooth works on it as it
    is.  With u = disp over S / 2 per axis, reordered to xyz:
        grid = Ids + u   (mat None: fields.from_displacement(disp), bit for bit)
        grid = ops.affine_grid(mat, (D, H, W)) + L (s * u),  L = mat[:, :, :3], s = S / (S - 1) per axis   (svf_grid's rule)
    -- the matrix applied to the deformed point.  Differentiable in disp only (mat is data: one that requires grad raises); the
    backward is the per-voxel transpose, a direct planar write without atomics, so runs repeat bit for bit and a batch equals its
    samples.  D * H * W * 3 < 2^30; with a matrix every axis needs two voxels."""
    who = "displacement_grid"
    _disp_check(who, "disp", disp)
    if mat is not None:
        _need_gpu(who, "mat", mat)
        if mat.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{who}: mat requires grad, and {who} is differentiable in disp only: pass mat.detach()")
        if mat.dtype != torch.float32 or tuple(mat.shape) != (disp.shape[0], 3, 4):
            raise ValueError(f"{who}: mat must be float32 ({disp.shape[0]}, 3, 4), got {mat.dtype} {tuple(mat.shape)}")
        if min(disp.shape[2:]) < 2:
            raise ValueError(f"{who}: with a matrix every axis needs at least two voxels, got {tuple(disp.shape[2:])}")
        mat = mat.detach().contiguous()
    return _DisplacementGrid.apply(disp.contiguous(), mat)


def displacement_step_scale(delta: Tensor, step: float) -> Tensor:
    """(N,) float32 on the device: step / max_w |delta[n, :, w]|_2 of an update field delta (N, 3, D, H, W) -- the factor that makes
    its longest vector `step` voxels long.  0 where that maximum is 0.  A voxel whose squared norm is not finite (a NaN, an Inf, an
    overflow) does not enter the maximum.  The maximum is an integer max on float bits: runs repeat bit for bit and a batch equals
    its samples.  Nothing is read back to the host.  Not differentiable."""
    who = "displacement_step_scale"
    _disp_check(who, "delta", delta)
    step = float(step)
    if not math.isfinite(step):
        raise ValueError(f"{who}: step must be finite, got {step!r}")
    delta = delta.detach().contiguous()
    N, _, D, H, W = delta.shape
    out = torch.empty((N,), dtype=torch.float32, device=delta.device)
    if _lib.profiler.enabled:
        _lib.profiler.meta = {"bytes": 12.0 * N * D * H * W}
    check(_lib.load().kmh_disp_step_scale(_p(delta), step, _p(out), N, D, H, W, _stream()), "kmh_disp_step_scale")
    return out


def displacement_update(disp: Tensor, delta: Tensor, scale: Optional[Tensor] = None) -> Tensor:
    """The greedy composition phi <- phi o (Id + d) on displacement fields (N, 3, D, H, W), d = delta * scale[n] (scale (N,) float32
    on the device, read inside the kernel; None: delta itself):
        out[n, :, w] = d[w] + U_n(w + d[w])
    U_n the trilinear interpolant of disp[n] with border clamping, at the sampler's own coordinate of the grid
    fields.from_displacement(d): the result is d + align_img(fields.from_displacement(d), disp), bit for bit, in one kernel.
    Every product and sum is a separately rounded fp32 operation in the order written.  Not differentiable: an input that requires
    grad raises."""
    who = "displacement_update"
    _disp_check(who, "disp", disp)
    _disp_check(who, "delta", delta, disp)
    if scale is not None:
        _need_gpu_f32(who, "scale", scale)
        if tuple(scale.shape) != (disp.shape[0],):
            raise ValueError(f"{who}: scale must be ({disp.shape[0]},), got {tuple(scale.shape)}")
    for name, t in (("disp", disp), ("delta", delta), ("scale", scale)):
        if t is not None and t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{who}: {name} requires grad, and {who} is not differentiable: pass {name}.detach()")
    disp, delta = disp.detach().contiguous(), delta.detach().contiguous()
    scale = None if scale is None else scale.detach().contiguous()
    N, _, D, H, W = disp.shape
    out = torch.empty_like(disp)
    if _lib.profiler.enabled:  # 12 B read + 12 B written per voxel, the gathers from cache
        _lib.profiler.meta = {"bytes": 24.0 * N * D * H * W}
    check(_lib.load().kmh_disp_update(_p(disp), _p(delta), _p(scale), _p(out), N, D, H, W, _stream()), "kmh_disp_update")
    return out


class _TpsPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, ctrl, pts):
        lib = _lib.load()
        theta, ctrl, pts = _prep(theta), _prep(ctrl), _prep(pts)
        N, T, _ = ctrl.shape
        P = pts.shape[1]
        out = torch.empty_like(pts)
        check(lib.kmh_tps_points_fwd(_p(theta), _p(ctrl), _p(pts), _p(out), N, T, P, _stream()), "kmh_tps_points_fwd")
        ctx.save_for_backward(theta, ctrl, pts)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        theta, ctrl, pts = ctx.saved_tensors
        N, T, _ = ctrl.shape
        P = pts.shape[1]
        g = _prep(g)
        dtheta, dctrl, dpts = torch.empty_like(theta), torch.empty_like(ctrl), torch.empty_like(pts)
        ws = workspace(int(lib.kmh_tps_points_bwd_ws_bytes(N, T, P)), g.device, "tps_bwd")
        check(lib.kmh_tps_points_bwd(_p(g), _p(theta), _p(ctrl), _p(pts), _p(dtheta), _p(dctrl), _p(dpts), N, T, P,
                                     _p(ws), _stream()), "kmh_tps_points_bwd")
        return dtheta, dctrl, dpts


def tps_points(theta: Tensor, ctrl: Tensor, pts: Tensor) -> Tensor:
    return _TpsPoints.apply(theta, ctrl, pts)


class _AffinePoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, M, pts):
        lib = _lib.load()
        M, pts = _prep(M), _prep(pts)
        N, P, _ = pts.shape
        out = torch.empty_like(pts)
        check(lib.kmh_affine_points_fwd(_p(M), _p(pts), _p(out), N, P, _stream()), "kmh_affine_points_fwd")
        ctx.save_for_backward(M, pts)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        M, pts = ctx.saved_tensors
        N, P, _ = pts.shape
        g = _prep(g)
        dM, dpts = torch.empty_like(M), torch.empty_like(pts)
        check(lib.kmh_affine_points_bwd(_p(g), _p(M), _p(pts), _p(dM), _p(dpts), N, P, _stream()),
              "kmh_affine_points_bwd")
        return dM, dpts


def affine_points(mat34: Tensor, pts: Tensor) -> Tensor:
    return _AffinePoints.apply(mat34, pts)


# --------------------------------------------------------------------------
# a5 / a6 / a7  fits
# --------------------------------------------------------------------------
class _MatrixFit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, w, kind):
        lib = _lib.load()
        x, y = _prep(x), _prep(y)
        w = None if w is None else _prep(w)
        N, K, _ = x.shape
        M = torch.empty((N, 3, 4), dtype=torch.float32, device=x.device)
        fn = lib.kmh_affine_fit_fwd if kind == "affine" else lib.kmh_rigid_fit_fwd
        check(fn(_p(x), _p(y), _p(w), _p(M), N, K, _stream()), f"kmh_{kind}_fit_fwd")
        ctx.save_for_backward(x, y, M) if w is None else ctx.save_for_backward(x, y, M, w)
        ctx.kind = kind
        return M

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        saved = ctx.saved_tensors
        x, y, M = saved[:3]
        w = saved[3] if len(saved) > 3 else None
        N, K, _ = x.shape
        g = _prep(g)
        dx, dy = torch.empty_like(x), torch.empty_like(y)
        dw = torch.empty_like(w) if (w is not None and ctx.needs_input_grad[2]) else None
        if ctx.kind == "affine":
            check(lib.kmh_affine_fit_bwd(_p(g), _p(x), _p(y), _p(w), _p(M), _p(dx), _p(dy), _p(dw), N, K, _stream()),
                  "kmh_affine_fit_bwd")
        else:
            check(lib.kmh_rigid_fit_bwd(_p(g), _p(x), _p(y), _p(w), _p(dx), _p(dy), _p(dw), N, K, _stream()),
                  "kmh_rigid_fit_bwd")
        return dx, dy, dw, None


def affine_fit(x: Tensor, y: Tensor, w: Optional[Tensor] = None) -> Tensor:
    return _MatrixFit.apply(x, y, w, "affine")


def rigid_fit(x: Tensor, y: Tensor, w: Optional[Tensor] = None) -> Tensor:
    return _MatrixFit.apply(x, y, w, "rigid")


class _AffineInverse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, M):
        lib = _lib.load()
        M = _prep(M)
        Mi = torch.empty_like(M)
        check(lib.kmh_affine_inverse_fwd(_p(M), _p(Mi), M.shape[0], _stream()), "kmh_affine_inverse_fwd")
        ctx.save_for_backward(Mi)
        return Mi

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        (Mi,) = ctx.saved_tensors
        g = _prep(g)
        dM = torch.empty_like(Mi)
        check(lib.kmh_affine_inverse_bwd(_p(g), _p(Mi), _p(dM), Mi.shape[0], _stream()), "kmh_affine_inverse_bwd")
        return dM


def affine_inverse(mat34: Tensor) -> Tensor:
    """(N,3,4) -> top 3 rows of inverse([M; 0 0 0 1])."""
    return _AffineInverse.apply(mat34)


class _TpsFit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctrl, tgt, lmbda, w):
        lib = _lib.load()
        ctrl, tgt, lmbda = _prep(ctrl), _prep(tgt), _prep(lmbda)
        w = None if w is None else _prep(w)
        N, T, _ = ctrl.shape
        assert lmbda.numel() == N
        theta = torch.empty((N, T + 4, 3), dtype=torch.float32, device=ctrl.device)
        # the LU factors must outlive the forward (the backward re-uses them): dedicated buffer
        ws = torch.empty(int(lib.kmh_tps_fit_ws_bytes(N, T)), dtype=torch.uint8, device=ctrl.device)
        check(lib.kmh_tps_fit_fwd(_p(ctrl), _p(tgt), _p(lmbda), _p(w), _p(theta), N, T, _p(ws), _stream()),
              "kmh_tps_fit_fwd")
        ctx.save_for_backward(ctrl, lmbda, theta, ws) if w is None else ctx.save_for_backward(ctrl, lmbda, theta, ws, w)
        return theta

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        saved = ctx.saved_tensors
        ctrl, lmbda, theta, ws = saved[:4]
        w = saved[4] if len(saved) > 4 else None
        N, T, _ = ctrl.shape
        g = _prep(g)
        dctrl, dtgt = torch.empty_like(ctrl), torch.empty_like(ctrl)
        dw = torch.empty_like(w) if (w is not None and ctx.needs_input_grad[3]) else None
        check(lib.kmh_tps_fit_bwd(_p(g), _p(theta), _p(ctrl), _p(lmbda), _p(w), _p(dctrl), _p(dtgt), _p(dw), N, T,
                                  _p(ws), _stream()), "kmh_tps_fit_bwd")
        return dctrl, dtgt, None, dw


def tps_fit(ctrl: Tensor, tgt: Tensor, lmbda: Tensor, w: Optional[Tensor] = None) -> Tensor:
    return _TpsFit.apply(ctrl, tgt, lmbda, w)


# --------------------------------------------------------------------------
# a4  center of mass on a materialised heat-map
# --------------------------------------------------------------------------
class _Com3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat):
        lib = _lib.load()
        feat = _prep(feat)
        N, K, D, H, W = feat.shape
        pts = torch.empty((N, K, 3), dtype=torch.float32, device=feat.device)
        sums = torch.empty((N, K, 4), dtype=torch.float32, device=feat.device)
        check(lib.kmh_com3d_fwd(_p(feat), _p(pts), _p(sums), N, K, D, H, W, _p(_reduce_ws(feat.device)), _stream()),
              "kmh_com3d_fwd")
        ctx.save_for_backward(feat, sums)
        return pts

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        feat, sums = ctx.saved_tensors
        N, K, D, H, W = feat.shape
        g = _prep(g)
        dfeat = torch.empty_like(feat)
        check(lib.kmh_com3d_bwd(_p(g), _p(feat), _p(sums), _p(dfeat), N, K, D, H, W, _stream()), "kmh_com3d_bwd")
        return dfeat


def com3d(feat: Tensor) -> Tensor:
    """(N,K,D,H,W) -> (N,K,3) in (z,y,x) order, [-1,1]."""
    return _Com3d.apply(feat)


# --------------------------------------------------------------------------
# LC2 / ImageLC2 similarity (keymorph/loss_ops.py:250-391)
# --------------------------------------------------------------------------
class _LC2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, us, mr, patch, radii, alpha, beta, mean):
        import ctypes
        shape = us.shape
        us, mr = _prep(us, "us"), _prep(mr, "mr")
        lib = _lib.load()
        N, S = shape[0], shape[-1]
        if mr.shape != shape or us.numel() != N * S ** 3:
            raise ValueError(f"lc2: expected two (N, [1,] S, S, S) volumes, got {tuple(shape)} and {tuple(mr.shape)}")
        nP = S // patch
        B, R = N * nP ** 3, len(radii)
        rad = (ctypes.c_int * R)(*radii)
        ws = torch.empty(max(int(lib.kmh_lc2_ws_bytes(B, R)), 1), dtype=torch.uint8, device=us.device)
        out = torch.empty(() if mean else (B,), dtype=torch.float32, device=us.device)
        check(lib.kmh_lc2_fwd(_p(us), _p(mr), N, S, patch, rad, R, alpha, beta, int(mean), _p(ws), _p(out), _stream()),
              "kmh_lc2_fwd")
        ctx.save_for_backward(us, mr, ws)
        ctx.args = (N, S, patch, radii, int(mean), shape)
        return out

    @staticmethod
    def backward(ctx, gout):
        import ctypes
        lib = _lib.load()
        us, mr, ws = ctx.saved_tensors
        N, S, patch, radii, mean, shape = ctx.args
        gout = _prep(gout)
        rad = (ctypes.c_int * len(radii))(*radii)
        dus = torch.empty_like(us) if ctx.needs_input_grad[0] else None
        dmr = torch.empty_like(mr) if ctx.needs_input_grad[1] else None
        check(lib.kmh_lc2_bwd(_p(us), _p(mr), _p(gout), N, S, patch, rad, len(radii), mean, _p(ws), _p(dus), _p(dmr),
                              _stream()), "kmh_lc2_bwd")
        return (None if dus is None else dus.view(shape)), (None if dmr is None else dmr.view(shape)), \
            None, None, None, None, None


def lc2(us: Tensor, mr: Tensor, patch: int, radii: Sequence[int], alpha: float = 1e-3, beta: float = 1e-2,
        mean: bool = False) -> Tensor:
    """LC2 of two (N, [1,] S, S, S) volumes tiled into non-overlapping patch^3 patches (S // patch per axis, the remainder
    dropped): per patch the mean over `radii` of clamp((var - dist) / max(var, beta), 0, 1) on the centred (2r + 1)^3 crop ->
    (N (S // patch)^3,) float32 in (n, pz, py, px) order, or its mean over the patches if `mean`.  Differentiable in both
    volumes.  A radius whose centred crop [pad:-pad] of a patch is not 2r + 1 wide (pad <= 0, or patch - (2r + 1) odd) raises
    ValueError: the reference's reshape fails there (keymorph/loss_ops.py:283-286)."""
    patch, radii = int(patch), tuple(int(r) for r in radii)
    if us.shape != mr.shape or us.dim() not in (4, 5) or (us.dim() == 5 and us.shape[1] != 1) \
            or not us.shape[-1] == us.shape[-2] == us.shape[-3]:
        raise ValueError(f"lc2: expected two (N, [1,] S, S, S) volumes, got {tuple(us.shape)} and {tuple(mr.shape)}")
    if not radii or us.shape[-1] < patch or us.shape[0] < 1:
        raise ValueError(f"lc2: no radius, or no {patch}^3 patch in a volume of shape {tuple(us.shape)}")
    for r in radii:
        w = 2 * r + 1
        pad = (patch - w) // 2
        if pad < 1 or patch - 2 * pad != w:
            raise ValueError(f"lc2: radius {r} does not fit a patch of {patch}: the crop [{pad}:-{pad}] is not {w} voxels wide")
    return _LC2.apply(us, mr, patch, radii, float(alpha), float(beta), bool(mean))


# --------------------------------------------------------------------------
# mutual information through a Parzen-window joint histogram (csrc/mi.hip states the definition)
# --------------------------------------------------------------------------
MI_MIN_BINS, MI_MAX_BINS = 8, 64


def _need_bins(who: str, bins) -> int:
    if int(bins) != bins or not MI_MIN_BINS <= bins <= MI_MAX_BINS:
        raise ValueError(f"{who}: bins must be an integer in [{MI_MIN_BINS}, {MI_MAX_BINS}], got {bins}")
    return int(bins)


def _mi_final(ws, rng, N, V, bins, cnt=None):
    """(mi (N,), G (N, bins, bins)) from the joint table a histogram pass (kmh_mi_hist*, kmh_warp_mi_hist*) left in ws, with
    p = h / V, or p = h / cnt[n] for the count (N,) a masked pass left on the device."""
    mi = torch.empty((N,), dtype=torch.float32, device=ws.device)
    G = torch.empty((N, bins, bins), dtype=torch.float32, device=ws.device)
    if cnt is None:
        check(_lib.load().kmh_mi_final(_p(ws), _p(rng), N, V, bins, _p(mi), _p(G), _stream()), "kmh_mi_final")
    else:
        check(_lib.load().kmh_mi_final_masked(_p(ws), _p(rng), _p(cnt), N, bins, _p(mi), _p(G), _stream()), "kmh_mi_final_masked")
    return mi, G


def _mi_forward(a, b, bins, range_a, range_b, ranges=None, mask=None):
    """(mi (N,), rng (N, 4), G (N, bins, bins), cnt) of two checked (N, 1, D, H, W) tensors: the histogram pass, then the finalise.
    ranges: a checked (N, 4) device tensor as mi_ranges returns it, used instead of range_a / range_b.  mask: a checked byte mask;
    only its voxels are counted and cnt (N,) int64 is their number, which stays on the device (cnt is None without a mask).  The
    ranges are the caller's, or the whole volumes' own: the range stage of kmh_mi_hist on its own (kmh_mi_range), then the masked
    histogram with the ranges given."""
    lib = _lib.load()
    N, V = a.shape[0], a.numel() // a.shape[0]
    dev = a.device
    if mask is not None and ranges is None:
        ranges = _mi_ranges(a, b, bins, range_a, range_b)
    ws = torch.empty(max(int(lib.kmh_mi_ws_bytes(N, bins)), 1), dtype=torch.uint8, device=dev)
    rng = torch.empty((N, 4), dtype=torch.float32, device=dev) if ranges is None else ranges
    cnt = None if mask is None else torch.empty((N,), dtype=torch.int64, device=dev)
    ra, rb = range_a or (0.0, 0.0), range_b or (0.0, 0.0)
    if _lib.profiler.enabled:  # 8 B read per voxel, at most 9 B with a mask
        _lib.profiler.meta = {"bytes": (8.0 if mask is None else 9.0) * N * V}
    if mask is not None:
        check(lib.kmh_mi_hist_masked(_p(a), _p(b), _p(mask), _p(rng), N, V, bins, _p(ws), _p(cnt), _stream()),
              "kmh_mi_hist_masked")
    elif ranges is not None:
        check(lib.kmh_mi_hist_ranges(_p(a), _p(b), _p(rng), N, V, bins, _p(ws), _stream()), "kmh_mi_hist_ranges")
    else:
        check(lib.kmh_mi_hist(_p(a), _p(b), N, V, bins, int(range_a is not None), ra[0], ra[1], int(range_b is not None), rb[0],
                              rb[1], _p(ws), _p(rng), _stream()), "kmh_mi_hist")
    mi, G = _mi_final(ws, rng, N, V, bins, cnt)
    return mi, rng, G, cnt


class _MI(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, bins, range_a, range_b, ranges=None, mask=None):
        mi, rng, G, cnt = _mi_forward(a, b, bins, range_a, range_b, ranges, mask)
        ctx.save_for_backward(a, b, rng, G, mask, cnt)
        ctx.bins = bins
        return mi

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        a, b, rng, G, mask, cnt = ctx.saved_tensors
        gout = _prep(gout)
        N, V = a.shape[0], a.numel() // a.shape[0]
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if _lib.profiler.enabled:  # 8 B (9 B with a mask) read and 4 B written per voxel and gradient
            _lib.profiler.meta = {"bytes": ((8.0 if cnt is None else 9.0) + 4.0 * ((da is not None) + (db is not None))) * N * V}
        if cnt is None:
            check(lib.kmh_mi_bwd(_p(a), _p(b), _p(rng), _p(G), _p(gout), N, V, ctx.bins, _p(da), _p(db), _stream()), "kmh_mi_bwd")
        else:
            check(lib.kmh_mi_bwd_masked(_p(a), _p(b), _p(mask), _p(rng), _p(G), _p(gout), _p(cnt), N, V, ctx.bins, _p(da), _p(db),
                                        _stream()), "kmh_mi_bwd_masked")
        return da, db, None, None, None, None, None


def _need_mask(who: str, name: str, mask, like: Tensor):
    """mask: None, or a uint8 / bool tensor of like's shape on the GPU -> contiguous uint8 (a bool mask viewed, not copied), or
    ValueError."""
    if mask is None:
        return None
    if not isinstance(mask, Tensor) or not mask.is_cuda or mask.device != like.device:
        raise ValueError(f"{who}: {name} must be on the volumes' GPU")
    if mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{who}: {name} must be uint8 or bool (non-zero = counted), got {mask.dtype}")
    if mask.shape != like.shape:
        raise ValueError(f"{who}: {name} must have the volumes' shape {tuple(like.shape)}, got {tuple(mask.shape)}")
    mask = mask.detach().contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _mi_check(a, b, bins, range_a, range_b):
    for name, t in (("a", a), ("b", b)):
        _need_gpu_f32("mutual_information", name, t)
    _need_volume_pair("mutual_information", a, b)
    bins = _need_bins("mutual_information", bins)
    out = []
    for name, r in (("range_a", range_a), ("range_b", range_b)):
        if r is not None:
            if len(r) != 2 or not float(r[0]) <= float(r[1]):
                raise ValueError(f"mutual_information: {name} must be (lo, hi) with lo <= hi, got {r}")
            r = (float(r[0]), float(r[1]))
        out.append(r)
    return a.contiguous(), b.contiguous(), bins, out[0], out[1]


def mutual_information(a: Tensor, b: Tensor, bins: int = 32, range_a=None, range_b=None, ranges: Optional[Tensor] = None,
                       mask: Optional[Tensor] = None) -> Tensor:
    """Mutual information (nats) of two (N, 1, D, H, W) float32 volumes on the current GPU, per sample -> (N,), differentiable in
    both.  Parzen-window joint histogram with the cubic B-spline and Mattes' padding: per sample and image, u = (x - lo) s + 1 with
    s = (bins - 3) / (hi - lo) over the image's own minimum and maximum (no gradient through them), or over `range_x = (lo, hi)`
    (values outside are taken at the range's ends); a constant image has s = 0, MI = 0 and zero gradients.  Two calls give
    bit-identical values and gradients; a batch equals its samples run one by one.  `ranges`: instead of range_a / range_b, the
    (N, 4) device tensor mi_ranges(a0, b) returns, per sample, for a volume a0 whose range bounds a's (a = a warp of a0): the
    host never reads a range (io.register_bspline).  `mask`: (N, 1, D, H, W) uint8 or bool on the GPU, data without a gradient:
    only voxels with mask != 0 are counted -- they alone enter the joint table, p = h / M_n with M_n their number, their gradient
    is scaled by 1 / M_n and every other voxel's is 0; M_n = 0 gives MI = 0 and zero gradients.  The ranges stay the caller's or
    the WHOLE volume's minimum and maximum, not the masked part's.  The host never reads M_n."""
    if ranges is not None:
        if range_a is not None or range_b is not None:
            raise ValueError("mutual_information: give either range_a / range_b or ranges, not both")
        a, b, bins, _, _ = _mi_check(a, b, bins, None, None)
        mask = _need_mask("mutual_information", "mask", mask, a)
        _need_gpu_f32("mutual_information", "ranges", ranges)
        if tuple(ranges.shape) != (a.shape[0], 4):
            raise ValueError(f"mutual_information: ranges must be ({a.shape[0]}, 4) as mi_ranges returns them, got "
                             f"{tuple(ranges.shape)}")
        return _MI.apply(a, b, bins, None, None, ranges.detach().contiguous(), mask)
    checked = _mi_check(a, b, bins, range_a, range_b)
    return _MI.apply(*checked, None, _need_mask("mutual_information", "mask", mask, a))


def _mi_table(a: Tensor, b: Tensor, bins: int = 32, range_a=None, range_b=None, ranges=None, mask=None):
    """(MI (N,), G (N, bins, bins)) without autograd: G = ln(p / (pa pb)) where the joint probability p > 0, else 0 -- the table the
    gradient of mutual_information gathers from.  ranges, mask: as mutual_information takes them."""
    checked = _mi_check(a.detach(), b.detach(), bins, range_a, range_b)
    mi, _, G, _ = _mi_forward(*checked, None if ranges is None else ranges.detach().contiguous(),
                              _need_mask("mutual_information", "mask", mask, checked[0]))
    return mi, G


# --------------------------------------------------------------------------
# mutual information of a fixed volume and a moving volume warped by a matrix, fused (csrc/warp_mi.hip states the definition)
# --------------------------------------------------------------------------
def _warp_mi_check(moving, fixed, mat, bins, ranges, who="warp_mutual_information"):
    tensors = [("moving", moving), ("fixed", fixed)] + ([("mat", mat)] if mat is not None else []) \
        + ([("ranges", ranges)] if ranges is not None else [])
    for name, t in tensors:
        _need_gpu_f32(who, name, t)
    _need_volume_pair(who, moving, fixed, max_voxels=1 << 30, min_w=2)     # buffer loads: 32-bit byte offsets into a sample
    bins = _need_bins(who, bins)
    N = moving.shape[0]
    if mat is not None and tuple(mat.shape) != (N, 3, 4):
        raise ValueError(f"{who}: mat must be ({N}, 3, 4), got {tuple(mat.shape)}")
    if ranges is not None and tuple(ranges.shape) != (N, 4):
        raise ValueError(f"{who}: ranges must be ({N}, 4) as mi_ranges returns them, got {tuple(ranges.shape)}")
    return bins


def _mi_ranges(moving, fixed, bins, range_a=None, range_b=None):
    lib = _lib.load()
    N, V = moving.shape[0], moving.numel() // moving.shape[0]
    ws = torch.empty(16 * N, dtype=torch.uint8, device=moving.device)
    rng = torch.empty((N, 4), dtype=torch.float32, device=moving.device)
    ra, rb = range_a or (0.0, 0.0), range_b or (0.0, 0.0)
    check(lib.kmh_mi_range(_p(moving), _p(fixed), N, V, bins, int(range_a is not None), ra[0], ra[1], int(range_b is not None),
                           rb[0], rb[1], _p(ws), _p(rng), _stream()), "kmh_mi_range")
    return rng


def mi_ranges(moving: Tensor, fixed: Tensor, bins: int = 32) -> Tensor:
    """(N, 4) float32 on the device, (lo, s) of `moving` then of `fixed` per sample, s = (bins - 3) / (max - min) or 0 for a
    constant volume: what warp_mutual_information takes as `ranges`.  Trilinear sampling with border padding cannot leave a
    volume's [min, max], so one call serves every warp of the pair.  No host synchronisation."""
    bins = _warp_mi_check(moving, fixed, None, bins, None, "mi_ranges")
    return _mi_ranges(moving.detach().contiguous(), fixed.detach().contiguous(), bins)


class _WarpMI(torch.autograd.Function):
    """With a mask or `inside`, over the counted voxels (csrc/warp_mi.hip states which); their count stays on the device."""
    @staticmethod
    def forward(ctx, moving, fixed, mat, rng, bins, fixed_mask=None, moving_mask=None, inside=False):
        lib = _lib.load()
        N, _, D, H, W = moving.shape
        masked = fixed_mask is not None or moving_mask is not None or inside
        ws = torch.empty(int(lib.kmh_warp_mi_ws_bytes(N, bins, D, H, W)), dtype=torch.uint8, device=moving.device)
        cnt = torch.empty((N,), dtype=torch.int64, device=moving.device) if masked else None
        if _lib.profiler.enabled:  # the fixed volume once, the moving volume about once (8 corners, coherent); the masks' bytes
            _lib.profiler.meta = {"bytes": (10.0 if masked else 8.0) * N * D * H * W}
        if masked:
            check(lib.kmh_warp_mi_hist_masked(_p(moving), _p(fixed), _p(fixed_mask), _p(moving_mask), _p(mat), _p(rng), N, D, H, W,
                                              bins, int(inside), _p(ws), _p(cnt), _stream()), "kmh_warp_mi_hist_masked")
        else:
            check(lib.kmh_warp_mi_hist(_p(moving), _p(fixed), _p(mat), _p(rng), N, D, H, W, bins, _p(ws), _stream()),
                  "kmh_warp_mi_hist")
        mi, G = _mi_final(ws, rng, N, D * H * W, bins, cnt)
        ctx.save_for_backward(moving, fixed, mat, rng, G, cnt, fixed_mask, moving_mask)
        ctx.bins, ctx.inside = bins, int(inside)
        ctx.mark_non_differentiable(G)
        return mi, G

    @staticmethod
    def backward(ctx, gout, _gG):
        if not ctx.needs_input_grad[2]:
            return (None,) * 8
        lib = _lib.load()
        moving, fixed, mat, rng, G, cnt, fixed_mask, moving_mask = ctx.saved_tensors
        gout = _prep(gout)
        N, _, D, H, W = moving.shape
        ws = torch.empty(int(lib.kmh_warp_mi_ws_bytes(N, ctx.bins, D, H, W)), dtype=torch.uint8, device=moving.device)
        dmat = torch.empty_like(mat)
        if _lib.profiler.enabled:
            _lib.profiler.meta = {"bytes": (8.0 if cnt is None else 10.0) * N * D * H * W}
        if cnt is None:
            check(lib.kmh_warp_mi_bwd(_p(moving), _p(fixed), _p(mat), _p(rng), _p(G), _p(gout), N, D, H, W, ctx.bins, _p(ws),
                                      _p(dmat), _stream()), "kmh_warp_mi_bwd")
        else:
            check(lib.kmh_warp_mi_bwd_masked(_p(moving), _p(fixed), _p(fixed_mask), _p(moving_mask), _p(mat), _p(rng), _p(G),
                                             _p(gout), _p(cnt), N, D, H, W, ctx.bins, ctx.inside, _p(ws), _p(dmat), _stream()),
                  "kmh_warp_mi_bwd_masked")
        return (None, None, dmat) + (None,) * 5


def _warp_mi(moving, fixed, mat, bins, ranges, fixed_mask=None, moving_mask=None, inside=False):
    bins = _warp_mi_check(moving, fixed, mat, bins, ranges)
    fixed_mask = _need_mask("warp_mutual_information", "fixed_mask", fixed_mask, fixed)
    moving_mask = _need_mask("warp_mutual_information", "moving_mask", moving_mask, moving)
    moving, fixed = moving.detach().contiguous(), fixed.detach().contiguous()
    rng = _mi_ranges(moving, fixed, bins) if ranges is None else ranges.detach().contiguous()
    return _WarpMI.apply(moving, fixed, mat.contiguous(), rng, bins, fixed_mask, moving_mask, bool(inside))


def warp_mutual_information(moving: Tensor, fixed: Tensor, mat: Tensor, bins: int = 32, ranges: Optional[Tensor] = None,
                            fixed_mask: Optional[Tensor] = None, moving_mask: Optional[Tensor] = None,
                            inside: bool = False) -> Tensor:
    """Mutual information (nats) of `fixed` and `moving` warped by `mat`, per sample -> (N,), in one pass: by definition
    mutual_information(align_img(affine_grid(mat, dims), moving), fixed, range_a=range of moving, range_b=range of fixed) sample by
    sample, with the same joint table bit for bit, but neither the grid nor the warped volume is stored.  moving, fixed:
    (N, 1, D, H, W) float32 on the current GPU (data: no gradient); mat (N, 3, 4) as affine_grid takes it, differentiable;
    ranges: mi_ranges(moving, fixed, bins), computed here when None.  Two calls give bit-identical values and gradients; a batch
    equals its samples run one by one.

    fixed_mask, moving_mask: (N, 1, D, H, W) uint8 or bool on the GPU (data), inside: bool.  Voxel v of the fixed lattice, with
    sampling coordinate g(v) = affine_grid(mat)[v], is COUNTED iff fixed_mask[v] != 0, moving_mask is non-zero at the voxel the
    nearest sampler reads for g(v), and (inside=True) |g(v)_k| <= 1 on all three axes (a NaN is outside); an argument left out
    does not restrict.  The result is mutual_information(warped, fixed, ranges, mask=c) with
    c = fixed_mask & (align_img(grid, moving_mask.float(), "nearest") != 0) & (grid.abs() <= 1).all(-1), same table bit for bit.
    The number of counted voxels M_n is piecewise constant in mat and not differentiated: dmat sums over the counted voxels,
    scaled by 1 / M_n.  The ranges stay those of the whole volumes."""
    return _warp_mi(moving, fixed, mat, bins, ranges, fixed_mask, moving_mask, inside)[0]


def _warp_mi_table(moving: Tensor, fixed: Tensor, mat: Tensor, bins: int = 32, ranges: Optional[Tensor] = None,
                   fixed_mask=None, moving_mask=None, inside=False):
    """(MI (N,), G (N, bins, bins)) of warp_mutual_information without autograd: _mi_table's counterpart."""
    mi, G = _warp_mi(moving, fixed, mat.detach(), bins, ranges, fixed_mask, moving_mask, inside)
    return mi, G


# --------------------------------------------------------------------------
# local normalised cross-correlation (csrc/lncc.hip states the definition)
# --------------------------------------------------------------------------
LNCC_MIN_WINDOW, LNCC_MAX_WINDOW = 3, 15


class _LNCC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, window, eps):
        lib = _lib.load()
        N, _, D, H, W = a.shape
        ws = workspace(int(lib.kmh_lncc_ws_bytes(N, D, H, W, window)), a.device, "lncc")
        out = torch.empty((N,), dtype=torch.float32, device=a.device)
        if _lib.profiler.enabled:  # 8 B read per voxel
            _lib.profiler.meta = {"bytes": 8.0 * a.numel()}
        check(lib.kmh_lncc_fwd(_p(a), _p(b), N, D, H, W, window, eps, _p(out), _p(ws), _stream()), "kmh_lncc_fwd")
        ctx.save_for_backward(a, b)
        ctx.window, ctx.eps = window, eps
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        a, b = ctx.saved_tensors
        gout = _prep(gout)
        N, _, D, H, W = a.shape
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        ws = workspace(int(lib.kmh_lncc_ws_bytes(N, D, H, W, ctx.window)), a.device, "lncc")
        if _lib.profiler.enabled:  # per voxel: 8 B read and 20 B of fields written, 20 + 8 B read and 4 B written per gradient
            _lib.profiler.meta = {"bytes": (56.0 + 4.0 * ((da is not None) + (db is not None))) * a.numel()}
        check(lib.kmh_lncc_bwd(_p(a), _p(b), _p(gout), N, D, H, W, ctx.window, ctx.eps, _p(da), _p(db), _p(ws), _stream()),
              "kmh_lncc_bwd")
        return da, db, None, None


def local_ncc(a: Tensor, b: Tensor, window: int = 9, eps: float = 1e-5) -> Tensor:
    """Local normalised cross-correlation of two (N, 1, D, H, W) float32 volumes on the current GPU, per sample -> (N,) in [0, 1]
    (higher is better), differentiable in both: the mean over the voxels of cross^2 / (va vb + eps) with cross, va, vb the
    covariance and the variances (times the count) over the in-bounds part of the window^3 cube around the voxel -- windows are
    truncated at the border, so the value does not change when a constant is added to a volume.  window odd in [3, 15]; eps is
    meant for volumes scaled to about [0, 1].  Two calls give bit-identical values and gradients; a batch equals its samples run
    one by one."""
    for name, t in (("a", a), ("b", b)):
        _need_gpu_f32("local_ncc", name, t)
    _need_volume_pair("local_ncc", a, b, max_voxels=1 << 31)
    if int(window) != window or not LNCC_MIN_WINDOW <= window <= LNCC_MAX_WINDOW or window % 2 == 0:
        raise ValueError(f"local_ncc: window must be an odd integer in [{LNCC_MIN_WINDOW}, {LNCC_MAX_WINDOW}], got {window}")
    if not float(eps) >= 0.0:
        raise ValueError(f"local_ncc: eps must be >= 0, got {eps}")
    return _LNCC.apply(a.contiguous(), b.contiguous(), int(window), float(eps))


# --------------------------------------------------------------------------
# MIND-SSC, the self-similarity context descriptor as a similarity (csrc/mind.hip states the definition)
# --------------------------------------------------------------------------
MIND_MAX_RADIUS, MIND_MAX_DILATION = 3, 3


class _MIND(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, bounds, radius, dilation):
        lib = _lib.load()
        N, _, D, H, W = a.shape
        ws = workspace(int(lib.kmh_mind_ws_bytes(N, D, H, W, radius, dilation)), a.device, "mind")
        out = torch.empty((N,), dtype=torch.float32, device=a.device)
        if _lib.profiler.enabled:  # 8 B read per voxel; the halos come from the caches
            _lib.profiler.meta = {"bytes": 8.0 * a.numel()}
        check(lib.kmh_mind_fwd(_p(a), _p(b), _p(bounds), N, D, H, W, radius, dilation, _p(out), _p(ws), _stream()), "kmh_mind_fwd")
        ctx.save_for_backward(a, b, bounds)
        ctx.radius, ctx.dilation = radius, dilation
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        a, b, bounds = ctx.saved_tensors
        gout = _prep(gout)
        N, _, D, H, W = a.shape
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        ws = workspace(int(lib.kmh_mind_ws_bytes(N, D, H, W, ctx.radius, ctx.dilation)), a.device, "mind")
        if _lib.profiler.enabled:  # per voxel and gradient: 8 B read, 48 B written and read, 24 B written and read, 4 B written
            _lib.profiler.meta = {"bytes": 156.0 * ((da is not None) + (db is not None)) * a.numel()}
        check(lib.kmh_mind_bwd(_p(a), _p(b), _p(bounds), _p(gout), N, D, H, W, ctx.radius, ctx.dilation, _p(da), _p(db), _p(ws),
                               _stream()), "kmh_mind_bwd")
        return da, db, None, None, None


def _mind_check(who, a, b, radius, dilation):
    for name, t in (("a", a), ("b", b)):
        _need_gpu_f32(who, name, t)
    _need_volume_pair(who, a, b, max_voxels=1 << 31)
    for name, v, top in (("radius", radius, MIND_MAX_RADIUS), ("dilation", dilation, MIND_MAX_DILATION)):
        if isinstance(v, bool) or int(v) != v or not 1 <= v <= top:
            raise ValueError(f"{who}: {name} must be an integer in [1, {top}], got {v!r}")
    return int(radius), int(dilation)


def mind_bounds(a: Tensor, b: Tensor, radius: int = 1, dilation: int = 2) -> Tensor:
    """(N, 2, 2) float32 on the device, [a or b][lo or hi]: 1e-3 and 1e3 times each sample's mean over the voxels of the
    descriptor's unclamped variance estimate mean_c m_c -- what mind_ssc_loss takes as `bounds`.  A driver computes them once per
    pair and keeps them while one volume is warped, as it does with mi_ranges.  No host synchronisation."""
    radius, dilation = _mind_check("mind_bounds", a, b, radius, dilation)
    lib = _lib.load()
    a, b = a.detach().contiguous(), b.detach().contiguous()
    N, _, D, H, W = a.shape
    ws = workspace(int(lib.kmh_mind_ws_bytes(N, D, H, W, radius, dilation)), a.device, "mind")
    bounds = torch.empty((N, 2, 2), dtype=torch.float32, device=a.device)
    check(lib.kmh_mind_bounds(_p(a), _p(b), N, D, H, W, radius, dilation, _p(bounds), _p(ws), _stream()), "kmh_mind_bounds")
    return bounds


def mind_ssc_loss(a: Tensor, b: Tensor, radius: int = 1, dilation: int = 2, bounds: Optional[Tensor] = None) -> Tensor:
    """MIND-SSC distance (Heinrich et al. 2013) of two (N, 1, D, H, W) float32 volumes on the current GPU, per sample -> (N,),
    >= 0, LOWER is better, differentiable in both: the mean over the voxels and the 12 channels of the squared difference of
    the two self-similarity context descriptors (box means over (2 radius + 1)^3 of squared differences between the six
    neighbours at distance `dilation`, minus their minimum, over their clamped mean, through exp(-.)).  A local metric for two
    modalities: the descriptor does not change under a -> s a + t.  radius, dilation in 1..3.  bounds (N, 2, 2): the clamp of the
    variance estimate, constants of the call as mutual information's ranges are; None: mind_bounds(a, b, radius, dilation) of
    these very inputs.  Two calls give bit-identical values and gradients; a batch equals its samples run one by one."""
    radius, dilation = _mind_check("mind_ssc_loss", a, b, radius, dilation)
    if bounds is None:
        bounds = mind_bounds(a, b, radius, dilation)
    else:
        _need_gpu_f32("mind_ssc_loss", "bounds", bounds)
        if tuple(bounds.shape) != (a.shape[0], 2, 2):
            raise ValueError(f"mind_ssc_loss: bounds must be ({a.shape[0]}, 2, 2) as mind_bounds returns them, got "
                             f"{tuple(bounds.shape)}")
    return _MIND.apply(a.contiguous(), b.contiguous(), bounds.detach().contiguous(), radius, dilation)


# --------------------------------------------------------------------------
# trilinear resize (F.interpolate(mode="trilinear", align_corners=False); keymorph/model.py:576-588)
# --------------------------------------------------------------------------
def resize_out_size(n_in: int, scale_factor: float) -> int:
    import math
    return int(math.floor(n_in * float(scale_factor)))


def resize_axis_scale(n_in: int, n_out: int, scale_factor=None):
    """The fp32 coordinate scale of one axis: the fp32 quotient in / out when a size was given, fp32(1 / scale_factor) when a
    factor was."""
    import numpy as np
    if scale_factor is None:
        return np.float32(n_in) / np.float32(n_out)
    return np.float32(1.0 / float(scale_factor))


def resize_axis_table(n_in: int, n_out: int, s):
    """THE per-axis definition shared by the kernel, the tests and the fp64 restatement.  For output index o:
    src = max(s * (o + 0.5) - 0.5, 0) in fp32 with separately rounded multiply and subtract, i0 = min(floor(src), in - 1),
    i1 = min(i0 + 1, in - 1), lam = src - i0.  Returns numpy (i0, i1, lam, lo, hi): lo[i] .. hi[i] is the range of outputs that
    reference input i (lo > hi: none); a set of referencing outputs that is not one contiguous range raises."""
    import numpy as np
    s = np.float32(s)
    o = np.arange(n_out, dtype=np.float32)
    src = np.maximum(s * (o + np.float32(0.5)) - np.float32(0.5), np.float32(0.0)).astype(np.float32)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = (src - i0.astype(np.float32)).astype(np.float32)
    lo = np.ones(n_in, dtype=np.int64)
    hi = np.zeros(n_in, dtype=np.int64)
    for i in range(n_in):
        ref = np.nonzero((i0 == i) | (i1 == i))[0]
        if len(ref):
            lo[i], hi[i] = ref[0], ref[-1]
            if hi[i] - lo[i] + 1 != len(ref):
                raise ValueError(f"resize {n_in} -> {n_out}: the outputs that read input {i} are not one contiguous range")
    return i0.astype(np.int32), i1.astype(np.int32), lam, lo.astype(np.int32), hi.astype(np.int32)


_RESIZE_TABS = {}


def _resize_tables(n_in: int, n_out: int, s, device):
    """device int32 tensors (forward table 3 * out, range table 2 * in) of one axis, built once per (in, out, s, device)"""
    import numpy as np
    key = (n_in, n_out, np.float32(s).tobytes(), str(device))
    t = _RESIZE_TABS.get(key)
    if t is None:
        i0, i1, lam, lo, hi = resize_axis_table(n_in, n_out, s)
        fwd = torch.from_numpy(np.concatenate([i0, i1, lam.view(np.int32)])).to(device)
        rng = torch.from_numpy(np.concatenate([lo, hi])).to(device)
        t = _RESIZE_TABS[key] = (fwd, rng)
    return t


class _ResizeTrilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, out_size, scales, channels_last):
        lib = _lib.load()
        x = _prep(x, "x")
        if channels_last:
            N, D, H, W, C = x.shape
        else:
            N, C, D, H, W = x.shape
        Do, Ho, Wo = out_size
        tabs = [_resize_tables(i, o, s, x.device) for i, o, s in zip((D, H, W), out_size, scales)]
        y = torch.empty((N, Do, Ho, Wo, C) if channels_last else (N, C, Do, Ho, Wo), dtype=torch.float32, device=x.device)
        if _lib.profiler.enabled:
            _lib.profiler.meta = {"bytes": 4.0 * (x.numel() + y.numel())}
        check(lib.kmh_resize_trilinear3d_fwd(_p(x), _p(y), N, C, D, H, W, Do, Ho, Wo, _p(tabs[0][0]), _p(tabs[1][0]),
                                             _p(tabs[2][0]), int(channels_last), _stream()), "kmh_resize_trilinear3d_fwd")
        ctx.tabs, ctx.dims, ctx.cl = tabs, (N, C, D, H, W, Do, Ho, Wo), bool(channels_last)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        gy = _prep(gy)
        N, C, D, H, W, Do, Ho, Wo = ctx.dims
        tz, ty, tx = ctx.tabs
        gx = torch.empty((N, D, H, W, C) if ctx.cl else (N, C, D, H, W), dtype=torch.float32, device=gy.device)
        check(lib.kmh_resize_trilinear3d_bwd(_p(gy), _p(gx), N, C, D, H, W, Do, Ho, Wo, _p(tz[0]), _p(ty[0]), _p(tx[0]),
                                             _p(tz[1]), _p(ty[1]), _p(tx[1]), int(ctx.cl), _stream()),
              "kmh_resize_trilinear3d_bwd")
        return gx, None, None, None


def resize_trilinear3d(x: Tensor, size=None, scale_factor=None, channels_last: bool = False) -> Tensor:
    """x (N,C,D,H,W), or (N,D,H,W,C) with channels_last, resized like F.interpolate(mode="trilinear", align_corners=False);
    exactly one of `size` (3 ints) and `scale_factor` (a number or 3 numbers).  Differentiable; the gradient is bitwise
    repeatable.  The two layouts give bit-identical values."""
    if (size is None) == (scale_factor is None):
        raise ValueError("resize_trilinear3d: give exactly one of size and scale_factor")
    if x.dim() != 5:
        raise ValueError(f"resize_trilinear3d: expected a 5-D tensor, got {tuple(x.shape)}")
    dims = tuple(x.shape[1:4]) if channels_last else tuple(x.shape[2:5])
    if size is not None:
        out = tuple(int(v) for v in size)
        factors = (None,) * 3
    else:
        factors = tuple(float(v) for v in scale_factor) if isinstance(scale_factor, (tuple, list)) else (float(scale_factor),) * 3
        if len(factors) != 3:
            raise ValueError("resize_trilinear3d: scale_factor needs one or three numbers")
        out = tuple(resize_out_size(i, f) for i, f in zip(dims, factors))
    if len(out) != 3 or min(out) < 1:
        raise ValueError(f"resize_trilinear3d: bad output size {out}")
    scales = tuple(resize_axis_scale(i, o, f) for i, o, f in zip(dims, out, factors))
    return _ResizeTrilinear.apply(x, out, scales, bool(channels_last))


# --------------------------------------------------------------------------
# connected components / clean_mask (keymorph/model.py:622-659)
# --------------------------------------------------------------------------
def _mask_bytes(mask: Tensor, name: str) -> Tensor:
    _need_gpu(None, name, mask)
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.to(torch.uint8)
    elif mask.dtype != torch.uint8:
        raise ValueError(f"{name}: expected a bool or uint8 mask, got {mask.dtype}")
    return mask.contiguous()


def connected_components3d(mask: Tensor) -> Tensor:
    """(D,H,W) bool / uint8 mask on the GPU -> int32 labels under full 26-neighbour connectivity: 1 + the raster-order linear
    index of the component's first voxel, 0 = background.  The numbering is canonical: the same on every run."""
    if mask.dim() != 3:
        raise ValueError(f"connected_components3d: expected a (D, H, W) mask, got {tuple(mask.shape)}")
    lib = _lib.load()
    m = _mask_bytes(mask, "mask")
    D, H, W = m.shape
    labels = torch.empty((D, H, W), dtype=torch.int32, device=m.device)
    if m.numel() == 0:
        return labels
    ws = workspace(int(lib.kmh_components3d_ws_bytes(1, D, H, W)), m.device, "components")
    check(lib.kmh_components3d(_p(m), _p(labels), 1, D, H, W, None, _p(ws), _stream()), "kmh_components3d")
    return labels


def clean_mask3d(mask: Tensor, threshold: float):
    """(N,D,H,W) bool / uint8 masks on the GPU -> (uint8 masks that keep the components with size / largest size > threshold,
    info): info is an int32 device tensor of N + 1 entries, the largest component size per sample and then a flag that is 1
    when some mask value was neither 0 nor 1."""
    if mask.dim() != 4:
        raise ValueError(f"clean_mask3d: expected (N, D, H, W) masks, got {tuple(mask.shape)}")
    lib = _lib.load()
    m = _mask_bytes(mask, "mask")
    N, D, H, W = m.shape
    out = torch.empty_like(m)
    info = torch.zeros(N + 1, dtype=torch.int32, device=m.device)
    if m.numel() == 0:
        return out, info
    ws = workspace(int(lib.kmh_components3d_ws_bytes(N, D, H, W)), m.device, "components")
    check(lib.kmh_clean_mask3d(_p(m), _p(out), N, D, H, W, float(threshold), _p(info), _p(ws), _stream()), "kmh_clean_mask3d")
    return out, info
