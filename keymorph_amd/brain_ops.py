"""Operators of the brain extractor (keymorph/model.py:533-616, notebooks/[B] Brain Extraction.ipynb), NDHWC like backbone_ops.

    conv_layer : Conv3d(k3,p1,bias) [-> InstanceNorm(affine=False)] [-> ReLU] with every launch ROUTED: the split-operand matrix
                 kernels of backbone_ops where they are built for the channel counts, the direct fp32 kernels of
                 csrc/conv_thin.hip otherwise (thin layers: 1, 4 or 8 channels on one side)
    upsample2  : the x2 trilinear upsampling of csrc/resize.hip on NDHWC tensors

Routing (DESIGN.md section 8a has the table).  A 3x3x3 launch Cin -> Cout goes to the split-operand kernels iff
Cin % 8 == 0 and Cout % 4 == 0: whole 8-channel input chunks and a 4-channel-aligned output, what their vector paths are
written for and what the backbones' own layers exercise.  Everything else must be served by the thin family or it is an error
(no eager fallback).  A layer's forward, data gradient (the transposed pair Cout -> Cin) and weight gradient are routed one by one.
"""
from __future__ import annotations

import torch

from . import _lib
from . import backbone_ops as B
from ._lib import check
from .ops import _p, _prep, _stream, workspace, resize_trilinear3d

Tensor = torch.Tensor


def matrix_route(cin: int, cout: int) -> bool:
    """True: the launch cin -> cout runs on the split-operand kernels; False: on the thin fp32 family."""
    return cin % 8 == 0 and cout % 4 == 0


def routes(cin: int, cout: int) -> dict:
    """'matrix' / 'thin' for the three launches of a layer cin -> cout."""
    name = lambda m: "matrix" if m else "thin"      # noqa: E731
    return {"fwd": name(matrix_route(cin, cout)), "dgrad": name(matrix_route(cout, cin)), "wgrad": name(matrix_route(cin, cout))}


def _need_thin(ok: int, what: str, cin: int, cout: int):
    if not ok:
        raise _lib.KeymorphHipError(f"no kernel serves the {what} of a 3x3x3 convolution {cin} -> {cout}: neither the "
                                    "split-operand family (Cin % 8 == 0, Cout % 4 == 0) nor the thin fp32 family")


def conv_fwd(x: Tensor, weight: Tensor, bias, relu: bool) -> Tensor:
    """y = conv(x) + bias [ReLU], x (N,D,H,W,Cin) -> (N,D,H,W,Cout)"""
    lib = _lib.load()
    N, D, H, W, Cin = x.shape
    Cout = weight.shape[0]
    if matrix_route(Cin, Cout):
        return B.conv3_raw(x, None, None, B.pack_weight(weight, False), bias, N, D, H, W, Cin, Cout, False, relu)
    _need_thin(lib.kmh_conv3d_thin_ok(Cin, Cout), "forward", Cin, Cout)
    y = torch.empty((N, D, H, W, Cout), dtype=torch.float32, device=x.device)
    check(lib.kmh_conv3d_thin_fwd(_p(x), _p(weight), _p(bias), _p(y), N, D, H, W, Cin, Cout, int(relu), _stream()),
          "kmh_conv3d_thin_fwd")
    return y


def conv_dgrad(dz: Tensor, dzmask, weight: Tensor) -> Tensor:
    """dx (N,D,H,W,Cin) of the layer `weight` (Cout,Cin,3,3,3); dzmask: the layer's ReLU output | None"""
    lib = _lib.load()
    N, D, H, W, Cout = dz.shape
    Cin = weight.shape[1]
    if matrix_route(Cout, Cin):
        return B.conv3_raw(dz, None, None, B.pack_weight(weight, True), None, N, D, H, W, Cout, Cin, False, False, mask=dzmask)
    _need_thin(lib.kmh_conv3d_thin_ok(Cout, Cin), "data gradient", Cin, Cout)
    dx = torch.empty((N, D, H, W, Cin), dtype=torch.float32, device=dz.device)
    check(lib.kmh_conv3d_thin_dgrad(_p(dz), _p(dzmask), _p(weight), _p(dx), N, D, H, W, Cin, Cout, _stream()),
          "kmh_conv3d_thin_dgrad")
    return dx


def conv_wgrad(x: Tensor, dz: Tensor, dzmask, Cout: int):
    """(dw (Cout,Cin,3,3,3), db (Cout)) of the layer for its input x and output gradient dz [masked by dzmask]"""
    lib = _lib.load()
    N, D, H, W, Cin = x.shape
    if matrix_route(Cin, Cout):
        dw = B.conv3_wgrad(x, None, None, dz, N, D, H, W, Cin, Cout, False, dzmask=dzmask)
        dzm = dz
        if dzmask is not None:
            dzm = torch.empty_like(dz)
            check(lib.kmh_relu_mask(_p(dz), _p(dzmask), dz.numel(), _p(dzm), _stream()), "kmh_relu_mask")
        db = B.channel_stats(dzm, None, N, D * H * W, Cout)[:, :, 0].sum(0).float()
        return dw, db
    _need_thin(lib.kmh_conv3d_thin_wgrad_ok(Cin, Cout), "weight gradient", Cin, Cout)
    dw = torch.empty((Cout, Cin, 3, 3, 3), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device)
    ws = workspace(int(lib.kmh_conv3d_thin_wgrad_ws_bytes(N, D, H, W, Cin, Cout)), x.device, "wgrad")
    check(lib.kmh_conv3d_thin_wgrad(_p(x), _p(dz), _p(dzmask), _p(dw), _p(db), N, D, H, W, Cin, Cout, _p(ws), _stream()),
          "kmh_conv3d_thin_wgrad")
    return dw, db


class _ConvBias(torch.autograd.Function):
    """Conv3d(k3,p1,bias) [-> ReLU], every launch routed.  relu=False is the network's final convolution."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        x, weight, bias = _prep(x, "x"), _prep(weight, "weight"), _prep(bias, "bias")
        y = conv_fwd(x, weight, bias, relu)
        ctx.relu = bool(relu)
        ctx.save_for_backward(x, weight, *([y] if relu else []))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, *rest = ctx.saved_tensors
        dz = _prep(dy)
        dzmask = rest[0] if ctx.relu else None
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = conv_wgrad(x, dz, dzmask, weight.shape[0])
        if ctx.needs_input_grad[0]:
            dx = conv_dgrad(dz, dzmask, weight)
        return dx, dw, db, None


class _InstanceNormRelu(torch.autograd.Function):
    """InstanceNorm3d(affine=False) -> ReLU on an NDHWC tensor of any channel count, from the norm kernels _ConvBlock uses."""

    @staticmethod
    def forward(ctx, z):
        lib = _lib.load()
        z = _prep(z)
        N, D, H, W, C = z.shape
        V = D * H * W
        scale, shift, mr = B.norm_coeffs(B.channel_stats(z, None, N, V, C), None, None, N, C, C, V)
        y = torch.empty_like(z)
        check(lib.kmh_norm_apply(_p(z), _p(scale), _p(shift), N, V, C, 1, _p(y), _stream()), "kmh_norm_apply")
        ctx.save_for_backward(z, y, mr)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        z, y, mr = ctx.saved_tensors
        N, D, H, W, C = z.shape
        V = D * H * W
        dy = _prep(dy)
        dym = torch.empty_like(dy)
        check(lib.kmh_relu_mask(_p(dy), _p(y), dy.numel(), _p(dym), _stream()), "kmh_relu_mask")
        c123, _, _ = B._gn_bwd_coeffs(B.channel_stats(dym, z, N, V, C), None, mr, N, C, C, V)
        return B._gn_bwd_apply(dym, z, c123, N, V, C, None, from_relu=False)


def all_matrix(cin: int, cout: int) -> bool:
    return matrix_route(cin, cout) and matrix_route(cout, cin)


def conv_layer(x: Tensor, weight: Tensor, bias: Tensor, use_in: bool = False, relu: bool = True) -> Tensor:
    """One block of Simple_Unet (keymorph/model.py:598-616): Conv3d(k3,p1,bias) -> [InstanceNorm] -> ReLU; relu=False (and no
    norm) is the final convolution.  A layer whose three launches all take the split-operand kernels is the ConvNet's block."""
    cout, cin = weight.shape[:2]
    if relu and all_matrix(cin, cout):
        return B.conv_block(x, weight, bias, None, None, cout if use_in else 0)
    if use_in:
        assert relu, "the reference has no InstanceNorm without the ReLU"
        return _InstanceNormRelu.apply(_ConvBias.apply(x, weight, bias, False))
    return _ConvBias.apply(x, weight, bias, relu)


def upsample2(x: Tensor) -> Tensor:
    """F.interpolate(scale_factor=2, mode="trilinear", align_corners=False) on (N,D,H,W,C)"""
    return resize_trilinear3d(x, scale_factor=2, channels_last=True)
