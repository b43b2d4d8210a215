"""GPU: the one-product (use_amp) arithmetic of the 27-tap kernels against its definition.

Under `amp_scope(True)` the split-operand kernels scale every operand tensor by its power-of-two range scale S, split it into
fp16 hi + lo exactly as for f16x3, and multiply only hi x hi (fp32 accumulation).  Through the operators that take raw operands
(no GroupNorm in front) S is an exact power of two read back from the device, so the definition can be restated exactly: each
operand v becomes fp16(v * S) / S, and the result is the plain fp64 convolution / correlation of those.  What is left is the
kernels' fp32 accumulation, i.e. the 3e-6 bar tests/test_backbone_gpu.py::test_conv_arithmetic_modes_vs_fp64 applies to f16x3.
Subjects: the 32- and 64-wide one-wave forward tiles (forward and data gradient) and the wave-specialised weight gradient, on a
volume that is ragged in every axis.  (The z-paired tile and the small-launch kernel have no one-product instance.)"""
import numpy as np
import pytest
import torch

from tests.test_conv_dispatch_gpu import conv3_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, DIMS = 2, (9, 13, 40)


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())


def hi_term(v, scale2):
    """fp64 value of the only term the one-product arithmetic keeps of v: fp16(v * S) / S, with {S, 1/S} from the device"""
    S, inv = float(scale2[0]), float(scale2[1])
    assert S * inv == 1.0 and float(np.log2(S)).is_integer()
    return (v.detach().cpu().float() * S).half().double() / S


def wgrad_fp64(x, dz):
    """dw[co, ci, kz, ky, kx] = sum_{n, v} x[n, v + tap - 1, ci] dz[n, v, co], zero padding; x, dz (N, D, H, W, C) fp64"""
    n, D, H, W, Cin = x.shape
    Cout = dz.shape[-1]
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))
    dw = torch.empty(Cout, Cin, 3, 3, 3, dtype=torch.float64)
    d2 = dz.reshape(-1, Cout).t()
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                dw[:, :, kz, ky, kx] = d2 @ xp[:, kz:kz + D, ky:ky + H, kx:kx + W, :].reshape(-1, Cin)
    return dw


@pytest.mark.parametrize("Cin,Cout,tile", [(32, 32, 1), (64, 64, 2)])
def test_one_product_arithmetic_is_the_hi_terms_convolution(Cin, Cout, tile):
    from keymorph_amd import _lib, backbone_ops as B
    lib = _lib.load()
    D, H, W = DIMS
    old_mode = B.CONV_MODE
    old_dispatch = lib.kmh_conv3d_fwd_bf_set_dispatch(2)
    try:
        B.set_conv_mode("f16x3")
        assert lib.kmh_conv3d_fwd_bf_variant(N, D, H, W, Cin, Cout, 2, 0, 0) == tile
        assert lib.kmh_conv3d_fwd_bf_variant(N, D, H, W, Cout, Cin, 2, 0, 0) == tile
        assert lib.kmh_conv3d_wgrad_bf_blocked_ok(N, D, H, W, Cin, Cout, 2) == 1        # the wave-specialised weight gradient
        g = torch.Generator().manual_seed(700 + Cin)
        x = (torch.randn(N, D, H, W, Cin, generator=g) + 0.3).to(DEV)
        w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) / np.sqrt(27 * Cin)).to(DEV)
        bias = (0.3 * torch.randn(Cout, generator=g)).to(DEV)
        dz = (torch.randn(N, D, H, W, Cout, generator=g) * 3e-3).to(DEV)
        xs, ds = B.absmax_scale(x), B.absmax_scale(dz)
        pk, pkt = B.pack_weight(w, False), B.pack_weight(w, True)

        def run():
            y = B.conv3_raw(x, None, None, pk, bias, N, D, H, W, Cin, Cout, False, True, ascale=xs)
            dx = B.conv3_raw(dz, None, None, pkt, None, N, D, H, W, Cout, Cin, False, False, ascale=ds)
            dw = B.conv3_wgrad(x, None, None, dz, N, D, H, W, Cin, Cout, False, dzmask=None, xscale=xs, dscale=ds)
            torch.cuda.synchronize()
            return {"forward": y, "data gradient": dx, "weight gradient": dw}

        with B.amp_scope(True):
            one = run()
        with B.amp_scope(False):
            three = run()

        xq, dq = hi_term(x, xs), hi_term(dz, ds)
        wq, wtq = hi_term(w, B._packed(pk)[1]), hi_term(w, B._packed(pkt)[1])
        want = {"forward": torch.relu(conv3_fp64(xq, wq) + bias.cpu().double()),
                "data gradient": conv3_fp64(dq, wtq.flip(2, 3, 4).permute(1, 0, 2, 3, 4).contiguous()),
                "weight gradient": wgrad_fp64(xq, dq)}
        for k in want:
            err, moved = rel_l2(one[k], want[k]), rel_l2(one[k], three[k])
            print(f"\n{Cin}->{Cout} {k}: one product vs its fp64 definition {err:.3e}, vs f16x3 {moved:.3e}")
            assert err < 3e-6, (k, err)
            assert moved > 1e-5, (k, moved)          # eleven-bit operands: about 3e-4; the flag reached the kernel
    finally:
        lib.kmh_conv3d_fwd_bf_set_dispatch(old_dispatch)
        B.set_conv_mode(old_mode)
