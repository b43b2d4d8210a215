"""GPU: backbone operators and whole (Truncated)UNet3D forward/backward vs the oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import keymorph_oracle as O
from tests.util import T, golden, seeded_state_dict, unet_shapes

pytestmark = pytest.mark.gpu
DEV = "cuda"


def close(a, b, atol=1e-5, rtol=1e-5):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a, b, atol=atol, rtol=rtol)


def gen(s):
    return torch.Generator().manual_seed(s)


def ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


@pytest.mark.parametrize("cfg", [
    dict(N=1, Cin=16, Cout=32, D=6, H=10, W=40),     # multi-tile in x, ragged
    dict(N=2, Cin=8, Cout=8, D=5, H=7, W=9),         # tiny channels (1 ch per group)
    dict(N=1, Cin=1, Cout=4, D=8, H=8, W=8),         # first layer: Cin = 1, GN with 1 group
    dict(N=1, Cin=48, Cout=64, D=4, H=9, W=33),      # decoder-like, NT = 2
    dict(N=1, Cin=96, Cout=96, D=3, H=4, W=5),       # 64 < Cout <= 96: the 96-wide N tile, both directions
    dict(N=2, Cin=32, Cout=96, D=5, H=11, W=37),     # the same on ragged multi-brick volumes
    dict(N=1, Cin=16, Cout=160, D=4, H=5, W=9),      # Cout > 96: 64-wide channel groups, the last one partly empty
    dict(N=1, Cin=12, Cout=20, D=4, H=4, W=6),       # odd sizes, Cin % 8 != 0
])
def test_single_conv_gcr(cfg):
    from keymorph_amd import backbone_ops as B
    g = gen(1)
    N, Cin, Cout, D, H, W = (cfg[k] for k in ("N", "Cin", "Cout", "D", "H", "W"))
    G = 1 if Cin < 8 else 8
    if Cin % G:
        G = 4
    x = torch.randn(N, Cin, D, H, W, generator=g).abs() + 0.1 * torch.randn(N, Cin, D, H, W, generator=g)
    gamma = 1 + 0.2 * torch.randn(Cin, generator=g)
    beta = 0.2 * torch.randn(Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / np.sqrt(27 * Cin)
    cot = torch.randn(N, Cout, D, H, W, generator=g)
    xr, gr, br, wr = (t.clone().requires_grad_(True) for t in (x, gamma, beta, w))
    yr = F.relu(F.conv3d(F.group_norm(xr, G, gr, br, 1e-5), wr, None, padding=1))
    (yr * cot).sum().backward()
    xh = ndhwc(x).to(DEV).requires_grad_(True)
    gh, bh, wh = (t.to(DEV).requires_grad_(True) for t in (gamma, beta, w))
    yh = B.single_conv_gcr(xh, gh, bh, wh, G, x_from_relu=False)
    (yh * ndhwc(cot).to(DEV)).sum().backward()
    close(ncdhw(yh), yr, 2e-5, 1e-4)
    s = float(wr.grad.abs().max())
    close(wh.grad, wr.grad, 2e-4 * s, 1e-3)
    close(ncdhw(xh.grad), xr.grad, 2e-4 * float(xr.grad.abs().max()), 1e-3)
    close(gh.grad, gr.grad, 2e-4 * float(gr.grad.abs().max()), 1e-3)
    close(bh.grad, br.grad, 2e-4 * float(br.grad.abs().max()), 1e-3)


def test_maxpool_upcat_pointwise():
    from keymorph_amd import backbone_ops as B
    g = gen(2)
    x = torch.randn(2, 6, 8, 6, 10, generator=g)
    cot = torch.randn(2, 6, 4, 3, 5, generator=g)
    xr = x.clone().requires_grad_(True)
    (F.max_pool3d(xr, 2) * cot).sum().backward()
    xh = ndhwc(x).to(DEV).requires_grad_(True)
    yh = B.maxpool2(xh)
    (yh * ndhwc(cot).to(DEV)).sum().backward()
    close(ncdhw(yh), F.max_pool3d(x, 2), 0)
    close(ncdhw(xh.grad), xr.grad, 0)
    # odd sizes
    x = torch.randn(1, 3, 7, 5, 9, generator=g)
    close(ncdhw(B.maxpool2(ndhwc(x).to(DEV))), F.max_pool3d(x, 2), 0)
    # upsample + concat (exact 2x and ragged)
    # channel counts 5 + 7: scalar kernels; 8 + 12: the 16-byte kernels (incl. the exact-2x gradient fast path)
    for (ds, dl, cs, cl) in (((8, 6, 10), (4, 3, 5), 5, 7), ((7, 5, 9), (3, 2, 4), 5, 7), ((8, 6, 10), (4, 3, 5), 8, 12),
                             ((7, 5, 9), (3, 2, 4), 8, 12), ((12, 4, 6), (6, 2, 3), 4, 4)):
        skip = torch.randn(2, cs, *ds, generator=g)
        low = torch.randn(2, cl, *dl, generator=g)
        cot = torch.randn(2, cs + cl, *ds, generator=g)
        sr, lr = skip.clone().requires_grad_(True), low.clone().requires_grad_(True)
        ref = torch.cat([sr, F.interpolate(lr, size=ds, mode="nearest")], 1)
        (ref * cot).sum().backward()
        sh, lh = ndhwc(skip).to(DEV).requires_grad_(True), ndhwc(low).to(DEV).requires_grad_(True)
        out = B.upcat(sh, lh)
        (out * ndhwc(cot).to(DEV)).sum().backward()
        close(ncdhw(out), ref, 0)
        close(ncdhw(sh.grad), sr.grad, 0)
        close(ncdhw(lh.grad), lr.grad, 1e-6)
    # pointwise (final conv)
    for (Cin, Cout, dims) in ((16, 16, (4, 5, 6)), (64, 200, (3, 8, 11)), (8, 40, (2, 3, 70))):
        x = torch.randn(2, Cin, *dims, generator=g)
        w = torch.randn(Cout, Cin, 1, 1, 1, generator=g) / np.sqrt(Cin)
        b = torch.randn(Cout, generator=g)
        cot = torch.randn(2, Cout, *dims, generator=g)
        xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
        ref = F.conv3d(xr, wr, br)
        (ref * cot).sum().backward()
        xh = ndhwc(x).to(DEV).requires_grad_(True)
        wh, bh = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        out = B.pointwise(xh, wh, bh)
        (out * cot.to(DEV)).sum().backward()
        close(out, ref, 2e-5, 1e-5)
        close(ncdhw(xh.grad), xr.grad, 1e-4, 1e-4)
        close(wh.grad, wr.grad, 1e-3, 1e-4)
        close(bh.grad, br.grad, 1e-3, 1e-4)
    # layout round trip
    x = torch.randn(2, 5, 3, 4, 7, generator=g).to(DEV)
    close(B.to_ncdhw(B.to_ndhwc(x)), x, 0)
    close(B.to_ndhwc(x), x.permute(0, 2, 3, 4, 1), 0)


@pytest.mark.parametrize("cfg", [(2, 1, 16, (9, 10, 37)), (1, 16, 32, (6, 9, 40)), (2, 8, 72, (5, 12, 33)),
                                 (1, 24, 8, (8, 8, 8))])
@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_conv_epilogue_statistics(cfg, mode):
    """the (sum y, sum y^2) pairs the conv epilogue emits for the next GroupNorm == a separate pass over y, for the
    z-paired (Cout <= 16), one- and two-tile variants and ragged bricks; and upsample+concat derives its statistics
    from those of its sources."""
    from keymorph_amd import backbone_ops as B
    N, Cin, Cout, dims = cfg
    old = B.CONV_MODE
    try:
        B.set_conv_mode(mode)
        g = gen(31)
        x = torch.randn(N, *dims, Cin, generator=g).to(DEV)
        gamma, beta = (1 + 0.2 * torch.randn(Cin, generator=g)).to(DEV), (0.2 * torch.randn(Cin, generator=g)).to(DEV)
        w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) / np.sqrt(27 * Cin)).to(DEV)
        G = 8 if Cin % 8 == 0 else 1
        y = B.single_conv_gcr(x, gamma, beta, w, G, x_from_relu=False)
        carried = B._peek_stats(y)
        assert carried is not None and carried.dtype == torch.float64
        V = dims[0] * dims[1] * dims[2]
        ref = B.channel_stats(y, None, N, V, Cout)
        close(carried, ref, 5e-7 * float(ref.abs().max()), 5e-7)   # fp32 partial sums of <= 64 values in both
        before = dict(B.STATS_STATS)
        B.single_conv_gcr(y, torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV),
                          (torch.randn(8, Cout, 3, 3, 3, generator=g) / 10).to(DEV), 8 if Cout % 8 == 0 else 1)
        assert B.STATS_STATS["carried"] == before["carried"] + 1 and B.STATS_STATS["measured"] == before["measured"]
        y.add_(1.0)                                   # an in-place edit invalidates the tag
        assert B._peek_stats(y) is None
    finally:
        B.set_conv_mode(old)


def test_upcat_statistics_from_sources():
    from keymorph_amd import backbone_ops as B
    g = gen(32)
    skip, low = torch.randn(2, 8, 6, 10, 5, generator=g).to(DEV), torch.randn(2, 4, 3, 5, 7, generator=g).to(DEV)
    B._tag_stats(skip, B.channel_stats(skip, None, 2, 480, 5))
    B._tag_stats(low, B.channel_stats(low, None, 2, 60, 7))
    out = B.upcat(skip, low)
    ref = B.channel_stats(out, None, 2, 480, 12)
    close(B._peek_stats(out), ref, 5e-7 * float(ref.abs().max()), 5e-7)
    ragged = B.upcat(torch.randn(2, 7, 6, 10, 5, generator=g).to(DEV), low)     # not an exact 2x: measured later
    assert B._peek_stats(ragged) is None


@pytest.mark.parametrize("dims", [(8, 6, 10), (7, 5, 9)])
def test_pool_fork_sums_both_gradients_in_one_pass(dims):
    """encoder output -> (max-pool to the next level, skip connection into upsample+concat): pool_fork + the lazy
    (strided-view) skip gradient of upcat == torch autograd on max_pool3d / interpolate / cat."""
    from keymorph_amd import backbone_ops as B
    g = gen(12)
    C, Cl = 6, 7
    dl = tuple(d // 2 for d in dims)
    x = torch.randn(2, C, *dims, generator=g)
    low = torch.randn(2, Cl, *dl, generator=g)
    cp, cc = torch.randn(2, C, *dl, generator=g), torch.randn(2, C + Cl, *dims, generator=g)
    xr, lr = x.clone().requires_grad_(True), low.clone().requires_grad_(True)
    pr = F.max_pool3d(xr, 2)
    cr = torch.cat([xr, F.interpolate(lr, size=dims, mode="nearest")], 1)
    ((pr * cp).sum() + (cr * cc).sum()).backward()
    for lazy in (True, False):
        xh, lh = ndhwc(x).to(DEV).requires_grad_(True), ndhwc(low).to(DEV).requires_grad_(True)
        ph, skip = B.pool_fork(xh)
        ch = B.upcat(skip, lh, lazy)
        ((ph * ndhwc(cp).to(DEV)).sum() + (ch * ndhwc(cc).to(DEV)).sum()).backward()
        close(ncdhw(ph), pr, 0)
        close(ncdhw(ch), cr, 0)
        close(ncdhw(xh.grad), xr.grad, 1e-6)
        close(ncdhw(lh.grad), lr.grad, 1e-6)
    # only one of the two branches has a gradient
    xh = ndhwc(x).to(DEV).requires_grad_(True)
    ph, skip = B.pool_fork(xh)
    (ph * ndhwc(cp).to(DEV)).sum().backward()
    xr.grad = None
    (F.max_pool3d(xr, 2) * cp).sum().backward()
    close(ncdhw(xh.grad), xr.grad, 0)
    xh = ndhwc(x).to(DEV).requires_grad_(True)
    ph, skip = B.pool_fork(xh)
    (skip * 2.0).sum().backward()
    close(xh.grad, torch.full_like(xh, 2.0), 0)


@pytest.mark.parametrize("name", ["tunet", "unet"])
def test_unet_golden(name):
    """Whole network vs the reference's own output + parameter gradients (tests/golden)."""
    from keymorph_amd.unet3d.model import TruncatedUNet3D, UNet3D
    g = golden("backbones_32.npz")
    if name == "tunet":
        net = TruncatedUNet3D(1, 16, 1, final_sigmoid=False, f_maps=8, layer_order="gcr", num_groups=8,
                              num_levels=4, is_segmentation=False, conv_padding=1)
        shapes = unet_shapes(16, 8, trunc=1)
    else:
        net = UNet3D(1, 8, final_sigmoid=False, f_maps=8, layer_order="gcr", num_groups=8, num_levels=4,
                     is_segmentation=False, conv_padding=1)
        shapes = unet_shapes(8, 8)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    net.load_state_dict(seeded_state_dict(shapes, 100), strict=True)
    net = net.to(DEV).train()
    y = net(T(g["x"]).to(DEV))
    close(y, g[f"{name}_out"], 1e-4, 1e-4)
    (y * T(g[f"{name}_cot"]).to(DEV)).sum().backward()
    # Gradients vs the oracle recomputed here (same weights): relative L2 per parameter.  A handful of
    # voxels sit within fp32 noise of a ReLU kink and flip their mask between ANY two fp32
    # implementations (each moves a 32k-term sum by ~1%), so max-abs is not a meaningful metric.
    from oracle import keymorph_oracle as O
    sdr = {k: v.clone().requires_grad_(True) for k, v in seeded_state_dict(shapes, 100).items()}
    yr = O.unet3d_forward(sdr, T(g["x"]), 4, 1 if name == "tunet" else 0, 8)
    (yr * T(g[f"{name}_cot"])).sum().backward()
    worst = 0.0
    for k, p in net.named_parameters():
        r = sdr[k].grad.double().reshape(-1)
        e = float((p.grad.cpu().double().reshape(-1) - r).norm() / r.norm())
        worst = max(worst, e)
        assert e < 3e-2, (k, e)
        ref = g[f"{name}_grad::{k}"]   # reference-generated (sum, abs-sum, first 8)
        gf = p.grad.reshape(-1)
        got = torch.cat([gf.sum()[None], gf.abs().sum()[None], gf[:8]])
        close(got[1:2], ref[1:2], 0, 3e-2)
    print(name, "worst param-grad rel L2 vs oracle:", worst)


@pytest.mark.parametrize("norm", ["instance", "none"])
def test_convnet_golden(norm):
    """ConvNet (keymorph/net.py) forward vs the reference golden; parameter gradients vs the oracle."""
    from keymorph_amd.net import ConvNet
    from oracle import keymorph_oracle as O
    from tests.util import convnet_shapes
    g = golden("backbones_32.npz")
    name = "convnet" if norm == "instance" else "convnet_none"
    net = ConvNet(3, 1, 8, norm)
    shapes = convnet_shapes(8)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    net.load_state_dict(seeded_state_dict(shapes, 100), strict=True)
    net = net.to(DEV).train()
    y = net(T(g["x"]).to(DEV))
    ref = g[f"{name}_out"]
    close(y, ref, 2e-4 * max(1.0, float(np.abs(ref).max())), 1e-3)
    (y * T(g[f"{name}_cot"]).to(DEV)).sum().backward()
    sdr = {k: v.clone().requires_grad_(True) for k, v in seeded_state_dict(shapes, 100).items()}
    yr = O.convnet_forward(sdr, T(g["x"]), norm)
    (yr * T(g[f"{name}_cot"])).sum().backward()
    for k, p in net.named_parameters():
        r = sdr[k].grad.double().reshape(-1)
        if norm == "instance" and k.endswith("conv.bias"):
            # InstanceNorm removes the per-channel mean, so d/d(bias) == 0 exactly: both sides are round-off
            wn = float(sdr[k.replace("bias", "weight")].grad.double().norm())
            assert float(p.grad.double().norm()) < 1e-3 * wn and float(r.norm()) < 1e-3 * wn, k
            continue
        e = float((p.grad.cpu().double().reshape(-1) - r).norm() / (r.norm() + 1e-30))
        assert e < 3e-2, (k, e)


@pytest.mark.parametrize("shape,N", [((32, 32, 32), 1), ((16, 48, 32), 2)])
def test_convnet_lazy_instance_norm_equals_block_by_block(shape, N, monkeypatch):
    """ConvNet(instance): the lazy route (IN + ReLU + MaxPool inside the next convolution's loader, three-launch backward:
    backbone_ops.convnet_instance_lazy) against the block-by-block route (KEYMORPH_NO_LAZY_IN=1: conv, statistics pass,
    norm apply, pooling, and their separate backward passes) and against the oracle's autograd (keymorph/net.py:7-36,
    layers.py:137-187): same keypoint logits, every weight gradient at the fp32 rounding level of the two HIP routes."""
    from keymorph_amd import backbone_ops as B
    from keymorph_amd.net import ConvNet
    from oracle import keymorph_oracle as O
    from tests.util import convnet_shapes
    shapes = convnet_shapes(8)
    sd = seeded_state_dict(shapes, 101)
    x = torch.rand((N, 1) + shape, generator=gen(11))
    outs = {}
    for lazy in (True, False):
        if lazy:
            monkeypatch.delenv("KEYMORPH_NO_LAZY_IN", raising=False)
        else:
            monkeypatch.setenv("KEYMORPH_NO_LAZY_IN", "1")
        net = ConvNet(3, 1, 8, "instance")
        net.load_state_dict(sd, strict=True)
        net = net.to(DEV).train()
        before = B.LAZY_IN_STATS["units"]
        y = net(x.to(DEV))
        assert (B.LAZY_IN_STATS["units"] - before) == (9 if lazy else 0)
        cot = torch.linspace(-1, 1, y.numel(), device=DEV).reshape(y.shape)
        (y * cot).sum().backward()
        outs[lazy] = (y.detach().cpu(), {k: p.grad.detach().cpu().double() for k, p in net.named_parameters()})
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    yr = O.convnet_forward(sdr, x, "instance")
    (yr * torch.linspace(-1, 1, yr.numel()).reshape(yr.shape)).sum().backward()
    scale = max(1.0, float(yr.abs().max()))
    close(outs[True][0], yr.detach(), 2e-4 * scale, 1e-3)
    close(outs[True][0], outs[False][0], 2e-5 * scale, 1e-4)
    for k in outs[True][1]:
        a, b, r = outs[True][1][k], outs[False][1][k], sdr[k].grad.double()
        if k.endswith("conv.bias"):          # d/d(bias) == 0 under InstanceNorm: exactly 0 here, round-off in the others
            assert float(a.abs().max()) == 0.0 and float(r.norm()) < 1e-3 * float(sdr[k.replace("bias", "weight")].grad.norm())
            continue
        assert float((a - b).norm() / (b.norm() + 1e-30)) < 2e-3, (k, "lazy vs block-by-block")
        assert float((a - r).norm() / (r.norm() + 1e-30)) < 3e-2, (k, "lazy vs oracle")


def test_convnet_instance_image_gradient_when_the_input_requires_it():
    """An image that requires a gradient (saliency / adversarial use) gets it through ConvNet(instance): the fused lazy
    units never form d/d(image), so such an input must take the block-by-block route -- against the oracle's autograd."""
    from keymorph_amd import backbone_ops as B
    from keymorph_amd.net import ConvNet
    from oracle import keymorph_oracle as O
    from tests.util import convnet_shapes
    shapes = convnet_shapes(8)
    sd = seeded_state_dict(shapes, 103)
    x = torch.rand((1, 1, 32, 32, 32), generator=gen(12))
    net = ConvNet(3, 1, 8, "instance")
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).train()
    xh = x.to(DEV).requires_grad_(True)
    before = B.LAZY_IN_STATS["units"]
    y = net(xh)
    assert B.LAZY_IN_STATS["units"] == before, "the lazy units ran although the image requires a gradient"
    cot = torch.linspace(-1, 1, y.numel(), device=DEV).reshape(y.shape)
    (y * cot).sum().backward()
    assert xh.grad is not None
    xr = x.clone().requires_grad_(True)
    yr = O.convnet_forward({k: v.clone() for k, v in sd.items()}, xr, "instance")
    (yr * cot.cpu()).sum().backward()
    e = float((xh.grad.cpu().double() - xr.grad.double()).norm() / (xr.grad.double().norm() + 1e-30))
    assert e < 3e-2, e
    # and without the requirement the lazy units are back
    y2 = net(x.to(DEV))
    assert B.LAZY_IN_STATS["units"] - before == 9
    close(y2, y.detach(), 2e-5 * max(1.0, float(y.abs().max())), 1e-4)


def test_convnet_instance_128_vs_oracle_forward_and_autograd():
    """The reference's other backbone at a size its blocks are not toys (keymorph/net.py:7-36; 128^3, 64 keypoints, the
    lazy-InstanceNorm route): keypoint logits and center-of-mass keypoints against the oracle, and every weight gradient of
    a keypoint-space loss against the oracle's autograd (host: ~20 s, in a child process: tests/oracle_at_size.py)."""
    from keymorph_amd import ops as kops
    from keymorph_amd.net import ConvNet
    from tests.oracle_at_size import oracle_convnet
    Kc, S = 64, 128
    ref = oracle_convnet(S, Kc)
    net = ConvNet(3, 1, Kc, "instance")
    net.load_state_dict(ref["sd"], strict=True)
    net = net.to(DEV).train()
    y = net(ref["x"].to(DEV))
    pts = kops.com3d(y)
    (pts * ref["cot"].to(DEV)).sum().backward()
    scale = float(ref["y"].abs().max())
    e_y = float((y.detach().cpu() - ref["y"]).abs().max()) / scale
    e_p = float((pts.detach().cpu() - ref["pts"]).abs().max())
    num = den = 0.0
    worst = ("", 0.0)
    for k, p in net.named_parameters():
        if k.endswith("conv.bias"):
            continue                                   # exactly zero under InstanceNorm (round-off in the oracle)
        a, r = p.grad.detach().cpu().double(), ref["grads"][k].double()
        n, d = float((a - r).pow(2).sum()), float(r.pow(2).sum())
        num, den = num + n, den + d
        if (n / (d + 1e-300)) ** 0.5 > worst[1]:
            worst = (k, (n / (d + 1e-300)) ** 0.5)
    e_g = (num / den) ** 0.5
    print(f"ConvNet 128^3 vs oracle: logits {e_y:.2e} of their maximum, keypoints {e_p:.2e}, weight gradients rel-L2 {e_g:.2e} "
          f"(worst tensor {worst[0]} {worst[1]:.2e})")
    assert e_y <= 1e-4 and e_p <= 1e-4, (e_y, e_p)
    assert e_g <= 2e-3 and worst[1] <= 1e-2, (e_g, worst)


def test_convblock_group_norm():
    from keymorph_amd import backbone_ops as B
    g = gen(5)
    x = torch.randn(2, 16, 6, 6, 10, generator=g)
    w = torch.randn(24, 16, 3, 3, 3, generator=g) / np.sqrt(27 * 16)
    b = 0.1 * torch.randn(24, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(24, generator=g), 0.1 * torch.randn(24, generator=g)
    cot = torch.randn(2, 24, 6, 6, 10, generator=g)
    R = [t.clone().requires_grad_(True) for t in (x, w, b, gamma, beta)]
    yr = F.relu(F.group_norm(F.conv3d(R[0], R[1], R[2], padding=1), 8, R[3], R[4], 1e-5))
    (yr * cot).sum().backward()
    Hh = [ndhwc(x).to(DEV).requires_grad_(True)] + [t.to(DEV).requires_grad_(True) for t in (w, b, gamma, beta)]
    yh = B.conv_block(*Hh, 8)
    (yh * ndhwc(cot).to(DEV)).sum().backward()
    close(ncdhw(yh), yr, 2e-5, 1e-4)
    for a, r, perm in zip(Hh, R, (True, False, False, False, False)):
        ga = ncdhw(a.grad) if perm else a.grad
        close(ga, r.grad, 2e-4 * float(r.grad.abs().max()), 1e-3)


def test_convblock_batch_norm():
    """ConvBlock(norm_type="batch") (keymorph/layers.py:137-187): training mode = batch statistics over (N, D, H, W)
    + running-average update, evaluation mode = the running statistics as a fixed affine map; forward, every gradient
    and the buffers against torch's Conv3d -> BatchNorm3d -> ReLU, two training steps then one evaluation pass."""
    from keymorph_amd import backbone_ops as B
    from keymorph_amd.net import ConvBlock
    g = gen(6)
    Cin, Cout, dims = 16, 24, (6, 5, 10)
    torch.manual_seed(4)
    blk = ConvBlock(Cin, Cout, 1, "batch", down_sample=False, dim=3)
    with torch.no_grad():
        blk.norm.weight.copy_(1 + 0.1 * torch.randn(Cout, generator=g))
        blk.norm.bias.copy_(0.1 * torch.randn(Cout, generator=g))
    ref_conv = torch.nn.Conv3d(Cin, Cout, 3, padding=1)
    ref_bn = torch.nn.BatchNorm3d(Cout)
    ref_conv.load_state_dict(blk.conv.state_dict())
    ref_bn.load_state_dict(blk.norm.state_dict())
    assert sorted(blk.state_dict()) == sorted(["conv.weight", "conv.bias", "norm.weight", "norm.bias", "norm.running_mean",
                                               "norm.running_var", "norm.num_batches_tracked"])
    blk = blk.to(DEV)
    for step, train in enumerate((True, True, False)):
        blk.train(train); ref_conv.train(train); ref_bn.train(train)
        x = torch.randn(3, Cin, *dims, generator=g) + 0.3
        cot = torch.randn(3, Cout, *dims, generator=g)
        for m in (blk, ref_conv, ref_bn):
            m.zero_grad(set_to_none=True)
        xr = x.clone().requires_grad_(True)
        yr = F.relu(ref_bn(ref_conv(xr)))
        (yr * cot).sum().backward()
        xh = ndhwc(x).to(DEV).requires_grad_(True)
        yh = blk(xh)
        (yh * ndhwc(cot).to(DEV)).sum().backward()
        close(ncdhw(yh), yr, 2e-5, 1e-4)
        close(ncdhw(xh.grad), xr.grad, 2e-4 * float(xr.grad.abs().max()), 1e-3)
        for a, r in ((blk.conv.weight, ref_conv.weight), (blk.conv.bias, ref_conv.bias), (blk.norm.weight, ref_bn.weight),
                     (blk.norm.bias, ref_bn.bias)):
            # (the conv bias gradient under training-mode batch norm is analytically zero: compare absolutely)
            close(a.grad, r.grad, 2e-4 * float(r.grad.abs().max()) + 2e-4, 1e-3)
        close(blk.norm.running_mean, ref_bn.running_mean, 1e-6, 1e-5)
        close(blk.norm.running_var, ref_bn.running_var, 1e-6, 1e-5)
        assert int(blk.norm.num_batches_tracked) == int(ref_bn.num_batches_tracked) == min(step + 1, 2)


@pytest.mark.parametrize("cfg", [(2, 16, 16, (6, 7, 9)), (1, 64, 200, (8, 8, 20)), (2, 8, 40, (3, 5, 70)),
                                 (1, 32, 130, (16, 16, 16)), (2, 64, 96, (4, 6, 64)), (1, 24, 40, (2, 3, 128))])
def test_fused_head_matches_unfused(cfg):
    """fused conv1x1 + ReLU + CoM (no heat-map) == pointwise -> com3d, values and all gradients."""
    from keymorph_amd import backbone_ops as B, ops
    N, Cin, Cout, dims = cfg
    g = gen(9)
    x = torch.randn(N, *dims, Cin, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, 1, generator=g) / np.sqrt(Cin)
    b = 0.3 * torch.randn(Cout, generator=g)
    cot = torch.randn(N, Cout, 3, generator=g)
    A = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    Bv = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    pa = B.head_com(*A)
    pb = ops.com3d(B.pointwise(*Bv))
    (pa * cot.to(DEV)).sum().backward()
    (pb * cot.to(DEV)).sum().backward()
    close(pa, pb, 2e-6, 1e-5)
    # and against the oracle
    from oracle import keymorph_oracle as O
    ref = O.center_of_mass(F.conv3d(ncdhw(x), w, b), "ij")
    close(pa, ref, 5e-6, 1e-5)
    for u, v in zip(A, Bv):
        close(u.grad, v.grad, 2e-4 * float(v.grad.abs().max()), 1e-3)
    # feat_from_relu: the feature gradient comes back multiplied by (feat > 0) (what the producing ReLU's backward
    # would do), the parameter gradients are untouched -- in every arithmetic mode
    old = B.CONV_MODE
    try:
        for mode in ("f16x3", "bf16x6", "f32"):
            B.set_conv_mode(mode)
            C = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
            (B.head_com(*C, feat_from_relu=True) * cot.to(DEV)).sum().backward()
            close(C[0].grad, Bv[0].grad * (Bv[0] > 0), 2e-4 * float(Bv[0].grad.abs().max()), 1e-3)
            close(C[1].grad, Bv[1].grad, 2e-4 * float(Bv[1].grad.abs().max()), 1e-3)
            close(C[2].grad, Bv[2].grad, 2e-4 * float(Bv[2].grad.abs().max()), 1e-3)
    finally:
        B.set_conv_mode(old)


@pytest.mark.parametrize("cfg", [(2, 64, 512, (8, 16, 64)), (1, 64, 200, (4, 8, 128)), (3, 32, 96, (6, 8, 32)),
                                 (2, 24, 130, (2, 4, 96))])
@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_fused_head_mask_backward(cfg, mode):
    """On whole-x-row geometries the forward stores [h > 0] and the backward kernels skip recomputing the logits
    (csrc/headcom.hip, headcom_bwd_{w,feat}_mask_kernel).  The mask backward must (i) actually run, (ii) agree with the
    recomputing kernels to rounding (same sign pattern, dh coefficients rounded differently) and (iii) with fp64 autograd
    of the materialised heat-map (keymorph/layers.py:92-134 on keymorph/unet3d/model.py:387-391)."""
    from keymorph_amd import backbone_ops as B
    from oracle import keymorph_oracle as O
    N, Cin, Cout, dims = cfg
    g = gen(31)
    x = torch.randn(N, *dims, Cin, generator=g).abs()           # a ReLU output, like the decoder's last block
    w = torch.randn(Cout, Cin, 1, 1, 1, generator=g) / np.sqrt(Cin)
    b = 0.3 * torch.randn(Cout, generator=g)
    cot, cw = torch.randn(N, Cout, 3, generator=g), torch.randn(N, Cout, generator=g)
    R = [t.clone().double().requires_grad_(True) for t in (x, w, b)]
    h = F.conv3d(ncdhw(R[0]), R[1], R[2])
    ((O.center_of_mass(h, "ij") * cot.double()).sum() + (F.relu(h).flatten(2).sum(-1) * cw.double()).sum()).backward()
    old, old_mask = B.CONV_MODE, B.HEAD_MASK
    grads = {}
    try:
        B.set_conv_mode(mode)
        for use_mask in (True, False):
            B.HEAD_MASK = use_mask
            before = dict(B.HEAD_STATS)
            A = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
            pa, wa = B.head_com_power(*A, feat_from_relu=False)
            ((pa * cot.to(DEV)).sum() + (wa * cw.to(DEV)).sum()).backward()
            assert B.HEAD_STATS["mask" if use_mask else "recompute"] == before["mask" if use_mask else "recompute"] + 1
            grads[use_mask] = [t.grad.cpu().double() for t in A]
            close(pa, O.center_of_mass(h, "ij").detach(), 5e-6, 1e-5)
        # no-grad forward: no mask is written
        before = dict(B.HEAD_STATS)
        B.HEAD_MASK = True
        with torch.no_grad():
            B.head_com(*[t.to(DEV) for t in (x, w, b)])
        assert B.HEAD_STATS["mask"] == before["mask"]
    finally:
        B.set_conv_mode(old)
        B.HEAD_MASK = old_mask
    for gm, gr, ref in zip(grads[True], grads[False], R):
        rn = float(ref.grad.norm())
        assert float((gm - gr).norm()) < 2e-6 * rn, ("mask vs recompute", float((gm - gr).norm()) / rn)
        assert float((gm - ref.grad).norm()) < 2e-5 * rn, ("mask vs fp64", float((gm - ref.grad).norm()) / rn)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6", "f32"])
def test_fused_head_power_output_and_gradient(mode):
    """second output of the fused head: power = sum relu(h) (keymorph/model.py:96-109) and its gradient, which rides
    in the same backward pass as the center-of-mass gradient; vs torch autograd on the materialised heat-map."""
    from keymorph_amd import backbone_ops as B
    from oracle import keymorph_oracle as O
    N, Cin, Cout, dims = 2, 16, 40, (6, 7, 9)
    g = gen(19)
    x = torch.randn(N, *dims, Cin, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, 1, generator=g) / np.sqrt(Cin)
    b = 0.3 * torch.randn(Cout, generator=g)
    cp, cw = torch.randn(N, Cout, 3, generator=g), torch.randn(N, Cout, generator=g)
    R = [t.clone().requires_grad_(True) for t in (x, w, b)]
    h = F.conv3d(ncdhw(R[0]), R[1], R[2])
    pr, wr = O.center_of_mass(h, "ij"), F.relu(h).flatten(2).sum(-1)
    ((pr * cp).sum() + (wr * cw).sum()).backward()
    old = B.CONV_MODE
    try:
        B.set_conv_mode(mode)
        A = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
        pa, wa = B.head_com_power(*A)
        ((pa * cp.to(DEV)).sum() + (wa * cw.to(DEV)).sum()).backward()
        close(pa, pr, 5e-6, 1e-5)
        close(wa, wr, 1e-5 * float(wr.detach().abs().max()), 1e-5)
        for u, v in zip(A, R):
            close(u.grad, v.grad, 2e-4 * float(v.grad.abs().max()), 1e-3)
        # power gradient alone (no dpts)
        A2 = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
        (B.head_com_power(*A2)[1] * cw.to(DEV)).sum().backward()
        R2 = [t.clone().requires_grad_(True) for t in (x, w, b)]
        (F.relu(F.conv3d(ncdhw(R2[0]), R2[1], R2[2])).flatten(2).sum(-1) * cw).sum().backward()
        for u, v in zip(A2, R2):
            close(u.grad, v.grad, 2e-4 * float(v.grad.abs().max()), 1e-3)
    finally:
        B.set_conv_mode(old)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6", "f32"])
def test_fused_head_dead_and_faint_keypoint_channels(mode):
    """Keypoint channels whose logits are <= 0 everywhere (sum relu(h) == 0: the center of mass is 0 / 1e-8) or positive
    at a single voxel happen after a few training steps.  Their 1 / mass gradient coefficients are up to 1e13 times a
    live channel's; they must not cost the live channels their gradient (one power-of-two range scale for all channels
    pushed them below fp16's range: 74 % error on the final conv's weight gradient at 256^3 before the fix)."""
    from keymorph_amd import backbone_ops as B
    from oracle import keymorph_oracle as O
    N, Cin, Cout, dims = 2, 16, 40, (6, 8, 32)
    g = gen(29)
    x = torch.randn(N, *dims, Cin, generator=g).abs()
    w = torch.randn(Cout, Cin, 1, 1, 1, generator=g) / np.sqrt(Cin)
    b = 0.3 * torch.randn(Cout, generator=g)
    w[3], b[3] = -w[3].abs(), -1.0                     # dead in every sample: non-negative features, negative weights
    w[17], b[17] = -w[17].abs(), -0.5
    w[9] = -w[9].abs()                                 # faint: positive (1e-3) at exactly one voxel of one sample
    resp9 = (x.double() * w[9].reshape(-1).double()).sum(-1)          # (N, D, H, W), all negative
    b[9] = 1e-3 - float(resp9.max())
    cot = torch.randn(N, Cout, 3, generator=g)
    R = [t.clone().double().requires_grad_(True) for t in (x, w, b)]
    h = F.conv3d(ncdhw(R[0]), R[1], R[2])
    mass = F.relu(h).flatten(2).sum(-1).detach()
    assert float(mass[:, 3].max()) == 0 and float(mass[:, 17].max()) == 0
    assert 0 < float(mass[:, 9].max()) < 1e-4 * float(mass.median())
    (O.center_of_mass(h, "ij") * cot.double()).sum().backward()
    old = B.CONV_MODE
    try:
        B.set_conv_mode(mode)
        A = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
        pa = B.head_com(*A)
        (pa * cot.to(DEV)).sum().backward()
        live = [k for k in range(Cout) if k not in (3, 9, 17)]
        close(pa[:, live], O.center_of_mass(h, "ij").detach()[:, live], 5e-6, 1e-5)
        gw, rw = A[1].grad.cpu().double(), R[1].grad
        for k in live:                                 # every live channel keeps its own relative accuracy
            assert float((gw[k] - rw[k]).norm() / rw[k].norm()) < 2e-3, (k, mode)
        assert float(gw[3].abs().max()) == 0 and float(gw[17].abs().max()) == 0
        close(A[2].grad[live], R[2].grad[live], 2e-4 * float(R[2].grad[live].abs().max()), 1e-3)
        gx, rx = A[0].grad.cpu().double(), R[0].grad
        assert float((gx - rx).norm() / rx.norm()) < 2e-3
        # an extremely faint channel (mass 1e-9: its coefficients are ~1e14 times a live channel's -- beyond what one
        # range scale can carry next to the others): the split-fp16 mode hands this backward to the three-term kernels
        b2 = b.clone()
        b2[9] = float(np.float32(1e-7 - float(resp9.max())))
        R2 = [t.clone().double().requires_grad_(True) for t in (x, w, b2)]
        h2 = F.conv3d(ncdhw(R2[0]), R2[1], R2[2])
        m2 = F.relu(h2).flatten(2).sum(-1).detach()
        m9 = float(m2[:, 9].max())
        if 0 < m9 < 1e-5:                               # (fp32 rounding of the bias may kill the voxel: then nothing to test)
            (O.center_of_mass(h2, "ij") * cot.double()).sum().backward()
            A2 = [t.to(DEV).requires_grad_(True) for t in (x, w, b2)]
            (B.head_com(*A2) * cot.to(DEV)).sum().backward()
            gw2, rw2 = A2[1].grad.cpu().double(), R2[1].grad
            for k in live:
                # (measured: 9e-6 with the hand-over, 1.5e-1 without it)
                assert float((gw2[k] - rw2[k]).norm() / rw2[k].norm()) < 5e-4, (k, mode, "extremely faint channel")
    finally:
        B.set_conv_mode(old)


@pytest.mark.parametrize("cfg", [(1, 16, 32, (6, 10, 40), 8), (2, 8, 8, (5, 7, 9), 8), (1, 1, 4, (8, 8, 8), 1),
                                 (1, 48, 64, (4, 9, 33), 8), (1, 12, 20, (4, 4, 6), 4)])
def test_conv_arithmetic_modes_vs_fp64(cfg):
    """GroupNorm -> conv3 -> ReLU, forward and all gradients, in every arithmetic mode against an fp64 reference:
    the split-operand modes must be fp32-class (bound 3e-6 relative to the tensor's max; measured ~5e-7 for f16x3 and
    bf16x6, 6.5e-7 for the plain fp32-MFMA kernel), and tiny / huge operand magnitudes must not matter for f16x3."""
    from keymorph_amd import backbone_ops as B
    N, Cin, Cout, dims, G = cfg
    old = B.CONV_MODE
    try:
        for amp_x, amp_w, amp_c in ((1.0, 1.0, 1.0), (3e-4, 40.0, 2e-6), (5e3, 1e-3, 3e4)):
            g = gen(1)
            x = torch.randn(N, Cin, *dims, generator=g) * amp_x + 0.3 * amp_x
            gamma, beta = 1 + 0.2 * torch.randn(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g)
            w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / np.sqrt(27 * Cin) * amp_w
            cot = torch.randn(N, Cout, *dims, generator=g) * amp_c
            R = [t.clone().double().requires_grad_(True) for t in (x, gamma, beta, w)]
            yr = F.relu(F.conv3d(F.group_norm(R[0], G, R[1], R[2], 1e-5), R[3], None, padding=1))
            (yr * cot.double()).sum().backward()
            for mode in ("f32", "bf16x6", "f16x3"):
                B.set_conv_mode(mode)
                Hh = [ndhwc(x).to(DEV).requires_grad_(True)] + [t.to(DEV).requires_grad_(True) for t in (gamma, beta, w)]
                yh = B.single_conv_gcr(*Hh, G, x_from_relu=False)
                (yh * ndhwc(cot).to(DEV)).sum().backward()

                def rel(a, b):
                    return float((a.detach().cpu().double() - b).abs().max()) / (float(b.abs().max()) + 1e-300)
                assert rel(ncdhw(yh), yr.detach()) < 3e-6, (mode, amp_x)
                assert rel(ncdhw(Hh[0].grad), R[0].grad) < 5e-6, (mode, amp_x)
                assert rel(Hh[3].grad, R[3].grad) < 3e-6, (mode, amp_x)
                assert rel(Hh[1].grad, R[1].grad) < 2e-5 and rel(Hh[2].grad, R[2].grad) < 2e-5, (mode, amp_x)
    finally:
        B.set_conv_mode(old)


def test_absmax_scale():
    """kmh_absmax_scale: S = 2^k with max|x| S in [2^14, 2^15), any alignment / length, min_abs floor, zeros."""
    from keymorph_amd import backbone_ops as B
    g = gen(2)
    base = torch.randn(100003, generator=g).to(DEV)
    for off, n, amp in ((0, 100003, 1.0), (1, 4097, 3e-5), (3, 7, 1e4), (2, 1, 0.37), (5, 64, 2.0 ** 14), (0, 33, 0.0)):
        x = base[off:off + n] * amp
        s = B.absmax_scale(x).cpu()
        m = float(x.abs().max())
        assert float(s[0]) * float(s[1]) == 1.0 and float(torch.log2(s[0])).is_integer()
        if m > 0:
            assert 2.0 ** 14 < m * float(s[0]) <= 2.0 ** 15, (off, n, amp, m, s)
        else:
            assert float(s[0]) == 1.0
    s = B.absmax_scale(base[:100] * 1e-3, 1.0).cpu()          # floor: the virtual "ones" channel of the first layer
    assert float(s[0]) == 2.0 ** 14


@pytest.mark.parametrize("cfg", [(2, 24, 16, (5, 9, 37)), (1, 64, 40, (4, 8, 32))])
def test_double_conv_blocked_gradient_handoff(cfg, monkeypatch):
    """The hidden activation's gradient travels channel-blocked between the two SingleConvs of a DoubleConv (an
    internal layout, backbone_ops.grad_blocked_ok): every gradient must be BIT-identical to the (N,D,H,W,C) hand-off."""
    from keymorph_amd import backbone_ops as B
    from keymorph_amd.unet3d.model import DoubleConv
    N, Cin, Cout, dims = cfg
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        torch.manual_seed(3)
        blk = DoubleConv(Cin, Cout, encoder=False).to(DEV)
        x0 = torch.randn(N, *dims, Cin, generator=gen(9)).abs().to(DEV)
        cot = torch.randn(N, *dims, Cout, generator=gen(10)).to(DEV)

        def run():
            for p_ in blk.parameters():
                p_.grad = None
            x = x0.clone().requires_grad_(True)
            y = blk(x, True)               # out_premasked: the cotangent is masked below, as a SingleConv's would be
            (y * (cot * (y.detach() > 0))).sum().backward()
            return [x.grad.clone()] + [p_.grad.clone() for p_ in blk.parameters()]

        before = B.BLOCKED_STATS["handoffs"]
        got = run()
        assert B.BLOCKED_STATS["handoffs"] == before + 1, "the blocked hand-off did not run"
        monkeypatch.setenv("KEYMORPH_NO_BLOCKED_GRADS", "1")
        ref = run()
        assert B.BLOCKED_STATS["handoffs"] == before + 1
        for a, r in zip(got, ref):
            assert torch.equal(a, r)
    finally:
        B.set_conv_mode(old)


def test_single_conv_statistics_fold_and_zero_gamma_fallback(monkeypatch):
    """GroupNorm's backward statistics come from the data gradient's epilogue and the per-sample weight gradient
    (no pass over dxn and x): same gradients as the direct statistics; a gamma that is exactly 0 (where dgamma cannot be
    recovered from the normalised input) flips the device-side gate to the direct path."""
    from keymorph_amd import backbone_ops as B
    g = gen(21)
    N, Cin, Cout, D, H, W = 3, 16, 24, 6, 9, 37
    x = torch.randn(N, Cin, D, H, W, generator=g).abs() + 0.1 * torch.randn(N, Cin, D, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / np.sqrt(27 * Cin)
    cot = torch.randn(N, Cout, D, H, W, generator=g)
    for zero_gamma in (False, True):
        gamma = 1 + 0.2 * torch.randn(Cin, generator=g)
        beta = 0.2 * torch.randn(Cin, generator=g)
        if zero_gamma:
            gamma[5] = 0.0
        R = [t.clone().requires_grad_(True) for t in (x, gamma, beta, w)]
        yr = F.relu(F.conv3d(F.group_norm(R[0], 8, R[1], R[2], 1e-5), R[3], None, padding=1))
        (yr * cot).sum().backward()
        grads = {}
        for fold in (True, False):
            if fold:
                monkeypatch.delenv("KEYMORPH_NO_STATS_FOLD", raising=False)
            else:
                monkeypatch.setenv("KEYMORPH_NO_STATS_FOLD", "1")
            Hh = [ndhwc(x).to(DEV).requires_grad_(True)] + [t.to(DEV).requires_grad_(True) for t in (gamma, beta, w)]
            before = B.STATS_STATS.get("folded", 0)
            yh = B.single_conv_gcr(Hh[0], Hh[1], Hh[2], Hh[3], 8, x_from_relu=False)
            (yh * ndhwc(cot).to(DEV)).sum().backward()
            assert (B.STATS_STATS.get("folded", 0) - before) == (1 if fold and B.conv_emits_stats() else 0)   # not in f32 mode
            grads[fold] = [ncdhw(Hh[0].grad)] + [t.grad for t in Hh[1:]]
            for a, r in zip(grads[fold], R):
                close(a, r.grad, 1e-4 * float(r.grad.abs().max()), 1e-3)
        for a, b in zip(grads[True], grads[False]):     # the two routes agree far inside the parity bar
            close(a, b, 3e-6 * float(b.abs().max()), 1e-4)


@pytest.mark.parametrize("cfg", [(2, 16, 24, 32, (3, 5, 18)), (1, 8, 40, 72, (4, 4, 33)), (1, 64, 128, 64, (2, 8, 32))])
@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_decoder_conv_without_the_upsampled_tensor(cfg, mode, monkeypatch):
    """conv3(GN(cat(skip, up2(low)))): the upsampled channels' contribution is computed from `low` with the 8 pre-summed
    taps per output parity (conv3_up2) and added in the skip channels' 27-tap launch -- same output and statistics as
    the convolution over the materialised concatenation, and as PyTorch."""
    from keymorph_amd import backbone_ops as B
    N, Cs, Cl, Cout, ld = cfg
    dims = tuple(2 * d for d in ld)
    old = B.CONV_MODE
    try:
        B.set_conv_mode(mode)
        g = gen(33)
        skip = torch.randn(N, *dims, Cs, generator=g).abs().to(DEV)
        low = torch.randn(N, *ld, Cl, generator=g).abs().to(DEV)
        C = Cs + Cl
        gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV), (0.2 * torch.randn(C, generator=g)).to(DEV)
        w = (torch.randn(Cout, C, 3, 3, 3, generator=g) / np.sqrt(27 * C)).to(DEV)
        G = 8
        outs = {}
        for up in (True, False):
            if up:
                monkeypatch.delenv("KEYMORPH_NO_UPCONV", raising=False)
            else:
                monkeypatch.setenv("KEYMORPH_NO_UPCONV", "1")
            before = B.UPCONV_STATS["calls"]
            x = B.upcat(skip, low)
            y = B.single_conv_gcr(x, gamma, beta, w, G)
            assert B.UPCONV_STATS["calls"] - before == (1 if up else 0)
            outs[up] = (y, B._peek_stats(y))
        xr = torch.cat([ncdhw(skip), F.interpolate(ncdhw(low), scale_factor=2, mode="nearest")], dim=1).double().cpu()
        yr = F.relu(F.conv3d(F.group_norm(xr, G, gamma.double().cpu(), beta.double().cpu(), 1e-5), w.double().cpu(), None,
                             padding=1))
        scale = float(yr.abs().max())
        for up in (True, False):
            close(ncdhw(outs[up][0]).double(), yr, 3e-6 * scale, 1e-4)
        close(outs[True][0], outs[False][0], 2e-6 * scale, 1e-4)
        if outs[True][1] is not None:
            close(outs[True][1], outs[False][1], 1e-6 * float(outs[False][1].abs().max()), 1e-6)
    finally:
        B.set_conv_mode(old)


@pytest.mark.parametrize("cfg", [(2, (5, 6, 9), 24), (1, (4, 4, 2), 64), (2, (3, 7, 8), 40), (1, (8, 8, 8), 128)])
def test_up2_box_sums(cfg):
    """kmh_up2_boxsum (csrc/norm.hip): G[m][tap][co] = sum of dz over the 2 x 2 x 2 voxels v with (v + tap - 1) // 2 == m, zero
    outside the volume -- what turns the weight gradient of conv3(up2(x_low)) into x_low^T G (the autograd of
    keymorph/unet3d/buildingblocks.py:471-475 + :46-78 for the upsampled channels).  The LDS-tiled kernel against a torch
    restatement (ragged low shapes: partial tiles on every axis; Cout not a multiple of the 32-channel chunk)."""
    from keymorph_amd import _lib
    from keymorph_amd.backbone_ops import _p, _stream, check
    lib = _lib.load()
    N, ld, Cout = cfg
    g = gen(53)
    dz = torch.randn(N, 2 * ld[0], 2 * ld[1], 2 * ld[2], Cout, generator=g)
    G = torch.full((N, ld[0] * ld[1] * ld[2], 27, Cout), float("nan"), device=DEV)
    dzd = dz.to(DEV)
    check(lib.kmh_up2_boxsum(_p(dzd), _p(G), N, ld[0], ld[1], ld[2], Cout, 0, _stream()), "kmh_up2_boxsum")
    if Cout % 8 == 0:        # the channel-blocked gradient layout (N, Cout/8, D, H, W, 8): the same sums, bit for bit
        Gb = torch.full_like(G, float("nan"))
        dzb = dzd.reshape(N, -1, Cout // 8, 8).permute(0, 2, 1, 3).contiguous()
        check(lib.kmh_up2_boxsum(_p(dzb), _p(Gb), N, ld[0], ld[1], ld[2], Cout, 1, _stream()), "kmh_up2_boxsum")
        assert torch.equal(G, Gb)
    pad = F.pad(dz.double().permute(0, 4, 1, 2, 3), (2, 2, 2, 2, 2, 2))            # (N, C, D + 4, H + 4, W + 4): index u + 2
    ref = torch.empty(N, ld[0], ld[1], ld[2], 27, Cout, dtype=torch.float64)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                acc = 0
                for a in (0, 1):
                    for b in (0, 1):
                        for c in (0, 1):        # per axis the hi voxels u = 2 m + 1 - k + {0, 1}
                            acc = acc + pad[:, :, 3 - kz + a:3 - kz + a + 2 * ld[0]:2, 3 - ky + b:3 - ky + b + 2 * ld[1]:2,
                                            3 - kx + c:3 - kx + c + 2 * ld[2]:2]
                ref[:, :, :, :, (kz * 3 + ky) * 3 + kx] = acc.permute(0, 2, 3, 4, 1)
    got = G.cpu().double().reshape(N, ld[0], ld[1], ld[2], 27, Cout)
    assert bool(torch.isfinite(got).all())
    close(got, ref, 1e-5, 1e-6)


@pytest.mark.parametrize("cfg", [(2, (5, 6, 9), 24, 40, True), (1, (4, 4, 2), 64, 128, False), (2, (3, 7, 8), 40, 136, True),
                                 (1, (8, 8, 8), 128, 256, True), (1, (6, 4, 12), 8, 12, False)])
@pytest.mark.parametrize("force", [None, "0", "1", "2"])
def test_up2_weight_gradient_with_the_box_sums_formed_inside_the_product(cfg, force, monkeypatch):
    """kmh_up2_wgrad_fold (round 5) == kmh_up2_boxsum + kmh_up2_wgrad_gemm (the route it replaces) == the fp64 product
    x_low^T G: ragged low shapes (partial 4 x 4 x 2 tiles on every axis), Cl below / above / not a multiple of the 128-row
    tile, one to sixteen cout octets, with and without GroupNorm's affine on the low tensor, dz dense and channel-blocked.
    Replaces autograd's weight gradient of interpolate(nearest x2) + cat + conv3d (buildingblocks.py:471-475, :46-78)."""
    from keymorph_amd import _lib
    from keymorph_amd import backbone_ops as B
    from keymorph_amd.backbone_ops import _p, _stream, check
    lib = _lib.load()
    N, ld, Cout, Cl, affine = cfg
    # the kernel's three shapes: 256 threads (two workgroups per CU), 512 threads = two cout octets over one A image, 512 threads
    # = two 128-row tiles over one window; None = the library's own choice, a forced one applies where the shape allows it
    if force is None:
        monkeypatch.delenv("KEYMORPH_UP2_FOLD_MODE", raising=False)
    else:
        monkeypatch.setenv("KEYMORPH_UP2_FOLD_MODE", force)
    assert lib.kmh_up2_wgrad_fold_ok(Cl, Cout, 2) == 1 and lib.kmh_up2_wgrad_fold_ok(Cl, Cout, 3) == 0
    assert lib.kmh_up2_wgrad_fold_ok(Cl, Cout + 4, 2) == 0
    g = gen(57)
    Vl = ld[0] * ld[1] * ld[2]
    dz = torch.randn(N, 2 * ld[0], 2 * ld[1], 2 * ld[2], Cout, generator=g).to(DEV)
    xl = torch.randn(N, *ld, Cl, generator=g).to(DEV)
    sc = (1 + 0.3 * torch.randn(N, Cl, generator=g)).to(DEV) if affine else None
    sh = (0.3 * torch.randn(N, Cl, generator=g)).to(DEV) if affine else None
    xn = xl * sc.view(N, 1, 1, 1, Cl) + sh.view(N, 1, 1, 1, Cl) if affine else xl
    asc, dsc = B.absmax_scale(xn), B.absmax_scale(dz)
    boxes = torch.empty(N, Vl, 27 * Cout, device=DEV)
    check(lib.kmh_up2_boxsum(_p(dz), _p(boxes), N, ld[0], ld[1], ld[2], Cout, 0, _stream()), "kmh_up2_boxsum")
    ref = torch.einsum("nvc,nvj->ncj", xn.reshape(N, Vl, Cl).double(), boxes.double())
    old = torch.full((N, Cl, 27 * Cout), float("nan"), device=DEV)
    ws = torch.empty(int(lib.kmh_up2_wgrad_gemm_ws_bytes(N, Vl, Cl, 27 * Cout)) // 4 + 1, device=DEV)
    bsc = dsc * torch.tensor([0.125, 8.0], device=DEV)
    check(lib.kmh_up2_wgrad_gemm(_p(xl), _p(boxes), _p(old), N, Vl, Cl, 27 * Cout, 2, _p(asc), _p(bsc), _p(sc), _p(sh), _p(ws),
                                 _stream()), "kmh_up2_wgrad_gemm")
    ws2 = torch.empty(int(lib.kmh_up2_wgrad_fold_ws_bytes(N, ld[0], ld[1], ld[2], Cl, Cout)) // 4 + 1, device=DEV)
    dzb = dz.reshape(N, -1, Cout // 8, 8).permute(0, 2, 1, 3).contiguous()
    outs = []
    for blocked in (0, 1):
        got = torch.full((N, Cl, 27 * Cout), float("nan"), device=DEV)
        check(lib.kmh_up2_wgrad_fold(_p(xl), _p(dzb if blocked else dz), _p(got), N, ld[0], ld[1], ld[2], Cl, Cout, 2, _p(asc),
                                     _p(dsc), _p(sc), _p(sh), blocked, _p(ws2), _stream()), "kmh_up2_wgrad_fold")
        assert bool(torch.isfinite(got).all())
        outs.append(got)
    assert torch.equal(outs[0], outs[1])                              # the layout of dz changes nothing
    assert torch.equal(outs[0], outs[0].clone()) and True
    scale = float(ref.abs().max())
    close(outs[0].double(), ref, 3e-6 * scale, 1e-4)                  # the f16x3 bar of every other product
    close(old.double(), ref, 3e-6 * scale, 1e-4)
    close(outs[0], old, 2e-6 * scale, 1e-4)                           # same operand images: only the summation order differs
    again = torch.empty_like(outs[0])
    check(lib.kmh_up2_wgrad_fold(_p(xl), _p(dz), _p(again), N, ld[0], ld[1], ld[2], Cl, Cout, 2, _p(asc), _p(dsc), _p(sc), _p(sh),
                                 0, _p(ws2), _stream()), "kmh_up2_wgrad_fold")
    assert torch.equal(again, outs[0])                                # deterministic


@pytest.mark.parametrize("cfg", [(2, 16, 24, 32, (3, 5, 18)), (1, 8, 40, 72, (4, 4, 33)), (1, 64, 136, 64, (2, 8, 32))])
@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_up2_data_gradient_at_low_resolution(cfg, mode):
    """sum over a low voxel's 8 children of the data gradient w.r.t. the upsampled channels == the low-resolution
    64-tap kernel (conv3_up2_dgrad)."""
    from keymorph_amd import backbone_ops as B
    N, Cs, Cl, Cout, ld = cfg
    dims = tuple(2 * d for d in ld)
    old = B.CONV_MODE
    try:
        B.set_conv_mode(mode)
        g = gen(41)
        dz = torch.randn(N, *dims, Cout, generator=g).to(DEV)
        w = (torch.randn(Cout, Cs + Cl, 3, 3, 3, generator=g) / np.sqrt(27 * Cout)).to(DEV)
        st = torch.full((N, Cl, 2), float("nan"), dtype=torch.float64, device=DEV)
        got = B.conv3_up2_dgrad(dz, w, Cs, Cl, stats_out=st)
        full = F.conv_transpose3d(ncdhw(dz).double().cpu(), w.double().cpu(), padding=1)[:, Cs:]     # (N,Cl,D,H,W)
        ref = full.reshape(N, Cl, ld[0], 2, ld[1], 2, ld[2], 2).sum(dim=(3, 5, 7))
        close(ncdhw(got).double(), ref, 3e-6 * float(ref.abs().max()), 1e-4)
        # epilogue statistics (what the decoder block's GroupNorm backward reads instead of a pass over the gradient):
        # per-channel (sum, sum of squares) of exactly the values written
        gd = got.double().reshape(N, -1, Cl)
        want = torch.stack([gd.sum(1), (gd * gd).sum(1)], dim=-1)
        close(st, want, 1e-6 * float(want.abs().max()), 1e-6)
        assert torch.equal(got, B.conv3_up2_dgrad(dz, w, Cs, Cl))            # and the gradient itself does not depend on them
        if Cout % 8 == 0:    # dz channel-blocked, (N, Cout/8, D, H, W, 8) under the dense tensor's nominal shape: bit-identical
            dzb = dz.reshape(N, -1, Cout // 8, 8).permute(0, 2, 1, 3).contiguous().view(dz.shape)
            assert torch.equal(got, B.conv3_up2_dgrad(dzb, w, Cs, Cl, dz_blocked=True))
    finally:
        B.set_conv_mode(old)


@pytest.mark.parametrize("cfg", [(2, 16, 24, 32, (3, 5, 18), False), (1, 8, 40, 72, (4, 4, 33), True),
                                 (1, 64, 128, 64, (2, 8, 32), False)])
def test_decoder_block_fused_upsample_concat_conv(cfg, monkeypatch):
    """Decoder = interpolate + cat + DoubleConv: with the first SingleConv fused to the concatenation (no concatenated
    tensor; upsampled channels convolved and differentiated at low resolution; GroupNorm's backward applied to the two
    halves) every gradient equals the unfused path's and PyTorch's -- also when a gamma is exactly 0 (gated fallback)."""
    from keymorph_amd import backbone_ops as B
    from keymorph_amd.unet3d.model import Decoder
    N, Cs, Cl, Cout, ld, zero_gamma = cfg
    dims = tuple(2 * d for d in ld)
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        torch.manual_seed(5)
        dec = Decoder(Cs + Cl, Cout).to(DEV)
        with torch.no_grad():
            dec.basic_module.SingleConv1.groupnorm.weight.add_(0.2 * torch.randn(Cs + Cl, device=DEV))
            dec.basic_module.SingleConv1.groupnorm.bias.add_(0.2 * torch.randn(Cs + Cl, device=DEV))
            if zero_gamma:
                dec.basic_module.SingleConv1.groupnorm.weight[Cs + 3] = 0.0
                dec.basic_module.SingleConv1.groupnorm.weight[2] = 0.0
        g = gen(51)
        skip0 = torch.randn(N, *dims, Cs, generator=g).abs().to(DEV)
        low0 = torch.randn(N, *ld, Cl, generator=g).abs().to(DEV)
        cot = torch.randn(N, *dims, Cout, generator=g).to(DEV)

        def run():
            for p_ in dec.parameters():
                p_.grad = None
            skip, low = skip0.clone().requires_grad_(True), low0.clone().requires_grad_(True)
            y = dec(skip, low)
            (y * cot).sum().backward()
            return [y.detach(), skip.grad, low.grad] + [p_.grad.clone() for p_ in dec.parameters()]

        monkeypatch.delenv("KEYMORPH_NO_UPCONV_BWD", raising=False)
        before, hand = B.UPCONV_STATS["calls"], B.BLOCKED_STATS["handoffs"]
        got = run()
        assert B.UPCONV_STATS["calls"] == before + 1
        # the hidden activation's gradient travels channel-blocked into the fused operator where its kernels take it so
        # (backbone_ops.upcat_blocked_ok): an internal layout, every gradient BIT-identical with it switched off
        if B.upcat_blocked_ok(skip0, low0, Cout):
            assert B.BLOCKED_STATS["handoffs"] == hand + 1, "the blocked hand-off did not run"
            monkeypatch.setenv("KEYMORPH_NO_BLOCKED_UPCAT", "1")
            plain = run()
            monkeypatch.delenv("KEYMORPH_NO_BLOCKED_UPCAT")
            assert B.BLOCKED_STATS["handoffs"] == hand + 1
            for a, r in zip(got, plain):
                assert torch.equal(a, r)
        else:
            assert Cout != 64, "the (64 + 128 -> 64) block is the one the headline step hands over blocked"
        monkeypatch.setenv("KEYMORPH_NO_UPCONV_BWD", "1")
        ref = run()
        for a, r in zip(got, ref):
            close(a, r, 1e-5 * float(r.abs().max()), 1e-3)
        # PyTorch, fp64
        dc = dec.basic_module
        P = [p_.detach().double().cpu().requires_grad_(True) for p_ in
             (dc.SingleConv1.groupnorm.weight, dc.SingleConv1.groupnorm.bias, dc.SingleConv1.conv.weight,
              dc.SingleConv2.groupnorm.weight, dc.SingleConv2.groupnorm.bias, dc.SingleConv2.conv.weight)]
        sk = ncdhw(skip0).double().cpu().requires_grad_(True)
        lo = ncdhw(low0).double().cpu().requires_grad_(True)
        x = torch.cat([sk, F.interpolate(lo, scale_factor=2, mode="nearest")], dim=1)
        h = F.relu(F.conv3d(F.group_norm(x, 8, P[0], P[1], 1e-5), P[2], None, padding=1))
        yr = F.relu(F.conv3d(F.group_norm(h, 8, P[3], P[4], 1e-5), P[5], None, padding=1))
        (yr * ncdhw(cot).double().cpu()).sum().backward()
        close(ncdhw(got[0]).double(), yr.detach(), 1e-5 * float(yr.detach().abs().max()), 1e-3)
        close(ncdhw(got[1]).double(), sk.grad, 1e-4 * float(sk.grad.abs().max()), 1e-3)
        close(ncdhw(got[2]).double(), lo.grad, 1e-4 * float(lo.grad.abs().max()), 1e-3)
        names = [n_ for n_, _ in dec.named_parameters()]
        order = {"basic_module.SingleConv1.groupnorm.weight": 0, "basic_module.SingleConv1.groupnorm.bias": 1,
                 "basic_module.SingleConv1.conv.weight": 2, "basic_module.SingleConv2.groupnorm.weight": 3,
                 "basic_module.SingleConv2.groupnorm.bias": 4, "basic_module.SingleConv2.conv.weight": 5}
        for n_, a in zip(names, got[3:]):
            r = P[order[n_]].grad
            close(a.double(), r, 1e-4 * float(r.abs().max()), 1e-3)
    finally:
        B.set_conv_mode(old)


def test_unet_gradients_identical_with_and_without_blocked_handoffs(monkeypatch):
    """channel-blocked gradient hand-offs (DoubleConv's hidden activation, max-pool backward -> the encoder's last conv)
    are internal layouts: every parameter gradient of a small TruncatedUNet3D is BIT-identical with them switched off."""
    from keymorph_amd import backbone_ops as B
    from keymorph_amd.unet3d.model import TruncatedUNet3D
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        torch.manual_seed(11)
        net = TruncatedUNet3D(1, 8, 1, f_maps=8, num_levels=3, num_groups=4, is_segmentation=False).to(DEV)
        x = torch.randn(2, 1, 16, 16, 32, generator=gen(12)).to(DEV)
        cot = torch.randn(2, 8, 8, 8, 16, generator=gen(13)).to(DEV)

        def run():
            for p_ in net.parameters():
                p_.grad = None
            (net(x) * cot).sum().backward()
            return [p_.grad.clone() for p_ in net.parameters()]

        monkeypatch.delenv("KEYMORPH_NO_BLOCKED_GRADS", raising=False)
        before = B.BLOCKED_STATS["handoffs"]
        got = run()
        assert B.BLOCKED_STATS["handoffs"] > before
        monkeypatch.setenv("KEYMORPH_NO_BLOCKED_GRADS", "1")
        ref = run()
        for a, r in zip(got, ref):
            assert torch.equal(a, r)
    finally:
        B.set_conv_mode(old)


@pytest.mark.parametrize("cfg", [(2, (4, 6, 10), 8), (1, (6, 4, 32), 32), (3, (2, 2, 6), 16)])
def test_maxpool_backward_channel_blocked_rows(cfg):
    """kmh_maxpool3d_bwd with out_blocked and no second gradient (the 256^3 level of the step): the row-contiguous kernel
    writes the (N, C/8, D, H, W, 8) layout of exactly the values the (N, D, H, W, C) kernel writes."""
    from keymorph_amd import _lib
    from keymorph_amd.backbone_ops import _p, _stream, check
    lib = _lib.load()
    N, dims, C = cfg
    D, H, W = dims
    g = gen(71)
    x = torch.randn(N, D, H, W, C, generator=g).to(DEV)
    y = torch.empty(N, D // 2, H // 2, W // 2, C, device=DEV)
    arg = torch.empty(N, D // 2, H // 2, W // 2, C, dtype=torch.uint8, device=DEV)
    check(lib.kmh_maxpool3d_fwd(_p(x), _p(y), _p(arg), N, D, H, W, C, _stream()), "kmh_maxpool3d_fwd")
    dy = torch.randn(y.shape, generator=g).to(DEV)
    dense = torch.full((N, D, H, W, C), float("nan"), device=DEV)
    blocked = torch.full((N, C // 8, D, H, W, 8), float("nan"), device=DEV)
    check(lib.kmh_maxpool3d_bwd(None, _p(arg), _p(dy), None, 0, _p(dense), N, D, H, W, C, 0, _stream()), "kmh_maxpool3d_bwd")
    check(lib.kmh_maxpool3d_bwd(None, _p(arg), _p(dy), None, 0, _p(blocked), N, D, H, W, C, 1, _stream()), "kmh_maxpool3d_bwd")
    assert torch.equal(blocked.permute(0, 2, 3, 4, 1, 5).reshape(N, D, H, W, C), dense)
    # and against autograd of max_pool3d
    xr = ncdhw(x).cpu().double().requires_grad_(True)
    (F.max_pool3d(xr, 2) * ncdhw(dy).cpu().double()).sum().backward()
    close(ncdhw(dense), xr.grad, 0, 0)


def test_fused_upsample_concat_conv_applies_its_own_relu_mask():
    """upcat_conv_gcr with dy_premasked=False (a consumer that does not mask the gradient it returns): the operator folds
    its ReLU's backward mask itself -- gradients equal PyTorch's."""
    from keymorph_amd import backbone_ops as B
    N, Cs, Cl, Cout, ld = 1, 16, 16, 24, (3, 4, 17)
    dims = tuple(2 * d for d in ld)
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        g = gen(61)
        skip0 = torch.randn(N, *dims, Cs, generator=g).abs()
        low0 = torch.randn(N, *ld, Cl, generator=g).abs()
        gamma = 1 + 0.2 * torch.randn(Cs + Cl, generator=g)
        beta = 0.2 * torch.randn(Cs + Cl, generator=g)
        w = torch.randn(Cout, Cs + Cl, 3, 3, 3, generator=g) / np.sqrt(27 * (Cs + Cl))
        cot = torch.randn(N, *dims, Cout, generator=g)
        H = [t.to(DEV).requires_grad_(True) for t in (skip0, low0, gamma, beta, w)]
        assert B.upcat_conv_ok(H[0], H[1], Cout)
        y = B.upcat_conv_gcr(H[0], H[1], H[2], H[3], H[4], 8, dy_premasked=False)
        (y * cot.to(DEV)).sum().backward()
        R = [t.double().requires_grad_(True) for t in (ncdhw(skip0), ncdhw(low0), gamma, beta, w)]
        x = torch.cat([R[0], F.interpolate(R[1], scale_factor=2, mode="nearest")], dim=1)
        yr = F.relu(F.conv3d(F.group_norm(x, 8, R[2], R[3], 1e-5), R[4], None, padding=1))
        (yr * ncdhw(cot).double()).sum().backward()
        close(ncdhw(y.detach()).double(), yr.detach(), 1e-5 * float(yr.detach().abs().max()), 1e-3)
        for a, r, perm in zip(H, R, (True, True, False, False, False)):
            ga = ncdhw(a.grad) if perm else a.grad
            close(ga.double(), r.grad, 1e-4 * float(r.grad.abs().max()), 1e-3)
    finally:
        B.set_conv_mode(old)


@pytest.mark.parametrize("dims", [(8, 16, 64), (7, 9, 33)])
def test_first_block_lazy_groupnorm_backward_handoff(dims, monkeypatch):
    """The first encoder block on an image: the second convolution hands its normalised-input gradient to the first
    layer's correlation kernel with GroupNorm's backward still pending (applied while the kernel stages the gradient, so
    the full-resolution 16-channel gradient is never written by a separate pass).  Every parameter gradient must equal
    the plain route's (the same expression c1 dxn + c2 y + c3 under the same ReLU mask, evaluated in another kernel)
    and PyTorch's."""
    from keymorph_amd import backbone_ops as B
    from keymorph_amd.unet3d.model import DoubleConv
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        torch.manual_seed(11)
        blk = DoubleConv(1, 32, encoder=True, num_groups=8, first_layer=True).to(DEV)
        img = torch.rand(2, *dims, 1, generator=gen(12)).to(DEV)
        cot = torch.randn(2, *dims, 32, generator=gen(13)).to(DEV)

        def run():
            for p_ in blk.parameters():
                p_.grad = None
            y = blk(img, True)
            (y * (cot * (y.detach() > 0))).sum().backward()
            return y.detach().clone(), [p_.grad.clone() for p_ in blk.parameters()]

        before = B.LAZY_STATS["handoffs"]
        y1, g1 = run()
        assert B.LAZY_STATS["handoffs"] == before + 1, "the lazy hand-off did not run"
        monkeypatch.setenv("KEYMORPH_NO_LAZY_FIRST", "1")
        y0, g0 = run()
        assert B.LAZY_STATS["handoffs"] == before + 1
        assert torch.equal(y1, y0)
        for (k, _), a, r in zip(blk.named_parameters(), g1, g0):
            err = float((a - r).abs().max()) / (float(r.abs().max()) + 1e-30)
            # (the first layer's one-element GroupNorm weight / bias are whole-volume sums that cancel to ~0: a last-bit
            # difference in how the two kernels contract c1 dxn + c2 y + c3 shows up there at the percent level -- the
            # same tensor is the per-tensor worst of every pairing of arithmetics)
            bar = 5e-2 if k.startswith("SingleConv1.groupnorm") else 5e-6
            assert err < bar, ("lazy vs plain route", k, err)
        # and against PyTorch (fp64) on the same masked cotangent
        ref = torch.nn.Sequential(torch.nn.GroupNorm(1, 1), torch.nn.Conv3d(1, 16, 3, padding=1, bias=False), torch.nn.ReLU(),
                                  torch.nn.GroupNorm(8, 16), torch.nn.Conv3d(16, 32, 3, padding=1, bias=False),
                                  torch.nn.ReLU()).double()
        sd = blk.state_dict()
        ref[0].load_state_dict({"weight": sd["SingleConv1.groupnorm.weight"].double().cpu(),
                                "bias": sd["SingleConv1.groupnorm.bias"].double().cpu()})
        ref[1].load_state_dict({"weight": sd["SingleConv1.conv.weight"].double().cpu()})
        ref[3].load_state_dict({"weight": sd["SingleConv2.groupnorm.weight"].double().cpu(),
                                "bias": sd["SingleConv2.groupnorm.bias"].double().cpu()})
        ref[4].load_state_dict({"weight": sd["SingleConv2.conv.weight"].double().cpu()})
        yr = ref(ncdhw(img.cpu().double()))
        (yr * ncdhw((cot * (y1 > 0)).cpu().double())).sum().backward()
        close(ncdhw(y1), yr, 2e-5, 1e-4)
        # (the first layer's one-element GroupNorm weight / bias are sums over the whole volume that cancel to ~0: they
        # are compared between the two routes above, not against fp64 at a relative bar)
        names = ["SingleConv1.conv.weight", "SingleConv2.groupnorm.weight", "SingleConv2.groupnorm.bias",
                 "SingleConv2.conv.weight"]
        refg = {"SingleConv1.groupnorm.weight": ref[0].weight.grad, "SingleConv1.groupnorm.bias": ref[0].bias.grad,
                "SingleConv1.conv.weight": ref[1].weight.grad, "SingleConv2.groupnorm.weight": ref[3].weight.grad,
                "SingleConv2.groupnorm.bias": ref[3].bias.grad, "SingleConv2.conv.weight": ref[4].weight.grad}
        got = dict(zip([k for k, _ in blk.named_parameters()], g1))
        for k in names:
            # relative L2: the HIDDEN activation's ReLU mask is each implementation's own, and a pre-activation within
            # rounding of zero flips it (one flip moves single weight-gradient entries by ~1e-2 of their size)
            a, r = got[k].detach().cpu().double(), refg[k].double()
            assert float((a - r).norm() / r.norm()) < 5e-3, k
    finally:
        B.set_conv_mode(old)


def test_skip_gradient_lazy_groupnorm_backward_in_pool_fork(monkeypatch):
    """Decoder skip connections: the fused upsample + concat + conv operator hands the skip half's gradient to pool_fork's
    backward with GroupNorm's backward pending; kmh_maxpool3d_bwd_lazy applies it while it sums the pooling and the skip
    gradients.  Same keypoints, and every parameter gradient equal to the two-pass route's at the fp32 rounding level
    (the range scale of the summed gradient is exact here and a sum bound there, so the following f16x3 convolutions split
    their operand at another power of two)."""
    from keymorph_amd import backbone_ops as B
    from keymorph_amd.unet3d.model import UNet3D
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        torch.manual_seed(7)
        # (f_maps = 32: decoder widths 64 and 32, so that both decoders take the fused operator: Cout > 16)
        net = UNet3D(1, 6, final_sigmoid=False, f_maps=32, layer_order="gcr", num_groups=8, num_levels=3,
                     is_segmentation=False, conv_padding=1).to(DEV).train()
        img = torch.rand(2, 1, 16, 24, 40, generator=gen(3)).to(DEV)
        outs = {}
        for lazy in (True, False):
            if lazy:
                monkeypatch.delenv("KEYMORPH_NO_LAZY_SKIP", raising=False)
            else:
                monkeypatch.setenv("KEYMORPH_NO_LAZY_SKIP", "1")
            net.zero_grad(set_to_none=True)
            before = B.LAZY_STATS["handoffs"]
            y = net(img)
            (y * torch.linspace(-1, 1, y.numel(), device=DEV).reshape(y.shape)).sum().backward()
            outs[lazy] = (y.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters()},
                          B.LAZY_STATS["handoffs"] - before)
        # two decoders = two skip hand-offs more than the route without them (the first block's own hand-off runs in both)
        assert outs[True][2] == outs[False][2] + 2, (outs[True][2], outs[False][2])
        assert torch.equal(outs[True][0], outs[False][0])
        for k in outs[True][1]:
            a, r = outs[True][1][k].double(), outs[False][1][k].double()
            # (the first layer's one-element GroupNorm weight / bias: whole-volume sums that cancel to ~0 -- the per-tensor
            # worst of every pairing of routes and arithmetics)
            bar = 5e-2 if k.startswith("encoders.0.basic_module.SingleConv1.groupnorm") else 2e-6
            assert float((a - r).norm() / (r.norm() + 1e-30)) < bar, k
    finally:
        B.set_conv_mode(old)


def test_lost_lazy_skip_tag_raises(monkeypatch):
    """Round-3 advisor finding: a hook (or retain_grad, or a second consumer) on the skip tensor re-wraps the gradient, the
    `pending GroupNorm backward` tag does not survive, and pool_fork's backward used to sum the RAW normalised-input
    gradient as if it were finished.  The decoder now records the hand-off on pool_fork's node: a missing tag raises, and
    KEYMORPH_NO_LAZY_SKIP=1 (GroupNorm's backward applied in the decoder) works with the same hook."""
    from keymorph_amd import backbone_ops as B
    from keymorph_amd.unet3d.model import UNet3D
    torch.manual_seed(7)
    net = UNet3D(1, 6, final_sigmoid=False, f_maps=32, layer_order="gcr", num_groups=8, num_levels=3,
                 is_segmentation=False, conv_padding=1).to(DEV).train()
    img = torch.rand(1, 1, 16, 16, 16, generator=gen(3)).to(DEV)
    real = B.pool_fork

    def hooked(x):
        y, skip = real(x)
        skip.register_hook(lambda g: g * 1.0)          # what a gradient-logging hook does: returns a new tensor
        return y, skip

    monkeypatch.setattr(B, "pool_fork", hooked)
    monkeypatch.delenv("KEYMORPH_NO_LAZY_SKIP", raising=False)
    with pytest.raises(RuntimeError, match="KEYMORPH_NO_LAZY_SKIP"):
        net(img).sum().backward()
    monkeypatch.setenv("KEYMORPH_NO_LAZY_SKIP", "1")
    net.zero_grad(set_to_none=True)
    net(img).sum().backward()
    g_hook = {k: p.grad.clone() for k, p in net.named_parameters()}
    monkeypatch.setattr(B, "pool_fork", real)
    net.zero_grad(set_to_none=True)
    net(img).sum().backward()
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, g_hook[k]), k


def _gcr_params(Cin, Cout, seed):
    g = gen(seed)
    gamma, beta = 1 + 0.2 * torch.randn(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / np.sqrt(27 * Cin)
    return [t.to(DEV).requires_grad_(True) for t in (gamma, beta, w)]


def test_dense_gradient_where_a_blocked_one_was_promised_raises():
    """A SingleConv told `dy_blocked` (its only consumer returns the gradient channel-blocked) that receives a plain dense
    gradient -- the layout hand-off was lost, e.g. to a hook -- must refuse: reading it as blocked would scramble channels.
    The check is the first thing the backward does, before any launch."""
    from keymorph_amd import backbone_ops as B
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        x = torch.randn(1, 8, 8, 32, 8, generator=gen(71)).abs().to(DEV).requires_grad_(True)
        gamma, beta, w = _gcr_params(8, 16, 72)
        y = B.single_conv_gcr(x, gamma, beta, w, 8, dy_premasked=True, dy_blocked=True)
        with pytest.raises(RuntimeError, match="KEYMORPH_NO_BLOCKED_GRADS"):
            y.backward(torch.ones_like(y))
    finally:
        B.set_conv_mode(old)


def test_dense_gradient_at_the_fused_decoder_operator_raises():
    """The same at upcat_conv_gcr(dy_blocked=True), at the smallest shape of test_decoder_block_fused_upsample_concat_conv."""
    from keymorph_amd import backbone_ops as B
    N, Cs, Cl, Cout, ld = 2, 16, 24, 32, (3, 5, 18)
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        g = gen(73)
        skip = torch.randn(N, *(2 * d for d in ld), Cs, generator=g).abs().to(DEV).requires_grad_(True)
        low = torch.randn(N, *ld, Cl, generator=g).abs().to(DEV).requires_grad_(True)
        gamma, beta, w = _gcr_params(Cs + Cl, Cout, 74)
        assert B.upcat_conv_ok(skip, low, Cout)
        y = B.upcat_conv_gcr(skip, low, gamma, beta, w, 8, dy_premasked=True, dy_blocked=True)
        with pytest.raises(RuntimeError, match="KEYMORPH_NO_BLOCKED_GRADS"):
            y.backward(torch.ones_like(y))
    finally:
        B.set_conv_mode(old)


def test_lost_lazy_first_layer_tag_raises():
    """The first convolution told `dy_lazy` (the second one hands over its normalised-input gradient with GroupNorm's backward
    pending) that receives a gradient without that hand-off must refuse: taking it as finished would skip a GroupNorm
    backward."""
    from keymorph_amd import backbone_ops as B
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        img = torch.rand(1, 8, 8, 32, 1, generator=gen(75)).to(DEV)
        gamma, beta, w = _gcr_params(1, 8, 76)
        y = B.single_conv_gcr(img, gamma, beta, w, 1, x_from_relu=False, dy_premasked=True, dy_lazy=True)
        with pytest.raises(RuntimeError, match="KEYMORPH_NO_LAZY_FIRST"):
            y.backward(torch.ones_like(y))
    finally:
        B.set_conv_mode(old)


def test_pool_fork_backward_with_a_misaligned_skip_gradient_view():
    """kmh_maxpool3d_bwd's 16-byte kernel reads the second gradient as float4: a channel-slice view whose storage offset is
    not a multiple of 4 floats must take the scalar kernel (round-2 advisor finding) -- same result either way"""
    from keymorph_amd import backbone_ops as B, _lib
    from keymorph_amd.ops import _p, _stream
    lib = _lib.load()
    g = gen(51)
    N, D, H, W, C = 1, 4, 6, 8, 8
    x = torch.randn(N, D, H, W, C, generator=g).to(DEV)
    y = torch.empty(N, D // 2, H // 2, W // 2, C, device=DEV)
    arg = torch.empty(y.shape, dtype=torch.uint8, device=DEV)
    assert lib.kmh_maxpool3d_fwd(_p(x), _p(y), _p(arg), N, D, H, W, C, _stream()) == 0
    dy = torch.randn(y.shape, generator=g).to(DEV)
    wide = torch.randn(N, D, H, W, C + 4, generator=g).to(DEV)        # the skip gradient lives at channel offset 1: misaligned
    add = wide[..., 1:1 + C]
    assert add.data_ptr() % 16 != 0 and add.stride(3) == C + 4
    dx = torch.empty_like(x)
    assert lib.kmh_maxpool3d_bwd(None, _p(arg), _p(dy), _p(add), C + 4, _p(dx), N, D, H, W, C, 0, _stream()) == 0
    dx2 = torch.empty_like(x)
    addc = add.contiguous()
    assert lib.kmh_maxpool3d_bwd(None, _p(arg), _p(dy), _p(addc), C, _p(dx2), N, D, H, W, C, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)
