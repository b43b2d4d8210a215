"""GPU: the "pooled + winners" gradient hand-off (layout kind 3).

The gradient of a convolution whose output feeds only a 2 x 2 x 2 max-pool has one non-zero per window and channel.  Instead of
scattering it into pre-split records (kmh_maxpool3d_bwd_split, kind 2) the backward hands the POOLED gradient and the winner
bytes to both consumers -- the z-paired data gradient (conv3_fwd_s_kernel<1, true, true, .., SPARSE>) and the wave-specialised
weight gradient (conv3_wgrad_ws_kernel<.., DSPARSE>) -- which build in their own staging the words the records would give them.
Everything here is a bit-for-bit comparison against the kind-2 route, which stays as the fall-back and the reference arm."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_dispatch_gpu import _pool_bwd_pair, conv3_fp64, dispatch, gen, group_norm_fp64, rel  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"

OP_SHAPES = [(2, (12, 16, 64), 16, 32), (2, (44, 60, 100), 16, 32), (1, (30, 62, 122), 8, 24)]


def _evict():
    torch.empty(64 << 20, device=DEV).normal_()          # 256 MB: nothing of the last launch stays in the caches


@pytest.mark.parametrize("N,shape,Cin,Cout", [(2, (8, 16, 64), 32, 16),       # 2 x 2 x 2 bricks
                                              (1, (12, 20, 34), 32, 16),      # partial bricks, cells cut by the volume edge
                                              (3, (6, 10, 70), 16, 8),
                                              (1, (4, 8, 32), 64, 16),        # one brick, 8 chunks
                                              (2, (44, 60, 100), 32, 16)])    # more bricks than workgroups: the persistent loop
def test_sparse_data_gradient_is_bit_identical_to_the_presplit_records(N, shape, Cin, Cout, dispatch):
    from keymorph_amd import _lib, backbone_ops as B
    from keymorph_amd.ops import _p, _stream, check
    lib = _lib.load()
    B.set_conv_mode("f16x3")
    D, H, W = shape
    V = D * H * W
    dy, arg, sc = _pool_bwd_pair(N, shape, Cin, 7)
    w = (torch.randn(Cin, Cout, 3, 3, 3, generator=gen(8)) * 0.05).to(DEV)
    pk = B.pack_weight(w, True)
    rec = torch.empty((N, Cin // 8, V + 1, 8), device=DEV)
    check(lib.kmh_maxpool3d_bwd_split(_p(arg), _p(dy), _p(sc), _p(rec), N, D, H, W, Cin, _stream()), "bwd split")
    dispatch(2)
    assert lib.kmh_conv3d_fwd_bf_sparse_ok(N, D, H, W, Cin, Cout, 2) == 1
    st2 = torch.empty((N, Cout, 2), dtype=torch.float64, device=DEV)
    y2 = B.conv3_raw(rec, None, None, pk, None, N, D, H, W, Cin, Cout, False, False, ascale=sc, in_blocked=2, stats_out=st2)

    def sparse():
        st = torch.full((N, Cout, 2), float("nan"), dtype=torch.float64, device=DEV)
        y = B.conv3_raw(dy, None, None, pk, None, N, D, H, W, Cin, Cout, False, False, ascale=sc, in_blocked=3, stats_out=st,
                        winners=arg)
        return y, st

    y3, st3 = sparse()
    assert torch.isfinite(y3).all() and float(y3.abs().max()) > 0
    assert torch.equal(y3, y2), float((y3 - y2).abs().max())
    assert torch.equal(st3, st2)
    for _ in range(3):
        _evict()
        ya, sta = sparse()
        assert torch.equal(ya, y3) and torch.equal(sta, st3)


@pytest.mark.parametrize("N,shape,Cin,Cout", OP_SHAPES)
def test_sparse_weight_gradient_is_bit_identical_to_the_presplit_records(N, shape, Cin, Cout, dispatch):
    from keymorph_amd import _lib, backbone_ops as B
    from keymorph_amd.ops import _p, _stream, check
    lib = _lib.load()
    B.set_conv_mode("f16x3")
    D, H, W = shape
    V = D * H * W
    dy, arg, sc = _pool_bwd_pair(N, shape, Cout, 11)
    g = gen(12)
    x = torch.randn(N, D, H, W, Cin, generator=g).to(DEV)
    scale = (1 + 0.2 * torch.randn(N, Cin, generator=g)).to(DEV)
    shift = (0.2 * torch.randn(N, Cin, generator=g)).to(DEV)
    xs = B.absmax_scale(x * scale.view(N, 1, 1, 1, Cin) + shift.view(N, 1, 1, 1, Cin))      # the NORMALISED input's range scale
    rec = torch.empty((N, Cout // 8, V + 1, 8), device=DEV)
    check(lib.kmh_maxpool3d_bwd_split(_p(arg), _p(dy), _p(sc), _p(rec), N, D, H, W, Cout, _stream()), "bwd split")
    assert lib.kmh_conv3d_wgrad_bf_sparse_ok(N, D, H, W, Cin, Cout, 2) == 1
    d2 = B.conv3_wgrad(x, scale, shift, rec, N, D, H, W, Cin, Cout, False, xscale=xs, dscale=sc, dz_blocked=2)
    d3 = B.conv3_wgrad(x, scale, shift, dy, N, D, H, W, Cin, Cout, False, xscale=xs, dscale=sc, dz_blocked=3, winners=arg)
    assert torch.isfinite(d3).all() and float(d3.abs().max()) > 0
    assert torch.equal(d3, d2), float((d3 - d2).abs().max())


_REF64 = {}


def _op_inputs(cfg):
    N, (D, H, W), Cin, Cout = cfg
    g = gen(600 + Cin)
    x = torch.randn(N, D, H, W, Cin, generator=g).abs() + 0.1 * torch.randn(N, D, H, W, Cin, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / np.sqrt(27 * Cin)
    cot = torch.randn(N, D // 2, H // 2, W // 2, Cout, generator=g)
    return x, gamma, beta, w, cot


def _ref64(cfg, G):
    """fp64 autograd of keymorph/unet3d/buildingblocks.py:46-78 + max_pool3d: (dx, dw), computed once per shape"""
    if cfg not in _REF64:
        x, gamma, beta, w, cot = _op_inputs(cfg)
        R = [t.double().requires_grad_(True) for t in (x, gamma, beta, w)]
        y64 = torch.relu(conv3_fp64(group_norm_fp64(R[0], G, R[1], R[2]), R[3]))
        p64 = F.max_pool3d(y64.permute(0, 4, 1, 2, 3), 2).permute(0, 2, 3, 4, 1)
        (p64 * (cot.double() * (p64.detach() > 0))).sum().backward()
        _REF64[cfg] = (R[0].grad, R[3].grad)
    return _REF64[cfg]


def _run_op(B, monkeypatch, tensors, cot, G, sparse, **kw):
    """-> (pooled output, the four gradients, increments of SPARSE_STATS and SPLIT_STATS)"""
    if sparse:
        monkeypatch.delenv("KEYMORPH_NO_SPARSE_POOLGRAD", raising=False)
    else:
        monkeypatch.setenv("KEYMORPH_NO_SPARSE_POOLGRAD", "1")
    Hh = [t.clone().requires_grad_(True) for t in tensors]
    b_sparse, b_split = B.SPARSE_STATS["handoffs"], B.SPLIT_STATS["handoffs"]
    yp = B.single_conv_gcr(*Hh, G, x_from_relu=False, dy_premasked=True, pool=True, **{"dy_blocked": True, **kw})
    (yp * (cot * (yp.detach() > 0))).sum().backward()
    return (yp.detach(), [t.grad for t in Hh], B.SPARSE_STATS["handoffs"] - b_sparse, B.SPLIT_STATS["handoffs"] - b_split)


@pytest.mark.parametrize("cfg", OP_SHAPES)
def test_conv_pool_backward_with_the_pooled_operand_equals_the_presplit_scatter(cfg, dispatch, monkeypatch):
    """single_conv_gcr(pool=True) backward, default (pooled + winners) against KEYMORPH_NO_SPARSE_POOLGRAD=1 (pre-split records):
    all four gradients bit for bit; against fp64 autograd with the pre-split test's bars (5e-6 on the weights, 2e-5 on x)."""
    from keymorph_amd import backbone_ops as B
    N, (D, H, W), Cin, Cout = cfg
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        dispatch(2)
        assert B.conv_pool_ok(N, D, H, W, Cin, Cout) and B.pool_grad_sparse_ok(N, D, H, W, Cin, Cout)
        x, gamma, beta, w, cot = (t.to(DEV) for t in _op_inputs(cfg))
        G = 8
        y3, g3, sp3, sl3 = _run_op(B, monkeypatch, (x, gamma, beta, w), cot, G, True)
        y2, g2, sp2, sl2 = _run_op(B, monkeypatch, (x, gamma, beta, w), cot, G, False)
        assert (sp3, sl3) == (1, 1) and (sp2, sl2) == (0, 1)
        assert torch.equal(y3, y2)
        for name, a, b in zip(("x", "gamma", "beta", "w"), g3, g2):
            assert torch.isfinite(a).all() and torch.equal(a, b), (name, float((a - b).abs().max()))
        dx64, dw64 = _ref64(cfg, G)
        ew, ex = rel(g3[3].cpu(), dw64), rel(g3[0].cpu(), dx64)
        print("fp64: dw", ew, "dx", ex)
        assert ew < 5e-6 and ex < 2e-5
    finally:
        B.set_conv_mode(old)


@pytest.mark.parametrize("case", ["odd", "cout20", "bf16x6_dgrad", "amp"])
def test_pooled_operand_is_refused_where_it_is_not_served_and_the_backward_still_runs(case, dispatch, monkeypatch):
    from keymorph_amd import backbone_ops as B
    N, Cin, Cout, dims, kw = 1, 16, 32, (8, 16, 64), {}
    if case == "odd":
        dims, kw = (9, 16, 64), {"dy_blocked": False}      # (an odd volume's gradient is not handed over channel-blocked)
    elif case == "cout20":
        Cout, kw = 20, {"dy_blocked": False}                # (nor is one with a partial 8-channel chunk: grad_blocked_ok)
    elif case == "bf16x6_dgrad":
        kw = {"dgrad_terms": 3}
    D, H, W = dims
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        dispatch(2)
        assert B.conv_pool_ok(N, D, H, W, Cin, Cout)
        g = gen(77)
        x = torch.randn(N, D, H, W, Cin, generator=g).abs().to(DEV)
        gamma, beta = (1 + 0.2 * torch.randn(Cin, generator=g)).to(DEV), (0.2 * torch.randn(Cin, generator=g)).to(DEV)
        w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) / np.sqrt(27 * Cin)).to(DEV)
        cot = torch.randn(N, D // 2, H // 2, W // 2, Cout, generator=g).to(DEV)
        with B.amp_scope(case == "amp"):
            if case != "bf16x6_dgrad":      # (the selector is an argument of the operator, not of the shape's predicate)
                assert not B.pool_grad_sparse_ok(N, D, H, W, Cin, Cout)
            ya, ga, spa, _ = _run_op(B, monkeypatch, (x, gamma, beta, w), cot, 8, True, **kw)
            yb, gb, spb, _ = _run_op(B, monkeypatch, (x, gamma, beta, w), cot, 8, False, **kw)
        assert spa == 0 and spb == 0
        assert torch.equal(ya, yb)
        for a, b in zip(ga, gb):
            assert torch.isfinite(a).all() and float(a.abs().max()) > 0 and torch.equal(a, b)
        B.set_conv_mode("bf16x6")
        assert not B.pool_grad_sparse_ok(1, 8, 16, 64, 16, 32)
    finally:
        B.set_conv_mode(old)


def test_pooled_operand_predicate_answers_for_the_shape(dispatch):
    """No allocation: the headline shape is served in f16x3 mode, whatever the forward dispatch mode."""
    from keymorph_amd import _lib, backbone_ops as B
    lib = _lib.load()
    old = B.CONV_MODE
    try:
        B.set_conv_mode("f16x3")
        for mode in (0, 1, 2):
            dispatch(mode)
            assert B.pool_grad_sparse_ok(4, 256, 256, 256, 16, 32)
            assert lib.kmh_conv3d_fwd_bf_sparse_ok(4, 256, 256, 256, 32, 16, 2) == 1
            assert lib.kmh_conv3d_wgrad_bf_sparse_ok(4, 256, 256, 256, 16, 32, 2) == 1
            assert lib.kmh_conv3d_fwd_bf_sparse_ok(4, 256, 256, 256, 32, 16, 1) == 0      # use_amp: not served
            assert lib.kmh_conv3d_fwd_bf_sparse_ok(1, 9, 16, 64, 32, 16, 2) == 0
    finally:
        B.set_conv_mode(old)
