"""GPU: csrc/pointwise.hip (the fp32-MFMA 1x1x1 head convolution: pack, forward, data gradient, weight / bias gradient) against the
fp64 restatement of tests/pointwise_ref.py at the sizes where its tiling changes path -- 128-voxel workgroup tiles, 32-wide MFMA
tiles, 64-channel LDS chunks, 128-wide Cout groups, 64-channel weight-gradient launches with an NT = 1 tail, slabs reduced in
double -- and the model's dispatch on the head width that sends every final conv above 64 input channels here.
tests/test_pointwise_reference_cpu.py pins the restatement.

Two arms per case (pointwise_ref's docstring): integer data whose fp32 sums are exact in any order -- BIT EQUALITY with the float32
cast of the fp64 result -- and real data with compensating channel scales under the derived bars (u = 2^-24): (K + 3) u sum|a b|
with K = Cin (forward, the bias one more term), Cout (data gradient), the longest one-slab chain (weight and bias gradient, from
the library's own slab count), + u |dw0 + dw| with accumulate = 1.  Each test prints error and bar; the docstrings carry the worst
ratio error / bar observed on gfx950 (MI355X)."""
import numpy as np
import pytest
import torch

from tests import pointwise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64              # floats of sentinel on either side of every output: a store outside the tensor shows


def _B():
    from keymorph_amd import backbone_ops as B
    return B


def _L():
    from keymorph_amd import _lib
    from keymorph_amd.ops import _p, _stream
    return _lib.load(), _lib.check, _p, _stream, _lib.KeymorphHipError


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)       # a copy: the cases are read-only


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {np.argwhere(bad)[0]}"


def _check(tag, got, truth, bar, quiet=False):
    """|got - truth| <= bar element by element; -> worst error / bar"""
    got, truth, bar = np.asarray(got, np.float64), np.asarray(truth, np.float64), np.broadcast_to(bar, np.shape(truth))
    assert got.shape == truth.shape, (tag, got.shape, truth.shape)
    err = np.abs(got - truth)
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))
    if not quiet:
        print(f"{tag}: error {float(err.max(initial=0.0)):.3e}, bar {float(bar.max(initial=0.0)):.3e}, worst error / bar {ratio:.3f}")
    assert np.isfinite(got).all() and ratio <= 1.0, f"{tag}: worst error / bar {ratio:.3f}"
    return ratio


class _Out:
    """an output tensor between two guards, pre-filled (NaN: an element the kernel leaves out shows in either arm)"""

    def __init__(self, shape, fill=None):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * GUARD,), -7.25, dtype=torch.float32, device=DEV)
        self.t = self.whole[GUARD:GUARD + n].view(shape)
        self.t.copy_(torch.full(shape, float("nan"), device=DEV) if fill is None else _dev(fill))

    def get(self, tag):
        w = _np(self.whole)
        assert (w[:GUARD] == -7.25).all() and (w[-GUARD:] == -7.25).all(), f"{tag}: a store outside the tensor"
        return w[GUARD:-GUARD].reshape(tuple(self.t.shape)).copy()


def _nslab(row):
    lib = _L()[0]
    N, V, Cin, Cout = row
    nbytes, per = int(lib.kmh_pointwise_wgrad_ws_bytes(N, V, Cin, Cout)), (Cout * Cin + Cout) * 4
    assert nbytes > 0 and nbytes % per == 0, (row, nbytes, per)
    return nbytes // per


def _run(row, c, bias=True, dbias=True, accumulate=0):
    """pack, forward, data gradient, weight gradient through the C ABI -> dict of float32 arrays (db None without dbias)"""
    lib, check, _p, _stream, _ = _L()
    N, V, Cin, Cout = row
    x, w, dy = _dev(c["x"]), _dev(c["w"]), _dev(c["dy"])
    b = _dev(c["b"]) if bias else None
    wt, y, dx = _Out((Cin, Cout)), _Out((N, Cout, V)), _Out((N, V, Cin))
    dw = _Out((Cout, Cin), c["dw0"] if accumulate else None)
    db = _Out((Cout,), c["db0"] if accumulate else None) if dbias else None
    ws = torch.empty(int(lib.kmh_pointwise_wgrad_ws_bytes(N, V, Cin, Cout)), dtype=torch.uint8, device=DEV)
    check(lib.kmh_pointwise_pack(_p(w), _p(wt.t), Cout, Cin, _stream()), "kmh_pointwise_pack")
    check(lib.kmh_pointwise_fwd(_p(x), _p(wt.t), _p(b), _p(y.t), N, V, Cin, Cout, _stream()), "kmh_pointwise_fwd")
    check(lib.kmh_pointwise_dgrad(_p(dy), _p(w), _p(dx.t), N, V, Cin, Cout, _stream()), "kmh_pointwise_dgrad")
    check(lib.kmh_pointwise_wgrad(_p(dy), _p(x), _p(dw.t), None if db is None else _p(db.t), N, V, Cin, Cout, accumulate, _p(ws),
                                  _stream()), "kmh_pointwise_wgrad")
    torch.cuda.synchronize()
    return {"wt": wt.get("wt"), "y": y.get("y"), "dx": dx.get("dx"), "dw": dw.get("dw"), "db": None if db is None else db.get("db")}


def _truth(row, c, bias=True, accumulate=0, dbias=True):
    """fp64 results and bars of one case: name -> (truth, bar)"""
    b = c["b"] if bias else None
    dw, db = R.wgrad(c["dy"], c["x"])
    acc0 = (c["dw0"], c["db0"] if dbias else None) if accumulate else None
    bw, bb = R.wgrad_bar(c["dy"], c["x"], _nslab(row), acc0)
    if accumulate:
        dw, db = dw + c["dw0"], db + c["db0"]
    return {"y": (R.fwd(c["x"], c["w"], b), R.fwd_bar(c["x"], c["w"], b)), "dx": (R.dgrad(c["dy"], c["w"]), R.dgrad_bar(c["dy"], c["w"])),
            "dw": (dw, bw), "db": (db, bb)}


def _compare(tag, arm, got, truth, names=("y", "dx", "dw", "db")):
    """exact arm: bits; real arm: the bars -> {name: worst error / bar}"""
    worst = {}
    for k in names:
        if got[k] is None:
            continue
        if arm == "exact":
            _same_bits(f"{tag} {k}", got[k], truth[k][0].astype(np.float32))
            worst[k] = 0.0
        else:
            worst[k] = _check(f"{tag} {k}", got[k], truth[k][0], truth[k][1], True)
    return worst


# ============================================================================================== C ABI level
@pytest.mark.parametrize("row", R.CASES, ids=R.ids())
def test_c_abi_vs_fp64(row):
    """kmh_pointwise_pack / _fwd / _dgrad / _wgrad on every row of the table, both arms, each run twice: wt is w.T bit for bit
    (Cout = 1 and Cin = 1 among the rows), the exact arm equals the float32 cast of the fp64 result in every bit, the real arm
    stays under its bars, the second run repeats the first in every bit (no atomics), and no store leaves a tensor.
    Observed worst error / bar over the table: y 0.371 (Cin = 1), dx 0.250 (Cout = 1), dw 0.266, db 0.194 (both at N V = 2):
    one or two roundings under a bar of four or five; 0.13 at most from K = 31 on."""
    for arm in ("exact", "real"):
        c = R.case(arm, row)
        got, again = _run(row, c), _run(row, c)
        for k in got:
            _same_bits(f"{arm} {k} repeated", again[k], got[k])
        _same_bits(f"{arm} wt", got["wt"], np.ascontiguousarray(c["w"].T))
        worst = _compare(arm, arm, got, _truth(row, c))
        if arm == "real":
            print(f"{row}: worst error / bar " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("row", R.CASES, ids=R.ids())
def test_accumulate_and_no_bias_gradient(row):
    """accumulate = 1 on pre-filled dw and dbias (integers in the exact arm): the result is dw0 + dw -- exact, or within the bar +
    u |dw0 + dw|.  With dbias = NULL (accumulating or not) dw keeps the bits of the run with a bias gradient.  Without a bias the
    forward is the plain product, bar (Cin + 3) u sum|w x|.
    Observed worst error / bar over the table: dw 0.337, db 0.306 (both at N V = 2), y without bias 0.284 (Cin = 3)."""
    for arm in ("exact", "real"):
        c = R.case(arm, row)
        worst = {}
        for accumulate in (1, 0):
            full, nodb = _run(row, c, accumulate=accumulate), _run(row, c, bias=False, dbias=False, accumulate=accumulate)
            assert nodb["db"] is None
            _same_bits(f"{arm} accumulate {accumulate}: dw without dbias", nodb["dw"], full["dw"])
            if accumulate:
                worst = _compare(f"{arm} accumulate", arm, full, _truth(row, c, accumulate=1), ("dw", "db"))
            else:
                worst["y nobias"] = _compare(f"{arm} no bias", arm, nodb, _truth(row, c, bias=False), ("y",))["y"]
        if arm == "real":
            print(f"{row}: worst error / bar " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_table_reaches_one_slab_and_many():
    """by the library's own workspace size the table holds rows whose weight gradient is one slab and rows with several, the
    largest row with a ragged last one (equal slabs would need N V to be a multiple of their number)"""
    ns = {row: _nslab(row) for row in R.CASES}
    print("slabs: " + "  ".join(f"{n}x{v}:{ns[(n, v, ci, co)]}" for n, v, ci, co in R.CASES))
    assert min(ns.values()) == 1 and ns[(3, 21, 65, 127)] == 1
    assert sum(1 for v in ns.values() if v > 1) >= 3
    big = (3, 6667, 65, 31)
    assert ns[big] > 2 and (3 * 6667) % ns[big] != 0
    assert all(R.wgrad_terms(r[0], r[1], ns[r]) <= R.K_RIGOROUS for r in R.CASES)


# ====================================================================================== non-finite containment
def _poison_cases():
    N, V, Cin, Cout = R.CONTAINMENT_ROW
    n, v, ci, co = N - 1, V - 1, Cin - 1, Cout - 1
    yes = {"x": {"y": (n, slice(None), v), "dw": (slice(None), ci)},
           "dy": {"dx": (n, v, slice(None)), "dw": (co, slice(None)), "db": (co,)},
           "w": {"y": (slice(None), co, slice(None)), "dx": (slice(None), slice(None), ci)}}
    at = {"x": (n, v, ci), "dy": (n, co, v), "w": (co, ci)}
    return [(name, at[name], yes[name], val) for name in ("x", "dy", "w") for val in (np.nan, np.inf)]


@pytest.mark.parametrize("name,at,hit,val", _poison_cases(), ids=[f"{c[0]}-{c[3]}" for c in _poison_cases()])
def test_non_finite_values_stay_in_their_outputs(name, at, hit, val):
    """one NaN / +inf in x at the last voxel of a ragged tile (and the last channel of a one-channel chunk), in dy at the last
    row of a ragged Cout tile, in w at its last element: exactly the outputs that depend on the element are non-finite -- that
    voxel's column of y and that column of dw; that voxel's row of dx, that row of dw and db; that channel's plane of y and
    column of dx -- and every other output is still within its bar: the zero-masked MFMA operands of the ragged tiles never
    meet a non-finite partner in a lane that is stored.  Real arm (no zeros: inf times a valid operand is inf, not NaN).
    Observed worst error / bar of the untouched outputs: 0.066 in all six runs (the clean row's dx)."""
    row = R.CONTAINMENT_ROW
    clean = R.real_case(*row)
    c = {k: v.copy() for k, v in clean.items()}
    c[name][at] = val
    got = _run(row, c)
    truth = _truth(row, clean)
    with np.errstate(invalid="ignore", over="ignore"):
        poisoned = {"y": R.fwd(c["x"], c["w"], c["b"]), "dx": R.dgrad(c["dy"], c["w"])}
        poisoned["dw"], poisoned["db"] = R.wgrad(c["dy"], c["x"])
    worst = 0.0
    for k in ("y", "dx", "dw", "db"):
        want = np.zeros(truth[k][0].shape, bool)
        if k in hit:
            want[hit[k]] = True
        assert np.array_equal(~np.isfinite(poisoned[k]), want), k            # the restatement agrees on what depends on it
        bad = ~np.isfinite(got[k])
        assert np.array_equal(bad, want), f"{k}: {int(bad.sum())} non-finite outputs, {int(want.sum())} depend on {name}{at}"
        worst = max(worst, _check(k, got[k][~want], truth[k][0][~want], truth[k][1][~want], True))
    print(f"{name}{at} = {val}: worst error / bar of the untouched outputs {worst:.3f}")


# =========================================================================================== autograd level
DIMS = {300: (3, 10, 10), 256: (4, 8, 8), 21: (1, 3, 7)}


def _autograd(row, c, bias):
    B = _B()
    N, V, Cin, Cout = row
    x = _dev(c["x"]).reshape(N, *DIMS[V], Cin).requires_grad_(True)
    w = _dev(c["w"]).reshape(Cout, Cin, 1, 1, 1).requires_grad_(True)
    b = None if bias is None else _dev(bias).requires_grad_(True)
    y = B.pointwise(x, w, b)
    assert y.shape == (N, Cout) + DIMS[V] and y.is_contiguous()
    g = _dev(np.ascontiguousarray(c["dy"].transpose(0, 2, 1))).reshape(N, *DIMS[V], Cout).permute(0, 4, 1, 2, 3)
    assert not g.is_contiguous()
    y.backward(g)
    return {"y": _np(y).reshape(N, Cout, V), "dx": _np(x.grad).reshape(N, V, Cin), "dw": _np(w.grad).reshape(Cout, Cin),
            "db": None if b is None else _np(b.grad)}


@pytest.mark.parametrize("row", R.AUTOGRAD_ROWS, ids=R.ids(R.AUTOGRAD_ROWS))
def test_autograd_wrapper_vs_fp64(row):
    """B.pointwise forward and .backward() with a non-contiguous dy, both arms, against the same reference and bars.
    Observed worst error / bar: y 0.031, dx 0.066, dw 0.042, db 0.010 -- the C ABI's figures for the same rows."""
    for arm in ("exact", "real"):
        c = R.case(arm, row)
        worst = _compare(arm, arm, _autograd(row, c, c["b"]), _truth(row, c))
        if arm == "real":
            print(f"{row}: worst error / bar " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("row", R.AUTOGRAD_ROWS, ids=R.ids(R.AUTOGRAD_ROWS))
def test_autograd_wrapper_without_bias(row):
    """bias = None through B.pointwise (exact arm): the forward is exact, there is no bias gradient, and dx and dw are
    identical in bits to the run with a zero bias"""
    c = R.exact_case(*row)
    none, zero = _autograd(row, c, None), _autograd(row, c, np.zeros(row[3], np.float32))
    _same_bits("y", none["y"], R.fwd(c["x"], c["w"], None).astype(np.float32))
    _same_bits("y with a zero bias", zero["y"], none["y"])
    assert none["db"] is None
    _same_bits("db of the zero bias", zero["db"], R.wgrad(c["dy"], c["x"])[1].astype(np.float32))
    for k in ("dx", "dw"):
        _same_bits(k, none[k], zero[k])
    _compare("no bias", "exact", none, _truth(row, c, bias=False), ("dx", "dw"))


# ============================================================================================= model wiring
def _net(trunc, K):
    """the smallest documented configurations: f_maps 32 at 4 levels, truncated by 1 (64 channels into the head) or by 2 (128)"""
    from keymorph_amd.unet3d.model import TruncatedUNet3D
    from tests.util import seeded_state_dict, unet_shapes
    net = TruncatedUNet3D(1, K, trunc, final_sigmoid=False, f_maps=32, layer_order="gcr", num_groups=8, num_levels=4,
                          is_segmentation=False, conv_padding=1)
    net.load_state_dict(seeded_state_dict(unet_shapes(K, 32, trunc=trunc), 100), strict=True)
    return net.to(DEV).train()


def _image():
    return torch.rand((2, 1, 16, 16, 16), generator=torch.Generator().manual_seed(7)).to(DEV)


def test_model_above_64_channels_goes_through_pointwise():
    """TruncatedUNet3D(f_maps 32) truncated by 2 has 128 channels in front of final_conv: keypoints_ij(x) is
    ops.com3d(B.pointwise(features(x), w, b)) computed by hand IN BITS, and so are the gradients of final_conv.weight,
    final_conv.bias and the image; forward(x) is B.pointwise(...) in bits; keypoint weighting, which needs the fused head,
    raises NotImplementedError from both of its entry points."""
    from keymorph_amd import ops
    B = _B()
    K = 33
    net = _net(2, K)
    assert net.final_conv.in_channels == 128 > B.HEAD_FUSED_MAX_CIN
    img = _image()
    cot = torch.randn((2, K, 3), generator=torch.Generator().manual_seed(8)).to(DEV)

    def grads(fn):
        net.zero_grad(set_to_none=True)
        x = img.clone().requires_grad_(True)
        p = fn(x)
        (p * cot).sum().backward()
        return p.detach(), net.final_conv.weight.grad.clone(), net.final_conv.bias.grad.clone(), x.grad.clone()

    calls = []
    real = B.pointwise
    B.pointwise = lambda *a: (calls.append(1), real(*a))[1]
    try:
        model = grads(net.keypoints_ij)
        assert len(calls) == 1
    finally:
        B.pointwise = real
    hand = grads(lambda x: ops.com3d(B.pointwise(net.features(x), net.final_conv.weight, net.final_conv.bias)))
    for nm, a, b in zip(("keypoints", "d final_conv.weight", "d final_conv.bias", "d image"), model, hand):
        assert a.shape == b.shape and bool(torch.isfinite(a).all()) and torch.equal(a, b), nm
    assert float(model[1].abs().max()) > 0 and float(model[3].abs().max()) > 0
    with torch.no_grad():
        y = net(img)
        assert y.shape == (2, K, 4, 4, 4)
        assert torch.equal(y, B.pointwise(net.features(img), net.final_conv.weight, net.final_conv.bias))
        _check("heat-map vs fp64", _np(y).reshape(2, K, 64), *_heatmap_truth(net, img))
    for fn in (net.keypoints_and_power, net.keypoints_and_moments):
        with pytest.raises(NotImplementedError, match="fused head"):
            fn(img)


def _heatmap_truth(net, img):
    """fp64 final conv of the model's own features and its bar (Cin + 3) u (sum|w x| + |b|)"""
    feat = _np(net.features(img))
    w, b = _np(net.final_conv.weight).reshape(net.final_conv.out_channels, -1), _np(net.final_conv.bias)
    x = feat.reshape(feat.shape[0], -1, feat.shape[-1])
    return R.fwd(x, w, b), R.fwd_bar(x, w, b)


def test_model_at_64_channels_takes_the_fused_head(monkeypatch):
    """truncated by 1 the head sees 64 channels: keypoints_ij reaches B.head_com (and never B.pointwise), its keypoints agree
    with com3d(pointwise(features)) to test_fused_head_matches_unfused's bound (atol 2e-6, rtol 1e-5), and keypoint weighting
    is served from both entry points with the same keypoints"""
    from keymorph_amd import ops
    B = _B()
    K = 33
    net = _net(1, K)
    assert net.final_conv.in_channels == 64 == B.HEAD_FUSED_MAX_CIN
    img = _image()
    seen = {"head_com": 0, "pointwise": 0}
    for name in seen:
        real = getattr(B, name)
        monkeypatch.setattr(B, name, lambda *a, _n=name, _f=real, **k: (seen.__setitem__(_n, seen[_n] + 1), _f(*a, **k))[1])
    with torch.no_grad():
        pts = net.keypoints_ij(img)
    assert seen == {"head_com": 1, "pointwise": 0}
    monkeypatch.undo()
    with torch.no_grad():
        ref = ops.com3d(B.pointwise(net.features(img), net.final_conv.weight, net.final_conv.bias))
        np.testing.assert_allclose(_np(pts), _np(ref), atol=2e-6, rtol=1e-5)
        pm = net.keypoints_and_moments(img)
        assert pm[3] == 512
        np.testing.assert_allclose(_np(pm[0]), _np(ref), atol=2e-6, rtol=1e-5)
    pw = net.keypoints_and_power(img)
    np.testing.assert_allclose(_np(pw[0]), _np(ref), atol=2e-6, rtol=1e-5)
    assert pw[1].shape == (2, K)


@pytest.mark.parametrize("Cin", [65, 68])
def test_fused_head_refuses_more_than_64_channels(Cin):
    """the other side of the dispatch: the fused head's C ABI answers -22 above 64 input channels, on its fp32 route (Cin = 65)
    and its split-operand route (Cin = 68), instead of computing something; so does the fp32 backward entry point"""
    B = _B()
    Err = _L()[4]
    r = np.random.default_rng(Cin)
    feat, w, b = (_dev(r.standard_normal(s).astype(np.float32)) for s in ((1, 2, 4, 32, Cin), (8, Cin, 1, 1, 1), (8,)))
    with pytest.raises(Err, match="-22"):
        B.head_com(feat, w, b)
    if Cin == 65:       # the fp32 backward entry point, which no wrapper reaches once the forward has refused: before any launch
        lib, _, _p, _stream, _ = _L()
        N, D, H, W, K = 1, 2, 4, 32, 8
        dpts, sums, dfeat, dw, db = (torch.zeros(s, device=DEV) for s in ((N, K, 3), (N, K, 4), (N, D, H, W, Cin), (K, Cin), (K,)))
        ws = torch.empty(int(lib.kmh_headcom_bwd_ws_bytes(N, D * H * W, Cin, K)), dtype=torch.uint8, device=DEV)
        assert lib.kmh_headcom_bwd(_p(dpts), None, _p(feat), _p(w), _p(b), _p(sums), _p(dfeat), _p(dw), _p(db), N, D, H, W, Cin, K,
                                   0, _p(ws), _stream()) == -22
