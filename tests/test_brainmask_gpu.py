"""GPU: the brain-extraction step -- trilinear resize (csrc/resize.hip), connected components / clean_mask
(csrc/components.hip), the thin and routed 3x3x3 layers (csrc/conv_thin.hip, keymorph_amd/brain_ops.py), Simple_Unet against
the reference's fixture and io.extract_brain -- at the smallest shapes at which each kernel can still go wrong."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import brainmask_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def gen(s):
    return torch.Generator().manual_seed(s)


def ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def close(a, b, atol, rtol):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a, b, atol=atol, rtol=rtol)


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


# ---- (a) resize -----------------------------------------------------------------------------------------------------------
_RESIZE_IDS = ["%s-%s-%s" % ("x".join(map(str, c[0])), c[1], c[2]) for c in R.RESIZE_CASES]


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=_RESIZE_IDS)
def test_resize_forward_backward(case):
    """Forward against the fp64 evaluation with the same fp32 tables: <= 1e-6 max|x| (three nested lerps are nine fp32
    roundings ~ 5.4e-7).  Backward against fp64 autograd of that restatement: per element <= (T + 4) 2^-24 sum|w g| with T the
    number of contributing outputs and sum|w g| the transposed operator applied to |g|.  Two backward runs are bit-identical."""
    from keymorph_amd import utils
    shape, size, factor = case
    g = gen(11)
    x = torch.randn(shape, generator=g)
    tabs, out = R.resize_tables(shape, size, factor)
    gy = torch.randn(shape[:2] + out, generator=g)
    x64 = x.double().requires_grad_(True)
    ref = R.resize_ref64(x64, tabs)
    (gref,) = torch.autograd.grad(ref, x64, gy.double())
    xa = x64.detach().clone().requires_grad_(True)
    (gabs,) = torch.autograd.grad(R.resize_ref64(xa, tabs), xa, gy.double().abs())
    T = R.resize_contributors(tabs).double()

    xd = x.to(DEV).requires_grad_(True)
    kw = dict(size=size) if size is not None else dict(scale_factor=factor)
    y = utils.resize_trilinear(xd, **kw)
    assert tuple(y.shape) == tuple(ref.shape) and y.dtype == torch.float32
    err = float((y.detach().cpu().double() - ref.detach()).abs().max())
    print(f"resize fwd {shape} -> {out}: max err {err:.3e} (bar {1e-6 * float(x.abs().max()):.3e})")
    assert err <= 1e-6 * float(x.abs().max())
    (g1,) = torch.autograd.grad(y, xd, gy.to(DEV), retain_graph=True)
    (g2,) = torch.autograd.grad(y, xd, gy.to(DEV))
    assert torch.equal(g1, g2)
    bound = (T + 4) * 2.0 ** -24 * gabs
    diff = (g1.cpu().double() - gref).abs()
    print(f"resize bwd: worst diff / bound {float((diff / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((diff <= bound).all())


@pytest.mark.parametrize("C", [4, 5, 32])
def test_resize_layouts_bit_identical(C):
    from keymorph_amd import ops
    g = gen(C)
    x = torch.randn(2, C, 5, 6, 7, generator=g).to(DEV)
    for kw in (dict(scale_factor=2), dict(size=(7, 4, 13))):
        a = ops.resize_trilinear3d(x.clone().requires_grad_(True), **kw)
        xl = ndhwc(x).requires_grad_(True)
        b = ops.resize_trilinear3d(xl, channels_last=True, **kw)
        assert torch.equal(a, ncdhw(b))
        cot = torch.randn(a.shape, generator=g).to(DEV)
        (gb,) = torch.autograd.grad(b, xl, ndhwc(cot))
        xa = x.clone().requires_grad_(True)
        (ga,) = torch.autograd.grad(ops.resize_trilinear3d(xa, **kw), xa, cot)
        assert torch.equal(ga, ncdhw(gb))


def test_resize_errors():
    from keymorph_amd import utils
    from keymorph_amd._lib import KeymorphHipError
    with pytest.raises(KeymorphHipError):
        utils.resize_trilinear(torch.zeros(1, 1, 4, 4, 4), scale_factor=2)
    with pytest.raises(ValueError):
        utils.resize_trilinear(torch.zeros(1, 1, 4, 4, 4, device=DEV))


# ---- (b) components and clean_mask ------------------------------------------------------------------------------------------
def _random_field():
    return (torch.rand(24, 24, 24, generator=gen(3)) < 0.06).numpy().astype(np.uint8)


def _patterns3():
    corners = np.zeros((3, 3, 3), dtype=np.uint8)
    corners[::2, ::2, ::2] = 1                                    # eight isolated corners
    centre = corners.copy()
    centre[1, 1, 1] = 1                                           # the centre joins all of them
    checker = (np.indices((3, 3, 3)).sum(0) % 2 == 0).astype(np.uint8)
    return {"corners": corners, "centre": centre, "checker": checker, "full": np.ones((3, 3, 3), dtype=np.uint8)}


MASKS = {
    "one_set": lambda: np.ones((1, 1, 1), dtype=np.uint8),
    **{"p3_" + k: (lambda v=v: v) for k, v in _patterns3().items()},
    "plane": lambda: (torch.rand(1, 20, 70, generator=gen(4)) < 0.45).numpy().astype(np.uint8),
    "corner_cubes": R.corner_cubes,
    "boxes_chains": R.boxes_and_chains,
    "serpentine": lambda: R.serpentine(32),
    "random": _random_field,
    "blob_islands": R.blob_and_islands,
}


@pytest.mark.parametrize("name", list(MASKS))
def test_components_and_clean_mask(name):
    from scipy import ndimage
    from keymorph_amd import ops
    from keymorph_amd.model import clean_mask
    m = MASKS[name]()
    lab_ref, n = R.label_oracle(m)
    if name == "random":
        sizes = np.bincount(lab_ref.reshape(-1))[1:]
        assert n >= 50 and len(set(sizes.tolist())) >= 4, (n, sorted(set(sizes.tolist())))
    md = torch.from_numpy(m).to(DEV)
    lab = ops.connected_components3d(md)
    assert lab.dtype == torch.int32 and tuple(lab.shape) == m.shape
    assert torch.equal(lab, ops.connected_components3d(md.bool()))           # two runs (and bool input): bit-identical
    lab = lab.cpu().numpy()
    assert np.array_equal(lab == 0, m == 0)
    on = m != 0
    pairs = np.unique(np.stack([lab[on], lab_ref[on]]), axis=1)
    assert pairs.shape[1] == n == len(np.unique(lab[on])) == len(np.unique(lab_ref[on]))       # a bijection
    idx = np.arange(m.size).reshape(m.shape)
    first = np.asarray(ndimage.minimum(idx, lab_ref, index=np.arange(1, n + 1)))
    assert np.array_equal(lab[on] - 1, first[lab_ref[on] - 1])               # label - 1 = the smallest linear index
    for thr in (0.2, 0.05):
        want = R.clean_mask_oracle(m, thr)
        got_np = clean_mask(m, thr)
        assert isinstance(got_np, np.ndarray) and got_np.dtype == np.uint8 and np.array_equal(got_np, want)
        got_t = clean_mask(md, thr)
        assert isinstance(got_t, torch.Tensor) and got_t.dtype == torch.uint8 and got_t.is_cuda
        assert np.array_equal(got_t.cpu().numpy(), want)
    assert np.array_equal(clean_mask(m.astype(np.float32)), R.clean_mask_oracle(m, 0.2))     # the notebook passes floats


def test_clean_mask_errors():
    from keymorph_amd import ops
    from keymorph_amd.model import clean_mask
    assert int(ops.connected_components3d(torch.zeros(1, 1, 1, dtype=torch.uint8, device=DEV)).item()) == 0
    with pytest.raises(ValueError):
        clean_mask(torch.zeros(4, 4, dtype=torch.uint8, device=DEV))                 # not 3-D
    with pytest.raises(ValueError):
        clean_mask(np.zeros((2, 3, 4, 5), dtype=np.uint8))
    with pytest.raises(ValueError):
        clean_mask(torch.full((3, 3, 3), 2, dtype=torch.uint8, device=DEV))          # values other than 0 / 1
    with pytest.raises(ValueError):
        clean_mask(np.array([[[0.0, 0.5]]]))
    with pytest.raises(ValueError):
        clean_mask(np.zeros((1, 1, 1), dtype=np.uint8))                              # empty: the reference's np.max([])
    with pytest.raises(ValueError):
        clean_mask(torch.zeros(5, 6, 7, dtype=torch.uint8, device=DEV))


def test_clean_mask_batch_is_per_sample():
    from keymorph_amd import ops
    ms = [R.boxes_and_chains(), np.roll(R.boxes_and_chains(), 3, axis=2)]
    out, info = ops.clean_mask3d(torch.from_numpy(np.stack(ms)).to(DEV), 0.2)
    for i, m in enumerate(ms):
        assert np.array_equal(out[i].cpu().numpy(), R.clean_mask_oracle(m, 0.2))
    largest = [int(np.bincount(R.label_oracle(m)[0].reshape(-1))[1:].max()) for m in ms]
    assert info.tolist() == largest + [0]


# ---- (c) the ten layer shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", R.LAYER_PAIRS)
def test_layer_shapes(cin, cout):
    """Forward with bias, data gradient and weight / bias gradient of every (Cin, Cout) of the network through whichever route
    brain_ops selects, against fp64 F.conv3d, with the bars test_convblock_group_norm uses for the same operators."""
    from keymorph_amd import brain_ops
    N, D, H, W = 2, 16, 8, 32
    g = gen(1000 + 37 * cin + cout)
    x = torch.randn(N, cin, D, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / np.sqrt(27 * cin)
    b = 0.1 * torch.randn(cout, generator=g)
    cot = torch.randn(N, cout, D, H, W, generator=g)
    ref = [t.double().requires_grad_(True) for t in (x, w, b)]
    yr = F.conv3d(ref[0], ref[1], ref[2], padding=1)
    (yr * cot.double()).sum().backward()
    got = [ndhwc(x).to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)]
    y = brain_ops._ConvBias.apply(got[0], got[1], got[2], False)
    (y * ndhwc(cot).to(DEV)).sum().backward()
    route = brain_ops.routes(cin, cout)
    errs = {"fwd": float((ncdhw(y).detach().cpu().double() - yr.detach()).abs().max())}
    for name, a, r in zip(("dgrad", "wgrad", "bias"), got, ref):
        ga = ncdhw(a.grad) if name == "dgrad" else a.grad
        errs[name] = float((ga.cpu().double() - r.grad).abs().max() / r.grad.abs().max())
    print(f"layer {cin} -> {cout} {route}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    close(ncdhw(y), yr, 2e-5, 1e-4)
    for a, r, perm in zip(got, ref, (True, False, False)):
        ga = ncdhw(a.grad) if perm else a.grad
        close(ga, r.grad, 2e-4 * float(r.grad.abs().max()), 1e-3)
    if route["wgrad"] == "thin":
        xd, dz = got[0].detach(), ndhwc(cot).to(DEV)
        a = brain_ops.conv_wgrad(xd, dz, None, cout)
        c = brain_ops.conv_wgrad(xd, dz, None, cout)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
        assert torch.equal(a[0], got[1].grad)


def test_thin_layer_relu_mask_and_ragged_volume():
    """The thin kernels on a volume that is no multiple of the 2 x 4 x 32 brick, with the ReLU fused into the forward and its
    mask into both gradients: against fp64 autograd with the mask taken from the computed output."""
    from keymorph_amd import brain_ops
    for cin, cout in ((1, 4), (8, 1), (4, 8)):
        g = gen(50 + cin)
        N, D, H, W = 2, 3, 5, 37
        x = torch.randn(N, cin, D, H, W, generator=g)
        w = torch.randn(cout, cin, 3, 3, 3, generator=g) / np.sqrt(27 * cin)
        b = 0.1 * torch.randn(cout, generator=g)
        cot = torch.randn(N, cout, D, H, W, generator=g)
        got = [ndhwc(x).to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)]
        y = brain_ops._ConvBias.apply(got[0], got[1], got[2], True)
        (y * ndhwc(cot).to(DEV)).sum().backward()
        ref = [t.double().requires_grad_(True) for t in (x, w, b)]
        zr = F.conv3d(ref[0], ref[1], ref[2], padding=1)
        mask = (ncdhw(y).cpu() > 0).double()
        close(ncdhw(y), F.relu(zr), 2e-5, 1e-4)
        (zr * mask * cot.double()).sum().backward()
        for a, r, perm in zip(got, ref, (True, False, False)):
            ga = ncdhw(a.grad) if perm else a.grad
            close(ga, r.grad, 2e-4 * float(r.grad.abs().max()), 1e-3)


# ---- (d) Simple_Unet against the fixture ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.FIXTURE_CASES))
def test_simple_unet_golden(fx, case):
    """The bars test_convnet_golden uses for these very blocks.  Also prints every tensor's relative L2 distance from the
    fixture's fp64 run beside the reference fp32's own (a record; not a bar)."""
    from keymorph_amd.model import Simple_Unet
    use_in, shape = R.FIXTURE_CASES[case]
    net = Simple_Unet(1, 1, use_in, R.ENC_NF, R.DEC_NF)
    net.load_state_dict(R.fixture_state_dict(fx), strict=True)
    net = net.to(DEV).train()
    x = torch.from_numpy(fx[f"{case}::x"]).to(DEV).requires_grad_(True)
    assert tuple(x.shape) == shape
    y = net(x)
    y.backward(torch.from_numpy(fx[f"{case}::cot"]).to(DEV))

    def rel(a, b):
        a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
        return float((a - b).norm() / (b.norm() + 1e-30))

    rows = [("y", y.detach().cpu(), fx[f"{case}::y"], fx[f"{case}::y64"]),
            ("gx", x.grad.cpu(), fx[f"{case}::gx"], fx[f"{case}::gx64"])]
    rows += [(k, p.grad.cpu(), fx[f"{case}::g::{k}"], fx[f"{case}::g64::{k}"]) for k, p in net.named_parameters()]
    print(f"Simple_Unet {case}: relative L2 from the fp64 run   this package | reference fp32")
    for k, mine, r32, r64 in rows:
        print(f"  {k:22s} {rel(mine, r64):.2e} | {rel(r32, r64):.2e}")

    ref = fx[f"{case}::y"]
    close(y, ref, 2e-4 * max(1.0, float(np.abs(ref).max())), 1e-3)
    for k, p in net.named_parameters():
        r = torch.from_numpy(fx[f"{case}::g::{k}"]).double().reshape(-1)
        if use_in and k.endswith("conv1.bias"):
            # InstanceNorm removes the per-channel mean, so d/d(bias) == 0 exactly: both sides are round-off
            wn = float(torch.from_numpy(fx[f"{case}::g::{k.replace('bias', 'weight')}"]).double().norm())
            assert float(p.grad.double().norm()) < 1e-3 * wn and float(r.norm()) < 1e-3 * wn, k
            continue
        e = float((p.grad.cpu().double().reshape(-1) - r).norm() / (r.norm() + 1e-30))
        assert e < 3e-2, (k, e)
    with torch.no_grad():
        y0 = net(x.detach())
        assert torch.equal(y0, y.detach())
        dp = torch.nn.DataParallel(net, device_ids=[torch.cuda.current_device()])
        assert torch.equal(dp(x.detach()), y0)


# ---- (e) extract_brain --------------------------------------------------------------------------------------------------------
def test_extract_brain(fx):
    from keymorph_amd.io import extract_brain
    from keymorph_amd.model import Simple_Unet, clean_mask
    from keymorph_amd.utils import resize_trilinear
    net = Simple_Unet(1, 1, False, R.ENC_NF, R.DEC_NF)
    net.load_state_dict(R.fixture_state_dict(fx), strict=True)
    net = net.to(DEV).eval()
    img = torch.randn(1, 1, 48, 40, 56, generator=gen(9)).to(DEV)
    with torch.no_grad():
        prob = resize_trilinear(net(resize_trilinear(img, size=(32, 32, 32))), scale_factor=2)
    level = float(prob.median())                           # seeded weights are no brain extractor: a level that splits the volume
    out = extract_brain(net, img, size=(32, 32, 32), level=level, clean_threshold=0.2)
    assert tuple(out.shape) == (1, 64, 64, 64) and out.dtype == torch.uint8 and out.is_cuda
    hand = clean_mask((prob[0, 0] >= level).to(torch.uint8), 0.2)
    assert torch.equal(out[0], hand)
    assert 0 < int(out.sum()) < out.numel()
    with pytest.raises(ValueError):
        extract_brain(net, img[:, 0], size=(32, 32, 32))
