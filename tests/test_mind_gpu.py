"""GPU: ops.mind_ssc_loss / ops.mind_bounds / loss_ops.MINDLoss (csrc/mind.hip) against the fp64 restatement of
tests/mind_ref.py -- value and both gradients -- and what is built on them (io.register_bspline(metric="mind"),
io.register_svf(metric="mind"), model.IntensityRegistration(metric="mind")).

The bars.  d32 = the distance of the restatement evaluated in fp32 on the CPU from its fp64 evaluation: what fp32 costs in any
order.  The value is compared absolutely, the gradients in relative L2 per sample; the kernel gets 4 x the LARGEST d32 over all
cases of the table (tests/test_lncc_gpu.py's rule).  Nothing comes from the kernel.  The gradient's d32 of `multi_tile` (6.7e-4
for db) and `masked` (6.6e-5) is not rounding of sums: at a voxel where two channels' distances agree to fp32's last bits the
argmin differs between fp32 and fp64, and the minimum's share of the cotangent moves to another channel; the other cases are at
2e-7 .. 2e-6.  Each test prints the case's own d32 beside the bar.  `masked` has exact 12-way ties, where autograd's choice is
not the definition's: it is compared against the closed form, which takes the lowest channel index as the kernel does.

Measured on an MI355X: see DESIGN.md section 8h."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import bspline_ref as B
from tests import mind_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


def _rel(x, ref):
    return float((x.to(F64) - ref).norm() / ref.norm())


def _evaluate(name, dtype):
    a, b, r, d = R.case_inputs(name)
    out, da, db = R.evaluate(a, b, r, d, dtype=dtype)
    if name in R.TIED:
        da, db = R.closed_form(a, b, r, d, dtype=dtype)
    return out, da, db


@functools.lru_cache(maxsize=None)
def reference(name):
    """(out64, da64, db64, d32 of the value, d32 of the gradients), computed once per case."""
    o64, da64, db64 = _evaluate(name, F64)
    o32, da32, db32 = _evaluate(name, torch.float32)
    d_val = float((o32.to(F64) - o64).abs().max())
    d_grad = max(_rel(g32[n], g64[n]) for g32, g64 in ((da32, da64), (db32, db64)) for n in range(o64.shape[0]))
    return o64, da64, db64, d_val, d_grad


@functools.lru_cache(maxsize=None)
def bars():
    """4 x the largest d32 of the family: (value, gradients)."""
    refs = [reference(name) for name in R.CASES]
    return 4 * max(r[3] for r in refs), 4 * max(r[4] for r in refs)


def run(name, need=(True, True), rows=None, bounds=None):
    from keymorph_amd import ops
    a, b, r, d = R.case_inputs(name)
    if rows is not None:
        a, b = a[rows], b[rows]
    x, y = a.to(DEV).requires_grad_(need[0]), b.to(DEV).requires_grad_(need[1])
    out = ops.mind_ssc_loss(x, y, r, d, bounds)
    out.sum().backward()
    return out.detach(), x.grad, y.grad


@pytest.mark.parametrize("name", list(R.CASES))
def test_value_and_gradients_match_fp64(name):
    o64, da64, db64, d_val, d_grad = reference(name)
    bar_val, bar_grad = bars()
    out, da, db = run(name)
    assert out.shape == o64.shape and out.dtype == torch.float32
    err = float((out.cpu().to(F64) - o64).abs().max())
    print(f"{name}: value {[f'{float(v):.6e}' for v in o64]}  abs error {err:.3e}  d32 {d_val:.3e}  bar {bar_val:.3e}")
    assert math.isfinite(err) and err <= bar_val, (name, err, bar_val)
    for which, g, g64 in (("da", da, da64), ("db", db, db64)):
        assert torch.isfinite(g).all()
        for n in range(g64.shape[0]):
            e = _rel(g[n].cpu(), g64[n])
            print(f"{name}[{n}]: {which} relative L2 {e:.3e}  d32 of the case {d_grad:.3e}  bar {bar_grad:.3e}")
            assert math.isfinite(e) and e <= bar_grad, (name, which, n, e, bar_grad)


def test_bounds_match_fp64():
    """ops.mind_bounds against the restatement: per-tile fp32 partials added in fp64, so the relative bar is 4 x the fp32
    restatement's own distance from fp64, the largest over the cases -- and d32 counts as no less than 2^-24, the rounding of
    the fp32 result itself."""
    from keymorph_amd import ops
    got, ref, d32 = {}, {}, 2.0 ** -24
    for name in R.CASES:
        a, b, r, d = R.case_inputs(name)
        ref[name] = R.bounds_of(a.double(), b.double(), r, d)
        d32 = max(d32, float(((R.bounds_of(a, b, r, d).double() - ref[name]) / ref[name]).abs().max()))
        got[name] = ops.mind_bounds(a.to(DEV), b.to(DEV), r, d)
    for name in R.CASES:
        assert got[name].shape == ref[name].shape and got[name].dtype == torch.float32
        e = float(((got[name].cpu().double() - ref[name]) / ref[name]).abs().max())
        print(f"{name}: bounds {ref[name].reshape(-1).tolist()}  relative error {e:.3e}  bar {4 * d32:.3e}")
        assert e <= 4 * d32, (name, e, d32)


def test_flat_and_masked_volumes_give_finite_gradients():
    from keymorph_amd import ops
    a, b, r, d = R.case_inputs("masked")
    half = a.shape[4] // 2
    out, da, db = run("masked")
    assert torch.isfinite(da).all() and torch.isfinite(db).all()
    # a's neighbour differences are 0 for x < half - d, so nothing of d out / d a lands below x = half - 2 d
    assert float(da[..., :half - 2 * d].abs().max()) == 0.0 and float(da.abs().max()) > 0.0
    flat = torch.full_like(b, 3.0).to(DEV).requires_grad_()
    y = b.to(DEV).requires_grad_()
    val = ops.mind_ssc_loss(flat, y, r, d)
    val.sum().backward()
    assert torch.isfinite(val).all() and torch.isfinite(flat.grad).all() and torch.isfinite(y.grad).all()
    assert float(ops.mind_ssc_loss(flat.detach(), flat.detach(), r, d)[0]) == 0.0
    assert float(ops.mind_ssc_loss(y.detach(), y.detach(), r, d)[0]) == 0.0


@pytest.mark.parametrize("name", list(R.CASES))
def test_repeat_runs_are_bit_identical(name):
    first, again = run(name), run(name)
    for x, y in zip(first, again):
        assert torch.equal(x, y)


def test_batch_equals_single_samples():
    out, da, db = run("batch")
    for n in range(out.shape[0]):
        o1, da1, db1 = run("batch", rows=slice(n, n + 1))
        assert torch.equal(o1[0], out[n]) and torch.equal(da1[0], da[n]) and torch.equal(db1[0], db[n])


@pytest.mark.parametrize("name", ["batch", "ragged_r2d2", "r3d3"])
def test_one_gradient_alone_equals_the_same_gradient_of_both(name):
    out, da, db = run(name)
    oa, da_only, none_b = run(name, need=(True, False))
    ob, none_a, db_only = run(name, need=(False, True))
    assert none_a is None and none_b is None
    assert torch.equal(oa, out) and torch.equal(ob, out)
    assert torch.equal(da_only, da) and torch.equal(db_only, db)


@pytest.mark.parametrize("name", ["batch", "ragged_r1d1"])
def test_bounds_none_equals_passing_mind_bounds(name):
    from keymorph_amd import ops
    a, b, r, d = R.case_inputs(name)
    bounds = ops.mind_bounds(a.to(DEV), b.to(DEV), r, d)
    assert bounds.shape == (a.shape[0], 2, 2)
    for x, y in zip(run(name), run(name, bounds=bounds)):
        assert torch.equal(x, y)
    # other bounds are another function
    assert not torch.equal(run(name, bounds=bounds * torch.tensor([1.0, 1e-3], device=DEV))[0], run(name)[0])


def test_mind_loss_is_the_mean():
    from keymorph_amd import ops
    from keymorph_amd.loss_ops import MINDLoss
    a, b, _, _ = R.case_inputs("batch")
    a, b = a.to(DEV), b.to(DEV)
    assert torch.equal(MINDLoss()(a, b), ops.mind_ssc_loss(a, b).mean())
    assert torch.equal(MINDLoss(radius=2, dilation=1)(a, b), ops.mind_ssc_loss(a, b, 2, 1).mean())
    x = a.clone().requires_grad_()
    MINDLoss()(x, b).backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().sum()) > 0


def test_input_checks():
    from keymorph_amd import _lib, ops
    a = torch.rand(2, 1, 8, 9, 10, device=DEV)
    b = torch.rand(2, 1, 8, 9, 10, device=DEV)
    assert ops.mind_ssc_loss(a, b).shape == (2,)
    for fn in (ops.mind_ssc_loss, ops.mind_bounds):
        with pytest.raises(_lib.KeymorphHipError):
            fn(a.cpu(), b)
        with pytest.raises(_lib.KeymorphHipError):
            fn(a, b.cpu())
        with pytest.raises(ValueError):
            fn(a[0], b[0])                                           # wrong rank
        with pytest.raises(ValueError):
            fn(a, b[:, :, :7])                                       # mismatched shapes
        with pytest.raises(ValueError):
            fn(a.expand(2, 2, 8, 9, 10), b.expand(2, 2, 8, 9, 10))   # C != 1
        with pytest.raises(ValueError):
            fn(a.double(), b.double())
        for radius, dilation in ((0, 2), (4, 2), (1.5, 2), (1, 0), (1, 4), (1, 2.5), (True, 2)):
            with pytest.raises(ValueError):
                fn(a, b, radius, dilation)
    with pytest.raises(ValueError):
        ops.mind_ssc_loss(a, b, 1, 2, torch.ones(2, 4, device=DEV))
    with pytest.raises(ValueError):
        ops.mind_ssc_loss(a, b, 1, 2, torch.ones(2, 2, 2, device=DEV, dtype=F64))
    # the ABI's own limits: -22 before anything is launched
    lib = _lib.load()
    out = torch.empty(2, device=DEV)
    bd = torch.empty(2, 2, 2, device=DEV)
    ws = torch.empty(int(lib.kmh_mind_ws_bytes(2, 8, 9, 10, 1, 2)), dtype=torch.uint8, device=DEV)
    da = torch.empty_like(a)
    p = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    assert lib.kmh_mind_bounds(p(a), p(b), 2, 8, 9, 10, 1, 2, p(bd), p(ws), s) == 0
    assert lib.kmh_mind_fwd(p(a), p(b), p(bd), 2, 8, 9, 10, 1, 2, p(out), p(ws), s) == 0
    for r, d in ((0, 2), (4, 2), (1, 0), (1, 4)):
        assert lib.kmh_mind_bounds(p(a), p(b), 2, 8, 9, 10, r, d, p(bd), p(ws), s) == -22
        assert lib.kmh_mind_fwd(p(a), p(b), p(bd), 2, 8, 9, 10, r, d, p(out), p(ws), s) == -22
        assert lib.kmh_mind_bwd(p(a), p(b), p(bd), p(out), 2, 8, 9, 10, r, d, p(da), None, p(ws), s) == -22
    for dims in ((0, 8, 9, 10), (2, 8, 0, 10), (2, 8, 9, -3), (2, 2048, 1024, 1024)):                # N = 0, an axis, 2^31 voxels
        assert lib.kmh_mind_bounds(p(a), p(b), *dims, 1, 2, p(bd), p(ws), s) == -22
        assert lib.kmh_mind_fwd(p(a), p(b), p(bd), *dims, 1, 2, p(out), p(ws), s) == -22
        assert lib.kmh_mind_bwd(p(a), p(b), p(bd), p(out), *dims, 1, 2, p(da), None, p(ws), s) == -22
    assert lib.kmh_mind_bounds(None, p(b), 2, 8, 9, 10, 1, 2, p(bd), p(ws), s) == -22
    assert lib.kmh_mind_bounds(p(a), p(b), 2, 8, 9, 10, 1, 2, None, p(ws), s) == -22
    assert lib.kmh_mind_bounds(p(a), p(b), 2, 8, 9, 10, 1, 2, p(bd), None, s) == -22
    assert lib.kmh_mind_fwd(None, p(b), p(bd), 2, 8, 9, 10, 1, 2, p(out), p(ws), s) == -22
    assert lib.kmh_mind_fwd(p(a), None, p(bd), 2, 8, 9, 10, 1, 2, p(out), p(ws), s) == -22
    assert lib.kmh_mind_fwd(p(a), p(b), None, 2, 8, 9, 10, 1, 2, p(out), p(ws), s) == -22
    assert lib.kmh_mind_fwd(p(a), p(b), p(bd), 2, 8, 9, 10, 1, 2, None, p(ws), s) == -22
    assert lib.kmh_mind_fwd(p(a), p(b), p(bd), 2, 8, 9, 10, 1, 2, p(out), None, s) == -22
    assert lib.kmh_mind_bwd(p(a), p(b), p(bd), p(out), 2, 8, 9, 10, 1, 2, p(da), None, p(ws), s) == 0
    assert lib.kmh_mind_bwd(p(a), p(b), p(bd), p(out), 2, 8, 9, 10, 1, 2, None, None, p(ws), s) == 0     # nothing asked for
    assert lib.kmh_mind_bwd(None, p(b), p(bd), p(out), 2, 8, 9, 10, 1, 2, p(da), None, p(ws), s) == -22
    assert lib.kmh_mind_bwd(p(a), p(b), None, p(out), 2, 8, 9, 10, 1, 2, p(da), None, p(ws), s) == -22
    assert lib.kmh_mind_bwd(p(a), p(b), p(bd), None, 2, 8, 9, 10, 1, 2, p(da), None, p(ws), s) == -22
    assert lib.kmh_mind_bwd(p(a), p(b), p(bd), p(out), 2, 8, 9, 10, 1, 2, p(da), None, None, s) == -22
    torch.cuda.synchronize()


def test_gradient_through_align_img_and_bspline_grid_matches_finite_differences():
    """d MIND / d(ctrl) of the chain bspline_grid -> align_img -> mind_ssc_loss at 16^3, bounds of the unwarped pair, against
    central differences of the fp64 restatement on the twelve control values that carry most gradient (chosen by the
    restatement's own autograd), h = 1e-6 as in tests/test_lncc_gpu.py.  The bar: the same central difference taken of the
    restatement evaluated in fp32 differs from the fp64 one by what fp32 costs this chain, 4 x the largest of the twelve; with a
    step of 1e-6 that is rounding noise over 2e-6, so tests/test_bspline_gpu.py's 2e-3 relative + 1e-6 is asserted as well: the
    smaller of the two holds."""
    from keymorph_amd import ops, synthetic
    from keymorph_amd.utils import align_img
    S, lat, r, d = 16, (5, 5, 5), 1, 2
    from tests import mi_ref
    m, f = mi_ref.smooth_pair((1, 1, S, S, S), 8)
    mat = synthetic.random_affine_matrix(5, "cpu")[:, :3, :].contiguous()
    ctrl = 0.05 * torch.randn(1, 3, *lat, generator=torch.Generator().manual_seed(2))
    c = ctrl.to(DEV).requires_grad_()
    bounds64 = R.bounds_of(m.double(), f.double(), r, d)
    bounds = ops.mind_bounds(m.to(DEV), f.to(DEV), r, d)
    loss = ops.mind_ssc_loss(align_img(ops.bspline_grid(c, (S, S, S), mat.to(DEV)), m.to(DEV)), f.to(DEV), r, d, bounds).sum()
    loss.backward()

    def host(cx, dtype):
        warped = F.grid_sample(m.to(dtype), B.bspline_grid(cx.to(dtype), (S, S, S), mat.to(dtype)), mode="bilinear",
                               padding_mode="border", align_corners=False)
        return R.mind_map(warped, f.to(dtype), r, d, bounds64).mean()
    c64 = ctrl.double().requires_grad_()
    base = host(c64, F64)
    base.backward()
    assert abs(float(base.detach()) - float(loss.detach())) < 1e-5
    picks = torch.topk(c64.grad.abs().reshape(-1), 12).indices.tolist()
    h = 1e-6
    fd = {}
    with torch.no_grad():
        for dtype in (F64, torch.float32):
            for flat in picks:
                vals = []
                for sgn in (1.0, -1.0):
                    cp = ctrl.double().clone()
                    cp.reshape(-1)[flat] += sgn * h
                    vals.append(float(host(cp, dtype)))
                fd[dtype, flat] = (vals[0] - vals[1]) / (2 * h)
    bar = 4 * max(abs(fd[torch.float32, flat] - fd[F64, flat]) for flat in picks)
    for flat in picks:
        got, ref = float(c.grad.reshape(-1)[flat]), fd[F64, flat]
        print(f"ctrl[{flat}]: kernel {got:.6e}  finite difference {ref:.6e}  fp64 autograd {float(c64.grad.reshape(-1)[flat]):.6e}"
              f"  fp32 finite difference {fd[torch.float32, flat]:.6e}  bar {bar:.3e}")
        assert math.isfinite(got) and abs(got - ref) <= min(bar, 2e-3 * abs(ref) + 1e-6), (flat, got, ref, bar)


# ---- the drivers -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inverted():
    """mind_ref.inverted_pair(), validated in tests/test_mind_cpu.py, and register_bspline(metric="mind")'s answer with its
    defaults from the identity matrix."""
    from keymorph_amd.io import register_bspline, voxel_to_mat
    fixed, moving = R.inverted_pair()
    mat = voxel_to_mat(torch.eye(3, device=DEV)[None], torch.zeros(1, 3, device=DEV), fixed.shape[2:])
    return fixed.to(DEV), moving.to(DEV), mat, register_bspline(fixed.to(DEV), moving.to(DEV), mat=mat, metric="mind")


def test_register_bspline_mind_recovers_under_inverted_contrast_and_bias(inverted):
    from keymorph_amd import fields, loss_ops, ops
    from keymorph_amd.io import apply_bspline, register_bspline
    f, m, mat, ctrl = inverted
    dims = tuple(f.shape[2:])
    truth = B.true_ctrl()
    err = float(B.displacement_error(ctrl, truth, dims)[0])
    start = float(B.displacement_error(torch.zeros_like(truth), truth, dims)[0])
    err_mi = float(B.displacement_error(register_bspline(f, m, mat=mat, metric="mi"), truth, dims)[0])
    bounds = ops.mind_bounds(m, f)
    before = float(ops.mind_ssc_loss(apply_bspline(m, torch.zeros_like(ctrl), mat), f, bounds=bounds)[0])
    after = float(ops.mind_ssc_loss(apply_bspline(m, ctrl, mat), f, bounds=bounds)[0])
    print(f"register_bspline(metric='mind'): mean displacement error {err:.3f} voxel (identity {start:.3f}; metric='mi' "
          f"{err_mi:.3f}; fp64 restatement, tests/test_mind_cpu.py: mind {R.RESTATED['mind']:.3f}, mi {R.RESTATED['mi']:.3f}); "
          f"MIND-SSC {before:.5f} -> {after:.5f}")
    assert ctrl.shape == truth.shape and ctrl.dtype == torch.float32
    assert err <= 0.6 * start, (err, start)
    assert err < err_mi, (err, err_mi)
    assert after < before, (after, before)
    assert loss_ops.jdlessthan0(fields.to_displacement(ops.bspline_grid(ctrl, dims, mat))) == 0


def test_register_svf_mind_runs_and_repeats(inverted):
    from keymorph_amd import ops
    from keymorph_amd.io import apply_svf, register_svf
    f, m, mat, _ = inverted
    first = register_svf(f, m, mat=mat, iters=5, metric="mind")
    again = register_svf(f, m, mat=mat, iters=5, metric="mind")
    assert torch.equal(first, again) and torch.isfinite(first).all() and float(first.abs().max()) > 0
    bounds = ops.mind_bounds(m, f)
    before = float(ops.mind_ssc_loss(m, f, bounds=bounds)[0])
    after = float(ops.mind_ssc_loss(apply_svf(m, first, mat), f, bounds=bounds)[0])
    print(f"register_svf(metric='mind', iters=5): MIND-SSC {before:.5f} -> {after:.5f}")
    assert after < before


def test_intensity_registration_mind_entry(inverted):
    """res["mind"] is ops.mind_ssc_loss of the warped pair with the bounds of the UNWARPED pair (img_m, img_f): the clamp the
    driver's finest level used, so the figure is the one the driver minimised."""
    from keymorph_amd import ops
    from keymorph_amd.model import IntensityRegistration
    from keymorph_amd.utils import align_img
    f, m, _, _ = inverted
    with torch.no_grad():
        res = IntensityRegistration(iters=5, bspline_iters=5, metric="mind")(f, m, transform_type=["affine", "bspline", "svf"])
        plain = IntensityRegistration(iters=5, bspline_iters=5)(f, m, transform_type=["affine", "bspline"])
    r = res["bspline"]
    assert set(r) == {"grid", "matrix", "ctrl", "mi", "mind", "time"} and r["mind"].shape == (1,)
    assert set(res["svf"]) == {"grid", "matrix", "ctrl", "mi", "mind", "inverse_grid", "time"}
    assert set(plain["bspline"]) == {"grid", "matrix", "ctrl", "mi", "time"}
    assert set(res["affine"]) == set(plain["affine"]) == {"grid", "matrix", "mi", "time"}
    assert torch.equal(res["affine"]["matrix"], plain["affine"]["matrix"])       # the matrix stages stay on mutual information
    for key in ("bspline", "svf"):
        assert torch.equal(res[key]["mind"], ops.mind_ssc_loss(align_img(res[key]["grid"], m), f, 1, 2, ops.mind_bounds(m, f, 1, 2)))
    with pytest.raises(ValueError):
        IntensityRegistration(metric="ncc")
