"""GPU: ops.local_ncc / loss_ops.LNCCLoss (csrc/lncc.hip) against the fp64 restatement of tests/lncc_ref.py -- value and both
gradients -- and what is built on them (io.register_bspline(metric="lncc"), model.IntensityRegistration(metric="lncc")).

The bars.  d32 = the distance of the restatement evaluated in fp32 on the CPU (direct window sums, each sample recentred by its
first voxel) from its fp64 evaluation: what fp32 costs in any order.  The value is compared absolutely, the gradients in relative
L2 per sample; the kernel gets 4 x the LARGEST d32 over all cases of the table (tests/test_mi_gpu.py's factor for another
summation order; the family maximum keeps a case whose fp32 error happened to cancel from setting an unreachable bar).  Nothing
comes from the kernel.

Measured on an MI355X: see DESIGN.md section 8f."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import bspline_ref as B
from tests import lncc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


def _rel(x, ref):
    return float((x.to(F64) - ref).norm() / ref.norm())


@functools.lru_cache(maxsize=None)
def reference(name):
    """(out64, da64, db64, d32 of the value, d32 of the gradients), computed once per case."""
    a, b, window = R.case_inputs(name)
    o64, da64, db64 = R.evaluate(a, b, window, dtype=F64)
    o32, da32, db32 = R.evaluate(a, b, window, dtype=torch.float32)
    d_val = float((o32.to(F64) - o64).abs().max())
    d_grad = max(_rel(g32[n], g64[n]) for g32, g64 in ((da32, da64), (db32, db64)) for n in range(a.shape[0]))
    return o64, da64, db64, d_val, d_grad


@functools.lru_cache(maxsize=None)
def bars():
    """4 x the largest d32 of the family: (value, gradients)."""
    refs = [reference(name) for name in R.CASES]
    return 4 * max(r[3] for r in refs), 4 * max(r[4] for r in refs)


def run(name, need=(True, True), rows=None):
    from keymorph_amd import ops
    a, b, window = R.case_inputs(name)
    if rows is not None:
        a, b = a[rows], b[rows]
    x, y = a.to(DEV).requires_grad_(need[0]), b.to(DEV).requires_grad_(need[1])
    out = ops.local_ncc(x, y, window)
    out.sum().backward()
    return out.detach(), x.grad, y.grad


@pytest.mark.parametrize("name", list(R.CASES))
def test_value_and_gradients_match_fp64(name):
    o64, da64, db64, d_val, d_grad = reference(name)
    bar_val, bar_grad = bars()
    out, da, db = run(name)
    assert out.shape == o64.shape and out.dtype == torch.float32
    err = float((out.cpu().to(F64) - o64).abs().max())
    print(f"{name}: value {[f'{float(v):.6f}' for v in o64]}  abs error {err:.3e}  d32 {d_val:.3e}  bar {bar_val:.3e}")
    assert math.isfinite(err) and err <= bar_val, (name, err, bar_val)
    for which, g, g64 in (("da", da, da64), ("db", db, db64)):
        assert torch.isfinite(g).all()
        for n in range(g64.shape[0]):
            e = _rel(g[n].cpu(), g64[n])
            print(f"{name}[{n}]: {which} relative L2 {e:.3e}  d32 of the case {d_grad:.3e}  bar {bar_grad:.3e}")
            assert math.isfinite(e) and e <= bar_grad, (name, which, n, e, bar_grad)


def test_constant_windows_score_zero_with_finite_gradients():
    a, b, window = R.case_inputs("masked")
    half, r = a.shape[4] // 2, window // 2
    out, da, db = run("masked")
    # the windows of x < half - r hold zeros alone: cc = 0 there, and nothing of the gradient reaches x < half - 2 r
    assert torch.isfinite(da).all() and torch.isfinite(db).all()
    assert float(da[..., :half - 2 * r].abs().max()) == 0.0 and float(db[..., :half - 2 * r].abs().max()) == 0.0
    zero = torch.zeros_like(a).to(DEV)
    from keymorph_amd import ops
    assert float(ops.local_ncc(zero, zero, window)[0]) == 0.0


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


@pytest.mark.parametrize("name", ["batch", "odd_box_w5", "w15"])
def test_one_gradient_alone_equals_the_same_gradient_of_both(name):
    out, da, db = run(name)
    oa, da_only, none_b = run(name, need=(True, False))
    ob, none_a, db_only = run(name, need=(False, True))
    assert none_a is None and none_b is None
    assert torch.equal(oa, out) and torch.equal(ob, out)
    assert torch.equal(da_only, da) and torch.equal(db_only, db)


def test_lncc_loss_is_minus_the_mean():
    from keymorph_amd import ops
    from keymorph_amd.loss_ops import LNCCLoss
    a, b, _ = R.case_inputs("batch")
    a, b = a.to(DEV), b.to(DEV)
    assert torch.equal(LNCCLoss()(a, b), -ops.local_ncc(a, b).mean())
    assert torch.equal(LNCCLoss(window=5, eps=1e-3)(a, b), -ops.local_ncc(a, b, 5, 1e-3).mean())
    x = a.clone().requires_grad_()
    LNCCLoss()(x, b).backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().sum()) > 0


def test_input_checks():
    from keymorph_amd import _lib, ops
    a = torch.rand(2, 1, 8, 9, 10, device=DEV)
    b = torch.rand(2, 1, 8, 9, 10, device=DEV)
    assert ops.local_ncc(a, b).shape == (2,)
    with pytest.raises(_lib.KeymorphHipError):
        ops.local_ncc(a.cpu(), b)
    with pytest.raises(_lib.KeymorphHipError):
        ops.local_ncc(a, b.cpu())
    with pytest.raises(ValueError):
        ops.local_ncc(a[0], b[0])                                    # wrong rank
    with pytest.raises(ValueError):
        ops.local_ncc(a, b[:, :, :7])                                # mismatched shapes
    with pytest.raises(ValueError):
        ops.local_ncc(a.expand(2, 2, 8, 9, 10), b.expand(2, 2, 8, 9, 10))      # C != 1
    with pytest.raises(ValueError):
        ops.local_ncc(a.double(), b.double())
    for window in (8, 1, 17, 9.5):
        with pytest.raises(ValueError):
            ops.local_ncc(a, b, window)
    with pytest.raises(ValueError):
        ops.local_ncc(a, b, 9, -1.0)
    # the ABI's own limits: -22 before anything is launched
    lib = _lib.load()
    out = torch.empty(2, device=DEV)
    ws = torch.empty(int(lib.kmh_lncc_ws_bytes(2, 8, 9, 10, 9)), dtype=torch.uint8, device=DEV)
    da = torch.empty_like(a)
    p = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    assert lib.kmh_lncc_fwd(p(a), p(b), 2, 8, 9, 10, 9, 1e-5, p(out), p(ws), s) == 0
    assert lib.kmh_lncc_fwd(p(a), p(b), 2, 8, 9, 10, 8, 1e-5, p(out), p(ws), s) == -22       # even
    assert lib.kmh_lncc_fwd(p(a), p(b), 2, 8, 9, 10, 17, 1e-5, p(out), p(ws), s) == -22      # > 15
    assert lib.kmh_lncc_fwd(p(a), p(b), 2, 8, 9, 10, 1, 1e-5, p(out), p(ws), s) == -22
    assert lib.kmh_lncc_fwd(p(a), p(b), 0, 8, 9, 10, 9, 1e-5, p(out), p(ws), s) == -22       # N = 0
    assert lib.kmh_lncc_fwd(p(a), p(b), 2, 8, 0, 10, 9, 1e-5, p(out), p(ws), s) == -22
    assert lib.kmh_lncc_fwd(p(a), p(b), 2, 2048, 1024, 1024, 9, 1e-5, p(out), p(ws), s) == -22      # 2^31 voxels
    assert lib.kmh_lncc_fwd(None, p(b), 2, 8, 9, 10, 9, 1e-5, p(out), p(ws), s) == -22
    assert lib.kmh_lncc_fwd(p(a), None, 2, 8, 9, 10, 9, 1e-5, p(out), p(ws), s) == -22
    assert lib.kmh_lncc_fwd(p(a), p(b), 2, 8, 9, 10, 9, 1e-5, None, p(ws), s) == -22
    assert lib.kmh_lncc_fwd(p(a), p(b), 2, 8, 9, 10, 9, 1e-5, p(out), None, s) == -22
    assert lib.kmh_lncc_bwd(p(a), p(b), p(out), 2, 8, 9, 10, 9, 1e-5, p(da), None, p(ws), s) == 0
    assert lib.kmh_lncc_bwd(p(a), p(b), p(out), 2, 8, 9, 10, 9, 1e-5, None, None, p(ws), s) == 0     # nothing asked for
    assert lib.kmh_lncc_bwd(p(a), p(b), p(out), 2, 8, 9, 10, 6, 1e-5, p(da), None, p(ws), s) == -22
    assert lib.kmh_lncc_bwd(p(a), p(b), p(out), 2, 8, 9, 10, 17, 1e-5, p(da), None, p(ws), s) == -22
    assert lib.kmh_lncc_bwd(p(a), p(b), p(out), 0, 8, 9, 10, 9, 1e-5, p(da), None, p(ws), s) == -22
    assert lib.kmh_lncc_bwd(None, p(b), p(out), 2, 8, 9, 10, 9, 1e-5, p(da), None, p(ws), s) == -22
    assert lib.kmh_lncc_bwd(p(a), p(b), None, 2, 8, 9, 10, 9, 1e-5, p(da), None, p(ws), s) == -22
    assert lib.kmh_lncc_bwd(p(a), p(b), p(out), 2, 8, 9, 10, 9, 1e-5, p(da), None, None, s) == -22
    torch.cuda.synchronize()


def test_gradient_through_align_img_and_bspline_grid_matches_finite_differences():
    """d(-LNCC)/d(ctrl) of the chain bspline_grid -> align_img -> local_ncc at 16^3 against central differences of the fp64
    restatement on the twelve control values that carry most gradient (chosen by the restatement's own autograd), h = 1e-6 as in
    tests/test_bspline_gpu.py (a larger step meets the trilinear blend's kinks).  The bar: the same central difference taken of
    the restatement evaluated in fp32 differs from the fp64 one by what fp32 costs this chain; 4 x the largest of the twelve.
    With a step of 1e-6 the fp32 difference is rounding noise over 2e-6 (measured: bar 1.2e-1 for gradients of 2e-2 .. 3e-2), so
    the bar of tests/test_bspline_gpu.py's test of the same chain under mutual information, 2e-3 relative + 1e-6, is asserted as
    well: the smaller of the two holds.  Measured on an MI355X: the twelve agree with the differences to 1e-8."""
    from keymorph_amd import ops, synthetic
    from keymorph_amd.utils import align_img
    S, lat, window = 16, (5, 5, 5), 9
    from tests import mi_ref
    m, f = mi_ref.smooth_pair((1, 1, S, S, S), 8)
    mat = synthetic.random_affine_matrix(5, "cpu")[:, :3, :].contiguous()
    ctrl = 0.05 * torch.randn(1, 3, *lat, generator=torch.Generator().manual_seed(2))
    c = ctrl.to(DEV).requires_grad_()
    loss = -ops.local_ncc(align_img(ops.bspline_grid(c, (S, S, S), mat.to(DEV)), m.to(DEV)), f.to(DEV), window).sum()
    loss.backward()

    def host(cx, dtype):
        warped = F.grid_sample(m.to(dtype), B.bspline_grid(cx.to(dtype), (S, S, S), mat.to(dtype)), mode="bilinear",
                               padding_mode="border", align_corners=False)
        return -R.lncc_map(warped, f.to(dtype), window).mean()
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


# ---- the driver ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def biased():
    """lncc_ref.biased_pair(), validated in tests/test_lncc_cpu.py, and register_bspline(metric="lncc")'s answer with its defaults
    from the identity matrix."""
    from keymorph_amd.io import register_bspline, voxel_to_mat
    fixed, moving = R.biased_pair()
    mat = voxel_to_mat(torch.eye(3, device=DEV)[None], torch.zeros(1, 3, device=DEV), fixed.shape[2:])
    return fixed.to(DEV), moving.to(DEV), mat, register_bspline(fixed.to(DEV), moving.to(DEV), mat=mat, metric="lncc")


def test_register_bspline_lncc_recovers_under_a_bias_field(biased):
    from keymorph_amd import fields, loss_ops, ops
    from keymorph_amd.io import apply_bspline, register_bspline
    f, m, mat, ctrl = biased
    dims = tuple(f.shape[2:])
    truth = B.true_ctrl()
    err = float(B.displacement_error(ctrl, truth, dims)[0])
    start = float(B.displacement_error(torch.zeros_like(truth), truth, dims)[0])
    err_mi = float(B.displacement_error(register_bspline(f, m, mat=mat, metric="mi"), truth, dims)[0])
    before = float(ops.local_ncc(apply_bspline(m, torch.zeros_like(ctrl), mat), f)[0])
    after = float(ops.local_ncc(apply_bspline(m, ctrl, mat), f)[0])
    print(f"register_bspline(metric='lncc'): mean displacement error {err:.3f} voxel (identity {start:.3f}; metric='mi' "
          f"{err_mi:.3f}; fp64 restatement, tests/test_lncc_cpu.py: lncc {R.RESTATED['lncc']:.3f}, mi {R.RESTATED['mi']:.3f}); "
          f"local NCC {before:.3f} -> {after:.3f}")
    assert ctrl.shape == truth.shape and ctrl.dtype == torch.float32
    assert err <= start / 2, (err, start)
    assert after > before, (after, before)
    assert loss_ops.jdlessthan0(fields.to_displacement(ops.bspline_grid(ctrl, dims, mat))) == 0


def test_intensity_registration_lncc_entry(biased):
    from keymorph_amd import ops
    from keymorph_amd.model import IntensityRegistration
    from keymorph_amd.utils import align_img
    f, m, _, _ = biased
    with torch.no_grad():
        res = IntensityRegistration(iters=5, bspline_iters=5, metric="lncc")(f, m, transform_type=["affine", "bspline"])
        plain = IntensityRegistration(iters=5, bspline_iters=5)(f, m, transform_type=["affine", "bspline"])
    r = res["bspline"]
    assert set(r) == {"grid", "matrix", "ctrl", "mi", "lncc", "time"} and r["lncc"].shape == (1,)
    assert set(plain["bspline"]) == {"grid", "matrix", "ctrl", "mi", "time"}
    assert set(res["affine"]) == set(plain["affine"]) == {"grid", "matrix", "mi", "time"}
    assert torch.equal(res["affine"]["matrix"], plain["affine"]["matrix"])       # the matrix stages stay on mutual information
    assert torch.equal(r["lncc"], ops.local_ncc(align_img(r["grid"], m), f))
    with pytest.raises(ValueError):
        IntensityRegistration(metric="ncc")
