"""GPU: LC2 / ImageLC2 (csrc/lc2.hip through keymorph_amd.loss_ops) against the reference's values and fp32 autograd in
tests/golden/lc2.npz, against the fp64 restatement of tests/test_lc2_cpu.py, and the properties of the kernels themselves:
batch independence, exact zeros outside the crops and their halos, bit-identical repeats, the reference's assertions, and a
gradient through align_img into an affine grid checked by finite differences."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_lc2_cpu import CASES, boxed, case_inputs, fp64_case, lc2_fp64, lc2_pair, rel_l2, support_mask
from tests.util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def module(name, reduction="mean"):
    from keymorph_amd.loss_ops import LC2, ImageLC2
    c = CASES[name]
    if c["patch"] is None:
        return LC2(radiuses=c["radii"])
    return ImageLC2(patch_size=c["patch"], radiuses=c["radii"], reduction=reduction)


def run_case(name, us=None, mr=None):
    """-> forward (LC2: (N,), ImageLC2: scalar mean), d/d(us), d/d(mr) of the reference's cotangent (LC2: ones; ImageLC2: 1)."""
    if us is None:
        us, mr = case_inputs(name)
    u = torch.tensor(us, device=DEV, requires_grad=True)
    m = torch.tensor(mr, device=DEV, requires_grad=True)
    out = module(name)(u, m)
    (out.sum() if CASES[name]["patch"] is None else out).backward()
    return out.detach(), u.grad, m.grad


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_match_reference(name):
    g = golden("lc2.npz")
    out, du, dm = run_case(name)
    assert out.dtype == torch.float32 and du.dtype == torch.float32 and dm.dtype == torch.float32
    du, dm = du.cpu().numpy(), dm.cpu().numpy()
    if CASES[name]["patch"] is None:
        assert out.shape == (CASES[name]["N"],)
        np.testing.assert_allclose(out.cpu().numpy(), g[f"{name}::fwd"], atol=1e-5, rtol=0)
        ref_du, ref_dm = g[f"{name}::dus"], g[f"{name}::dmr"]
    else:
        assert out.shape == ()
        assert abs(float(out) - float(g[f"{name}::fwd_mean"])) <= 1e-5
        us, mr = case_inputs(name)
        none = module(name, None)(torch.tensor(us, device=DEV), torch.tensor(mr, device=DEV))
        assert none.shape == g[f"{name}::fwd_none"].shape
        np.testing.assert_allclose(none.cpu().numpy(), g[f"{name}::fwd_none"], atol=1e-5, rtol=0)
        ref_du, ref_dm, du, dm = g[f"{name}::dus_box"], g[f"{name}::dmr_box"], boxed(du, name), boxed(dm, name)
    assert rel_l2(du, ref_du) < 1e-4 and rel_l2(dm, ref_dm) < 1e-4, (rel_l2(du, ref_du), rel_l2(dm, ref_dm))
    assert np.array_equal(du == 0, ref_du == 0) and np.array_equal(dm == 0, ref_dm == 0)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_match_fp64(name):
    per64, du64, dm64 = fp64_case(name)
    out, du, dm = run_case(name)
    if CASES[name]["patch"] is None:
        np.testing.assert_allclose(out.cpu().numpy(), per64.numpy(), atol=1e-6, rtol=0)
    else:
        assert abs(float(out) - float(per64.mean())) <= 1e-6
        us, mr = case_inputs(name)
        none = module(name, None)(torch.tensor(us, device=DEV), torch.tensor(mr, device=DEV))
        np.testing.assert_allclose(none.cpu().numpy(), per64.numpy(), atol=1e-6, rtol=0)
    assert rel_l2(du.cpu(), du64) < 1e-5 and rel_l2(dm.cpu(), dm64) < 1e-5


def test_batch_equals_stacked_single_samples():
    from keymorph_amd.loss_ops import LC2, ImageLC2
    us, mr = lc2_pair(11, 3, 17, ("plain", "flat", "sat"))
    for mod in (LC2(), ImageLC2(patch_size=17, radiuses=(3, 6), reduction=None)):
        u = torch.tensor(us, device=DEV, requires_grad=True)
        m = torch.tensor(mr, device=DEV, requires_grad=True)
        out = mod(u, m)
        (out * torch.arange(1.0, 4.0, device=DEV)).sum().backward()
        for i in range(3):
            ui = torch.tensor(us[i:i + 1], device=DEV, requires_grad=True)
            mi = torch.tensor(mr[i:i + 1], device=DEV, requires_grad=True)
            oi = mod(ui, mi)
            ((i + 1.0) * oi.sum()).backward()
            assert torch.equal(out[i:i + 1].detach(), oi.detach())
            assert torch.equal(u.grad[i:i + 1], ui.grad) and torch.equal(m.grad[i:i + 1], mi.grad)


@pytest.mark.parametrize("name", ["lc2_s15", "lc2_s17", "img110"])
def test_exact_zeros_outside_crops_and_halos(name):
    _, du, dm = run_case(name)
    outside = torch.tensor(~support_mask(name), device=DEV)
    assert not du[outside].any() and not dm[outside].any()
    assert du[~outside].any() and dm[~outside].any()


def test_patch_order_is_n_d_h_w():
    """Patch (n, pz, py, px) of ImageLC2(reduction=None) is LC2 of that sub-volume."""
    from keymorph_amd.loss_ops import LC2, ImageLC2
    us, mr = lc2_pair(12, 2, 40, ("plain", "plain"))
    u, m = torch.tensor(us, device=DEV), torch.tensor(mr, device=DEV)
    per = ImageLC2(patch_size=19, radiuses=(4,), reduction=None)(u, m)
    assert per.shape == (16,)
    k = 0
    for n in range(2):
        for pz in range(2):
            for py in range(2):
                for px in range(2):
                    sl = (slice(n, n + 1), slice(None), slice(19 * pz, 19 * pz + 19), slice(19 * py, 19 * py + 19),
                          slice(19 * px, 19 * px + 19))
                    assert torch.equal(per[k:k + 1], LC2(radiuses=(4,))(u[sl].contiguous(), m[sl].contiguous()))
                    k += 1


def test_repeat_runs_are_bit_identical():
    for name in ("lc2_s17", "img102"):
        a, b = run_case(name), run_case(name)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_run_method_and_one_input_gradient():
    from keymorph_amd.loss_ops import LC2
    us, mr = case_inputs("lc2_s15")
    u, m = torch.tensor(us, device=DEV), torch.tensor(mr, device=DEV, requires_grad=True)
    got = LC2().run(u, m, 4, alpha=2e-3, beta=0.05)
    want = lc2_fp64(torch.tensor(us).double(), torch.tensor(mr).double(), 15, (4,), 2e-3, 0.05)
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.numpy(), atol=1e-6, rtol=0)
    got.sum().backward()
    assert m.grad is not None and m.grad.abs().sum() > 0


def test_reference_assertions_and_errors():
    from keymorph_amd._lib import KeymorphHipError
    from keymorph_amd.loss_ops import LC2, ImageLC2
    z = lambda *s: torch.zeros(*s, device=DEV)             # noqa: E731
    x15 = z(2, 1, 15, 15, 15)
    with pytest.raises(AssertionError):
        LC2()(x15, z(2, 1, 15, 15, 17))                  # shapes differ
    with pytest.raises(AssertionError):
        LC2()(z(1, 1, 15, 15, 17), z(1, 1, 15, 15, 17))  # not cubic
    with pytest.raises(AssertionError):
        LC2()(z(1, 1, 16, 16, 16), z(1, 1, 16, 16, 16))  # even size
    with pytest.raises(ValueError):
        LC2()(x15, x15)                                  # r = 7 fills S = 15: the reference's crop is empty
    with pytest.raises(ValueError):
        LC2(radiuses=(9,))(x15, x15)
    with pytest.raises(AssertionError):
        ImageLC2(reduction="sum")
    with pytest.raises(AssertionError):
        ImageLC2()(z(1, 2, 60, 60, 60), z(1, 2, 60, 60, 60))   # the reference's odd shape[1] check
    with pytest.raises(AssertionError):
        ImageLC2()(z(1, 1, 60, 60, 61), z(1, 1, 60, 60, 61))
    with pytest.raises(AssertionError):
        ImageLC2()(z(1, 1, 60, 60, 60), z(1, 1, 61, 61, 61))
    with pytest.raises(ValueError):
        ImageLC2()(z(1, 3, 60, 60, 60), z(1, 3, 60, 60, 60))   # odd, but more than one channel
    with pytest.raises(ValueError):
        ImageLC2(patch_size=50)(z(1, 1, 100, 100, 100), z(1, 1, 100, 100, 100))   # 50 - 11 is odd
    with pytest.raises(ValueError):
        ImageLC2()(z(1, 1, 40, 40, 40), z(1, 1, 40, 40, 40))   # no 51^3 patch
    with pytest.raises(KeymorphHipError):
        LC2()(torch.zeros(1, 1, 17, 17, 17), torch.zeros(1, 1, 17, 17, 17))
    # flat inputs: var = 0 < beta, raw value exactly 0 -> 0, finite zero gradients
    x = z(1, 1, 17, 17, 17).requires_grad_()
    out = LC2()(x, x)
    out.sum().backward()
    assert float(out.detach()) == 0.0 and not x.grad.any()


def test_gradient_through_align_img_matches_finite_differences():
    """One backward of ImageLC2()(align_img(grid, us), mr) at 128^3 with an affine grid built by the HIP grid generator;
    d loss / d grid at a few voxels inside crops against central differences of an fp64 host evaluation (F.grid_sample,
    the fp64 restatement), and a finite, non-zero gradient on the affine matrix."""
    from keymorph_amd import ops, synthetic
    from keymorph_amd.loss_ops import ImageLC2
    from keymorph_amd.utils import align_img
    S = 128
    us, mr = lc2_pair(13, 1, S, ("plain",))
    u, m = torch.tensor(us, device=DEV), torch.tensor(mr, device=DEV)
    mat = synthetic.random_affine_matrix(5, DEV)[:, :3, :].contiguous().requires_grad_()
    grid = ops.affine_grid(mat, (S, S, S))
    grid.retain_grad()
    loss = ImageLC2()(align_img(grid, u), m)
    loss.backward()
    assert mat.grad is not None and torch.isfinite(mat.grad).all() and mat.grad.abs().sum() > 0
    g64 = grid.detach().cpu().double()
    u64, m64 = torch.tensor(us).double(), torch.tensor(mr).double()
    warp = lambda gr: F.grid_sample(u64, gr, mode="bilinear", padding_mode="border", align_corners=False)   # noqa: E731
    warped = warp(g64)
    assert abs(float(lc2_fp64(warped, m64, 51, (5,)).mean()) - float(loss)) < 1e-5
    h = 1e-5
    for z, y, x in [(25, 25, 25), (27, 22, 76), (75, 80, 30)]:
        for c in range(3):
            vals = []
            for sgn in (1.0, -1.0):
                gp = g64[:, z:z + 1, y:y + 1, x:x + 1].clone()
                gp[..., c] += sgn * h
                w2 = warped.clone()
                w2[0, 0, z, y, x] = warp(gp)[0, 0, 0, 0, 0]
                vals.append(float(lc2_fp64(w2, m64, 51, (5,)).mean()))
            fd = (vals[0] - vals[1]) / (2 * h)
            got = float(grid.grad[0, z, y, x, c])
            assert math.isfinite(got) and abs(got - fd) <= 2e-3 * abs(fd) + 1e-6, (z, y, x, c, got, fd)
