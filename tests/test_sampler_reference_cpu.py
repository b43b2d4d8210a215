"""CPU: the fp64 sampler reference of tests/sampler_ref.py equals F.grid_sample (ATen grid_sampler_3d, border,
align_corners=False) on every grid of the sampler conformance tests -- so it chooses ATen's cell and ATen's clamp mask at
lattice points and voxel-centre borders, where one ulp of the source coordinate moves floor() or the mask."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import sampler_ref as R

CASES = R.cases()


def _aten(x, grid, gout):
    xt = torch.from_numpy(x).requires_grad_(True)
    gt = torch.from_numpy(grid).requires_grad_(True)
    out = R.ref_grid_sample_cpu(xt, gt)
    (out * torch.from_numpy(gout)).sum().backward()
    return out.detach().numpy(), gt.grad.numpy(), xt.grad.numpy()


@pytest.mark.parametrize("name,x,grid", CASES, ids=[c[0] for c in CASES])
def test_reference_equals_aten(name, x, grid):
    gout = R.cotangent(x, grid, 7)
    out, dgrid, dx = _aten(x, grid, gout)
    R.assert_fwd(out, R.grid_sample(x, grid), x, name)
    R.assert_grid_grad(dgrid, R.grid_sample_bwd_grid(x, grid, gout), x, gout, name)
    scale = R.grid_sample_bwd_input(x.shape, grid, gout, absolute=True)
    assert (np.abs(dx - R.grid_sample_bwd_input(x.shape, grid, gout)) <= 1e-5 * scale).all(), name
    near = R.ref_grid_sample_cpu(x, grid, "nearest").numpy()
    assert np.array_equal(near, R.grid_sample_nearest(x, grid).astype(np.float32)), name


def test_the_lattice_cases_reach_the_kinks():
    """the cases are not vacuous: on the identity grids some source coordinates are exact lattice points and some sit one ulp
    below one (floor picks the lower cell), the border grids hit both clamp boundaries exactly and (at least at the first centre) one ulp inside,
    and the 2x downsampling grid's coordinates are exact half-integers (nearest's rint ties)"""
    g = R.identity(1, (1, 1, 100))[..., 0].ravel()
    c, _ = R.source_coord(g, 100)
    assert (c == np.arange(100)).any() and (c < np.arange(100)).any()
    b = R.border_points(97)
    c, m = R.source_coord(b, 97)
    assert c[1] == 0 and c[4] == 96 and m[1] == 0 and m[4] == 0 and 0 < c[2] < 1 and m[2] == 97 / 2
    c, _ = R.source_coord(R.identity(1, (1, 1, 4))[..., 0].ravel(), 8)
    assert np.array_equal(c, np.arange(4) * 2 + 0.5)


def test_fp32_rounding_of_the_product_matters():
    """a fused multiply-add in ((g + 1) * size - 1) / 2 -- the product not rounded -- moves floor() at some lattice points
    of the W = 100 identity grid: the reference's one-rounding-per-operation is load-bearing"""
    g = R.identity(1, (1, 1, 100))[..., 0].ravel().astype(np.float32)
    exact = ((g.astype(np.float64) + 1.0) * 100 - 1.0)          # the fused product (exact in fp64), then one rounding
    fused = (exact.astype(np.float32) / np.float32(2)).astype(np.float64)
    rounded, _ = R.source_coord(g, 100)
    assert (np.floor(fused) != np.floor(rounded)).any()


def test_nan_coordinate_follows_aten():
    """the documented NaN rule (sampler_taps.h header): ATen's forward samples a NaN coordinate at the far border of its axis,
    and its backward gives such a voxel a zero grid gradient on all three axes and sends nothing to the input"""
    rng = np.random.default_rng(3)
    x = rng.random((1, 2, 3, 4, 5), dtype=np.float32)
    grid = R.identity(1, (3, 4, 5))
    grid[0, 1, 2, 3, 0] = np.nan
    grid[0, 2, 0, 1, 1] = np.nan
    grid[0, 0, 3, 4, 2] = np.nan
    gout = R.cotangent(x, grid, 4)
    out, dgrid, dx = _aten(x, grid, gout)
    R.assert_fwd(out, R.grid_sample(x, grid), x)
    R.assert_grid_grad(dgrid, R.grid_sample_bwd_grid(x, grid, gout), x, gout)
    scale = R.grid_sample_bwd_input(x.shape, grid, gout, absolute=True)
    assert (np.abs(dx - R.grid_sample_bwd_input(x.shape, grid, gout)) <= 1e-5 * scale).all()
    assert np.array_equal(out[0, :, 1, 2, 3], x[0, :, 1, 2, 4])
    assert np.array_equal(out[0, :, 2, 0, 1], x[0, :, 2, 3, 1]) and np.array_equal(out[0, :, 0, 3, 4], x[0, :, 2, 3, 4])
    ref = R.grid_sample_bwd_grid(x, grid, gout)
    assert (ref[0, 1, 2, 3] == 0).all() and (ref[0, 2, 0, 1] == 0).all() and (ref[0, 0, 3, 4] == 0).all()


def test_loss_references():
    """the fp64 MSE and Dice rows (and their cotangents) against autograd of the same expressions in fp64"""
    rng = np.random.default_rng(6)
    p, t = rng.random((2, 3, 4, 5, 6)), rng.random((2, 3, 4, 5, 6))
    pt = torch.from_numpy(p).requires_grad_(True)
    l = ((pt - torch.from_numpy(t)) ** 2).mean()
    l.backward()
    val, cot = R.mse(p, t)
    assert abs(val - l.item()) <= 1e-15 and np.allclose(cot, pt.grad.numpy(), rtol=1e-13, atol=0)
    g = rng.standard_normal((2, 3))
    pt = torch.from_numpy(p).requires_grad_(True)
    tt = torch.from_numpy(t)
    num = 2 * (tt * pt).sum((2, 3, 4)) + 1
    den = (pt * pt).sum((2, 3, 4)) + (tt * tt).sum((2, 3, 4)) + 1
    rows = 1 - num / den
    (rows * torch.from_numpy(g)).sum().backward()
    r, cot = R.dice_rows(p, t, g)
    assert np.allclose(r, rows.detach().numpy(), rtol=1e-14, atol=0)
    assert np.allclose(cot, pt.grad.numpy(), rtol=1e-12, atol=1e-16)
