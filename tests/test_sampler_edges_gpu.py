"""GPU: the sampler kernels (csrc/sampler.hip, warp_dice.hip, losses.hip) against the fp64 reference of tests/sampler_ref.py at lattice points, clamp
borders, non-finite coordinates and the shape edges that pick each kernel arm.

Bars (against fp64, whose coordinate is ATen's fp32 one): forward 1e-6 * max|x|; grid gradient per axis
1e-5 * C * (size / 2) * max|x| * max|gout|; input gradient 1e-5 of the summed |weights * gout| per voxel; nearest exact;
losses 1e-6 relative.  A gradient taken in the neighbouring cell, or a flipped clamp mask, misses the grid bar by orders of
magnitude.  The environment switches of the library are read once per process, so their arms run in child processes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()


def _np(t):
    return t.detach().cpu().numpy()


def _run_sampler(x, grid, gout):
    from keymorph_amd import ops
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    gd = torch.from_numpy(grid).to(DEV).requires_grad_(True)
    out = ops.grid_sample3d(xd, gd)
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    near = ops.grid_sample3d(xd.detach(), gd.detach(), "nearest")
    return _np(out), _np(gd.grad), _np(xd.grad), _np(near)


def _check_sampler(name, x, grid, gout, out, dgrid, dx, near, input_grad=True):
    R.assert_fwd(out, R.grid_sample(x, grid), x, name)
    R.assert_grid_grad(dgrid, R.grid_sample_bwd_grid(x, grid, gout), x, gout, name)
    if input_grad:
        scale = R.grid_sample_bwd_input(x.shape, grid, gout, absolute=True)
        err = np.abs(dx - R.grid_sample_bwd_input(x.shape, grid, gout))
        assert (err <= 1e-5 * scale).all(), f"{name}: input gradient error {float((err - 1e-5 * scale).max()):.3e} over the bar"
    ref = R.grid_sample_nearest(x, grid).astype(np.float32)
    assert np.array_equal(near, ref), f"{name}: nearest differs at {int((near != ref).sum())} values"


@pytest.mark.parametrize("name,x,grid", CASES, ids=[c[0] for c in CASES])
def test_grid_sample3d_vs_fp64(name, x, grid):
    """ops.grid_sample3d, bilinear and nearest: forward, d/d(grid), d/d(volume)"""
    gout = R.cotangent(x, grid, 11)
    _check_sampler(name, x, grid, gout, *_run_sampler(x, grid, gout))


def test_multichannel_kernel_is_bit_equal_to_channel_by_channel():
    """the C >= 2 tiled kernel blends the same corner values as the single-channel one: bit-equal on lattice grids too"""
    from keymorph_amd import ops
    for name, x, grid in CASES:
        if x.shape[1] < 2 or x.shape[1] > 16:
            continue
        xd, gd = torch.from_numpy(x).to(DEV), torch.from_numpy(grid).to(DEV)
        out = ops.grid_sample3d(xd, gd)
        for c in range(x.shape[1]):
            assert torch.equal(out[:, c:c + 1], ops.grid_sample3d(xd[:, c:c + 1].contiguous(), gd)), (name, c)


@pytest.mark.parametrize("W", [100, 97])
def test_align_img_4d_route(W):
    """utils.align_img of (N, C, H, W) with an (N, Ho, Wo, 2) grid: a depth-1 volume sampled at z = 0"""
    from keymorph_amd import utils
    rng = np.random.default_rng(W)
    x = rng.random((2, 3, 7, W), dtype=np.float32) + np.float32(0.25)
    g3 = R.identity(2, (1, 7, W))
    g3[1, ..., :2] = rng.random((1, 7, W, 2), dtype=np.float32) * np.float32(2.4) - np.float32(1.2)
    g3[..., 2] = 0
    g2 = np.ascontiguousarray(g3[:, 0, ..., :2])
    gout = rng.standard_normal((2, 3, 7, W)).astype(np.float32)
    gd = torch.from_numpy(g2).to(DEV).requires_grad_(True)
    out = utils.align_img(gd, torch.from_numpy(x).to(DEV))
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    x3 = x[:, :, None]
    R.assert_fwd(_np(out), R.grid_sample(x3, g3)[:, :, 0], x3)
    ref = R.grid_sample_bwd_grid(x3, g3, gout[:, :, None])[:, 0]
    R.assert_grid_grad(np.concatenate([_np(gd.grad), ref[..., 2:]], -1), ref, x3, gout[:, :, None])
    near = utils.align_img(gd.detach(), torch.from_numpy(x).to(DEV), "nearest")
    assert np.array_equal(_np(near), R.grid_sample_nearest(x3, g3)[:, :, 0].astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ losses
MSE_CASES = [c for c in CASES if c[1].shape[1] <= 14]


def _check_warp_mse(name, x, grid, fixed, loss, warped, dgrids):
    p = R.grid_sample(x, grid)
    val, cot = R.mse(p, fixed)
    assert abs(loss - val) <= 1e-6 * val, f"{name}: loss {loss} vs {val}"
    R.assert_fwd(warped, p, x, name)
    ref = R.grid_sample_bwd_grid(x, grid, cot)
    for k, dg in enumerate(dgrids):
        R.assert_grid_grad(dg, ref, x, cot, f"{name} backward {k}")


def _run_warp_mse(x, grid, fixed):
    """the first backward hands out the gradient of the fused pass (when the shape allows it); the second, over the retained
    graph, recomputes it through the separate MSE-backward and grid-backward kernels"""
    from keymorph_amd import ops
    gd = torch.from_numpy(grid).to(DEV).requires_grad_(True)
    loss, warped = ops.warp_mse(torch.from_numpy(x).to(DEV), gd, torch.from_numpy(fixed).to(DEV))
    loss.backward(retain_graph=True)
    g1 = _np(gd.grad)
    gd.grad = None
    loss.backward()
    return loss.item(), _np(warped), [g1, _np(gd.grad)]


@pytest.mark.parametrize("name,x,grid", MSE_CASES, ids=[c[0] for c in MSE_CASES])
def test_warp_mse_vs_fp64(name, x, grid):
    """ops.warp_mse: loss, warped volume and d(loss)/d(grid) of the fused single pass (N * ovox % 4 == 0 and W >= 2) or of
    the fallback launches, and of the recomputing second backward"""
    fixed = np.random.default_rng(5).random(x.shape[:2] + grid.shape[1:4], dtype=np.float32)
    _check_warp_mse(name, x, grid, fixed, *_run_warp_mse(x, grid, fixed))


def _onehot(N, C, shape, rng):
    lab = rng.integers(0, C, (N,) + tuple(shape))
    return np.ascontiguousarray(np.moveaxis(np.eye(C, dtype=np.float32)[lab], -1, 1))


def _check_warp_dice(name, x, grid, fixed, loss, dgrid):
    p = R.grid_sample(x, grid)
    N, C = x.shape[:2]
    g = np.full((N, C), 1.0 / (N * C))
    rows, cot = R.dice_rows(p, fixed, g)
    val = float(rows.mean())
    # (relative to the ratio (2 I + 1) / (P + T + 1) the loss is 1 minus: the loss itself is 0 where the two agree)
    assert abs(loss - val) <= 1e-6 * max(abs(val), abs(1.0 - val)), f"{name}: Dice loss {loss} vs {val}"
    R.assert_grid_grad(dgrid, R.grid_sample_bwd_grid(x, grid, cot), x, R.dice_cot_scale(p, fixed, g), name)


def _run_warp_dice(x, grid, fixed, seg_grad=False):
    from keymorph_amd import loss_ops
    gd = torch.from_numpy(grid).to(DEV).requires_grad_(True)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(seg_grad)
    loss = loss_ops.warp_dice_loss(gd, xd, torch.from_numpy(fixed).to(DEV))
    loss.backward()
    return loss.item(), _np(gd.grad)


DICE_CASES = [("identity_W100", (1, 3, 4, 100), "identity"), ("shift_W97_N3", (3, 5, 4, 97), "shift"),
              ("down2", (1, 7, 8, 12), "down"), ("border_ovox105", (2, 5, 6, 7), "border"),
              ("random_ovox45", (3, 6, 7, 8), "random"), ("W2_H1_D1", (1, 1, 1, 2), "random")]


def _dice_grid(kind, N, shape, rng):
    if kind == "identity":
        return R.identity(N, shape)
    if kind == "shift":
        return R.shift(R.identity(N, shape), shape, (2, -1, 1))
    if kind == "down":
        return R.identity(N, tuple(s // 2 for s in shape))
    if kind == "border":
        return R.border_grid(N, shape, (3, 5, 7), 3)
    out = (3, 3, 5) if shape[0] > 1 else (1, 1, 7)
    return rng.random((N,) + out + (3,), dtype=np.float32) * np.float32(2.6) - np.float32(1.3)


@pytest.mark.parametrize("C", [1, 3, 4, 14])
@pytest.mark.parametrize("name,shape,kind", DICE_CASES, ids=[c[0] for c in DICE_CASES])
def test_warp_dice_vs_fp64(name, shape, kind, C):
    """loss_ops.warp_dice_loss: fused float arm (soft segmentations, and one-hot at C < 4), label arm (one-hot, C >= 4),
    and the align_img + DiceLoss fallback (the moving segmentation needs a gradient)"""
    rng = np.random.default_rng(C)
    N, shp = shape[0], shape[1:]
    grid = _dice_grid(kind, N, shp, rng)
    oshape = grid.shape[1:4]
    for arm in ("soft", "onehot", "fallback"):
        if arm == "soft":
            x, fixed = rng.random((N, C) + shp, dtype=np.float32), rng.random((N, C) + oshape, dtype=np.float32)
        else:
            x, fixed = _onehot(N, C, shp, rng), _onehot(N, C, oshape, rng)
        _check_warp_dice(f"{name} C={C} {arm}", x, grid, fixed, *_run_warp_dice(x, grid, fixed, arm == "fallback"))


def test_warp_dice_channel_and_row_boundaries():
    """the fused kernels serve C <= 128 and N * C <= 65536 rows; C = 129 and N * C = 65537 take align_img + DiceLoss"""
    from keymorph_amd import ops
    rng = np.random.default_rng(17)
    for N, C, shp in ((1, 128, (3, 4, 6)), (1, 129, (3, 4, 6)), (512, 128, (1, 1, 2)), (1, 65537, (1, 1, 2))):
        x = rng.random((N, C) + shp, dtype=np.float32)
        fixed = rng.random((N, C) + shp, dtype=np.float32)
        grid = np.ascontiguousarray(np.broadcast_to(R.identity(1, shp), (N,) + shp + (3,)))
        grid = grid + (rng.random(grid.shape, dtype=np.float32) - np.float32(0.5)) * np.float32(0.3)
        fused = C <= 128 and N * C <= 65536
        assert ops.warp_dice_ok(torch.from_numpy(x).to(DEV), torch.from_numpy(grid).to(DEV)) == fused, (N, C)
        _check_warp_dice(f"N={N} C={C}", x, grid, fixed, *_run_warp_dice(x, grid, fixed))


@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 9), (1, 1, 1, 1, 1), (1, 1, 1, 1, 2), (1, 1, 1, 1, 3), (3, 4, 1, 1, 1),
                                   (1, 2, 16, 16, 16)])
def test_mse_loss_and_dice_rows_vs_fp64(shape):
    """ops.mse_loss and ops.dice_rows with their gradients, numel % 4 in {0, 1, 2, 3}"""
    from keymorph_amd import ops
    rng = np.random.default_rng(sum(shape))
    a, b = rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32)
    ad = torch.from_numpy(a).to(DEV).requires_grad_(True)
    l = ops.mse_loss(ad, torch.from_numpy(b).to(DEV))
    (l * 3.0).backward()
    val, cot = R.mse(a, b)
    assert abs(l.item() - val) <= 1e-6 * val
    assert np.allclose(_np(ad.grad), 3.0 * cot, rtol=1e-6, atol=1e-6 * float(np.abs(cot).max()))
    N, C = shape[:2]
    ad = torch.from_numpy(a.reshape(N * C, -1)).to(DEV).requires_grad_(True)
    rows = ops.dice_rows(ad, torch.from_numpy(b.reshape(N * C, -1)).to(DEV))
    g = rng.standard_normal(N * C).astype(np.float32)
    (rows * torch.from_numpy(g).to(DEV)).sum().backward()
    ref, cot = R.dice_rows(a.reshape(N, C, -1), b.reshape(N, C, -1), g.reshape(N, C))
    assert (np.abs(_np(rows) - ref.reshape(-1)) <= 1e-6 * np.maximum(np.abs(ref), np.abs(1 - ref)).reshape(-1)).all()
    assert np.allclose(_np(ad.grad), cot.reshape(N * C, -1), rtol=1e-5, atol=1e-6 * float(np.abs(cot).max()))


# ------------------------------------------------------------------------------------------------------------ NaN
def test_nan_coordinates():
    """a NaN coordinate follows ATen's CPU kernels (sampler_taps.h header): the forward clamps it to the far border of its axis,
    the voxel passes no gradient to the grid or the volume; every other voxel is unaffected -- through the lane-contiguous
    (C = 1), tiled multi-channel (C = 2, 14), plain (W = 1) kernels and the fused losses"""
    from keymorph_amd import loss_ops
    rng = np.random.default_rng(23)
    for N, C, shp in ((1, 1, (6, 7, 100)), (2, 2, (9, 9, 9)), (1, 14, (5, 6, 97)), (1, 2, (5, 6, 1))):
        x = rng.random((N, C) + shp, dtype=np.float32) + np.float32(0.25)
        grid = R.identity(N, shp)
        nan_at = [(0, 1, 2, 0, 0), (0, 2, 0, 0, 1), (N - 1, 3, 4, 0, 2), (N - 1, 0, 0, 0, 0)]
        for i in nan_at:
            grid[i] = np.nan
        gout = R.cotangent(x, grid, 3)
        out, dgrid, dx, near = _run_sampler(x, grid, gout)
        _check_sampler(f"NaN {shp} C={C}", x, grid, gout, out, dgrid, dx, near)
        for n, z, y, xx, k in nan_at:
            assert (dgrid[n, z, y, xx] == 0).all()
        clean = ~np.isnan(grid).any(-1)
        base = R.identity(N, shp)
        ref_clean = R.grid_sample(x, base)
        assert np.abs(out - ref_clean).max(1)[clean].max() <= 1e-6 * float(x.max())
        fixed = rng.random(x.shape, dtype=np.float32)
        _check_warp_mse(f"NaN warp_mse {shp}", x, grid, fixed, *_run_warp_mse(x, grid, fixed))
        if shp[2] >= 2:
            gd = torch.from_numpy(grid).to(DEV).requires_grad_(True)
            loss = loss_ops.warp_dice_loss(gd, torch.from_numpy(x).to(DEV), torch.from_numpy(fixed).to(DEV))
            loss.backward()
            _check_warp_dice(f"NaN Dice {shp}", x, grid, fixed, loss.item(), _np(gd.grad))


# ------------------------------------------------------------------------------------------------------------ env arms
ARMS = {
    "lc_wdilp2_dense": {"KMH_SAMPLER_MC": "0", "KMH_WD_ILP_A": "2", "KMH_WD_ILP_B": "2", "KEYMORPH_DICE_NO_LABELS": "1"},
    "mc2_minc1": {"KMH_SAMPLER_MC": "2", "KMH_SAMPLER_MC_MINC": "1"},
    "mc4_nobox_minc1": {"KMH_SAMPLER_BOX": "0", "KMH_SAMPLER_MC_MINC": "1"},
    "old": {"KMH_SAMPLER_OLD": "1"},
    "walk": {"KMH_WD_BLOCKS": "8", "KMH_MC_BLOCKS": "8"},
}
ARM_CASES = ["identity_W100_C1", "identity_H97_C2", "shift_W97_C14", "xz_flip_W100_C2", "down2_N3_C1", "border_C2_ovox105",
             "beyond_C3_ovox15", "steep_affine_C2", "random_N3_C4_ovox45"]


def _arm_inputs():
    byname = {n: (x, g) for n, x, g in CASES}
    rng = np.random.default_rng(99)
    out = []
    for n in ARM_CASES:
        x, g = byname[n]
        out.append((n, x, g, R.cotangent(x, g, 13), rng.random(x.shape[:2] + g.shape[1:4], dtype=np.float32)))
    return out


def _dice_inputs():
    rng = np.random.default_rng(98)
    out = []
    for C in (3, 14):
        x, f = _onehot(2, C, (5, 6, 97), rng), _onehot(2, C, (5, 6, 97), rng)
        out.append((f"onehot{C}", x, R.shift(R.identity(2, (5, 6, 97)), (5, 6, 97), (1, 0, -1)), f))
    x, f = rng.random((1, 4, 4, 5, 100), dtype=np.float32), rng.random((1, 4, 4, 5, 100), dtype=np.float32)
    out.append(("soft4", x, R.identity(1, (4, 5, 100)), f))
    return out


# The "walk" arm: 8 persistent blocks per sample row over 10 x 16 x 100 = 16 000 output voxels.  The Dice kernels see 16 chunks
# of 1024 voxels, the last one ragged (640): every block walks two consecutive chunks, so the register prefetch of the next
# chunk runs, and the block that owns chunks 14 and 15 steps from a prefetched full chunk to the element-wise tail.  The
# multi-channel kernel sees 7 x 2 x 2 = 28 tiles of 16 x 8 x 8, three or four per block: tx = 0..5 fast (Wo % 4 == 0), tx = 6
# an edge tile.  No default-sized case makes a block take more than one chunk or tile.
WALK_SHAPE = (10, 16, 100)


def _walk_inputs():
    """(sampler cases, Dice cases) of the walk arm: C = 2 under a mild rotation about z (the tiles' source boxes fit the LDS
    box), and the three Dice arms on a shifted identity"""
    rng = np.random.default_rng(97)
    N, shp = 2, WALK_SHAPE
    theta = torch.zeros(N, 3, 4)
    for n, a in enumerate((0.08, -0.05)):
        theta[n] = torch.tensor([[np.cos(a), -np.sin(a), 0, 0.01], [np.sin(a), np.cos(a), 0, -0.02], [0, 0, 1, 0]])
    rot = torch.nn.functional.affine_grid(theta, (N, 1) + shp, align_corners=False).numpy()
    x = rng.random((N, 2) + shp, dtype=np.float32) + np.float32(0.25)
    sampler = [("walk_rot_C2", x, rot, R.cotangent(x, rot, 13), None)]
    grid = R.shift(R.identity(N, shp), shp, (1, 0, -1))
    dice = [(f"walk_onehot{C}", _onehot(N, C, shp, rng), grid, _onehot(N, C, shp, rng)) for C in (3, 14)]
    dice.append(("walk_soft4", rng.random((N, 4) + shp, dtype=np.float32), grid, rng.random((N, 4) + shp, dtype=np.float32)))
    return sampler, dice


def _inputs(arm):
    return _walk_inputs() if arm == "walk" else (_arm_inputs(), _dice_inputs())


def child_main(path, arm=None):
    """one environment arm (set by the parent before this process started): every sampler entry point on the arm's cases
    (fixed is None: no warp + MSE)"""
    res = {}
    sampler, dice = _inputs(arm)
    for n, x, g, gout, fixed in sampler:
        out, dgrid, dx, near = _run_sampler(x, g, gout)
        res.update({f"{n}/out": out, f"{n}/dgrid": dgrid, f"{n}/dx": dx, f"{n}/near": near})
        if fixed is None:
            continue
        loss, warped, (g1, g2) = _run_warp_mse(x, g, fixed)
        res.update({f"{n}/mse": np.float64(loss), f"{n}/warped": warped, f"{n}/mse_g1": g1, f"{n}/mse_g2": g2})
    for n, x, g, f in dice:
        loss, dgrid = _run_warp_dice(x, g, f)
        res.update({f"{n}/dice": np.float64(loss), f"{n}/dice_g": dgrid})
    np.savez(path, **res)


def test_environment_arms(tmp_path):
    """KMH_SAMPLER_MC=0|2, KMH_SAMPLER_BOX=0, KMH_SAMPLER_MC_MINC=1, KMH_SAMPLER_OLD=1, KMH_WD_ILP_A/B=2,
    KEYMORPH_DICE_NO_LABELS=1 and KMH_WD_BLOCKS=KMH_MC_BLOCKS=8 (on the walk inputs), each arm in a fresh child process, one
    after another, stopping at the first that fails"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import test_sampler_edges_gpu as m\n"
            "m.child_main(sys.argv[1], sys.argv[2])\n" % ROOT)
    keep = {k: v for k, v in os.environ.items() if not (k.startswith("KMH_") or k == "KEYMORPH_DICE_NO_LABELS")}
    for arm, env in ARMS.items():
        path = str(tmp_path / f"{arm}.npz")
        r = subprocess.run([sys.executable, "-c", code, path, arm], env=dict(keep, **env), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, f"arm {arm} exited with {r.returncode}:\n{r.stderr[-3000:]}"
        got = np.load(path)
        sampler, dice = _inputs(arm)
        for n, x, g, gout, fixed in sampler:
            what = f"{arm}: {n}"
            _check_sampler(what, x, g, gout, got[f"{n}/out"], got[f"{n}/dgrid"], got[f"{n}/dx"], got[f"{n}/near"])
            if fixed is not None:
                _check_warp_mse(what, x, g, fixed, float(got[f"{n}/mse"]), got[f"{n}/warped"],
                                [got[f"{n}/mse_g1"], got[f"{n}/mse_g2"]])
        for n, x, g, f in dice:
            _check_warp_dice(f"{arm}: {n}", x, g, f, float(got[f"{n}/dice"]), got[f"{n}/dice_g"])
