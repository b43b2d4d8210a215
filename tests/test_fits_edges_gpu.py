"""GPU: the closed-form stage (csrc/fits.hip affine_fit, rigid_fit, affine_inverse, com3d; csrc/grids.hip affine_points) against
the fp64 restatement of tests/fits_ref.py at reflections, equal singular values, rank edges, real-world offsets, every weighting
and the K / N / P that change a kernel's path.  tests/test_fits_reference_cpu.py pins the restatement and the case classes.

Bars.  Fits and inverse compute in fp64 from fp32 inputs and round once: |got - truth| <= 8 eps32 max|truth| + 8 floor, the
floor measured on the CPU from the restatement alone (fits_ref's docstring).  The truth of a gradient is fp64 autograd of
the oracle, or central differences of the restatement on the exactly symmetric clouds, where autograd is not finite.
affine_inverse's backward reads the fp32-rounded inverse: max(8 eps32 max|truth|, 1.25 x the error of fp32 torch.inverse
autograd on the CPU).  affine_points is fp32 arithmetic; with u = eps32 / 2 its bars are the running-error bounds of its sums:
forward 8 u (|M| |p| + |t|) for 7 roundings, dpts 6 u |M|^T |g|, dM (ceil(P / 256) + 3) 2 u sum |g| |p| (a thread adds
ceil(P / 256) fp32 products, the block sum is fp64, one rounding on the store).  com3d is fp32 arithmetic against the fp32
oracle's own error: forward max(8 eps32, 1.25 x), backward max(16 eps32 max|truth|, 2 x).

Classes B and C (rank <= 2) assert properties only: the reference's output there hangs on LAPACK's sign of a null vector.
"""
import zlib

import numpy as np
import pytest
import torch

from oracle import keymorph_oracle as O
from tests import fits_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = R.EPS32
CASES = R.fit_cases()
FIT_PARAMS = [(k, c) for c in CASES for k in c["kinds"]]


def _ops():
    from keymorph_amd import ops
    return ops


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _run_fit(kind, x, y, w, cot):
    """batched (N, K, 3) float32 arrays -> M, dx, dy, dw as tensors on the device"""
    fit = _ops().affine_fit if kind == "affine" else _ops().rigid_fit
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(True)      # noqa: E731
    xd, yd, wd = t(x), t(y), t(w)
    M = fit(xd, yd, wd)
    (M * torch.from_numpy(cot).to(DEV)).sum().backward()
    return M.detach(), xd.grad, yd.grad, None if wd is None else wd.grad


def _check(tag, got, truth, floor=0.0):
    err, bar = float(np.abs(got - truth).max()), R.bound(truth, floor)
    print(f"{tag}: error {err:.3e}, bar {bar:.3e} (floor {floor:.1e})")
    assert np.isfinite(got).all() and err <= bar, f"{tag}: error {err:.3e} over the bar {bar:.3e}"


def _check_sample(tag, kind, x, y, w, cot, mode, got):
    M, floor, grads, gfloors = R.fit_truth(kind, x, y, w, cot, mode)
    _check(f"{tag} M", got[0], M, floor)
    for nm, g, t, f in zip(("dx", "dy", "dw"), got[1:], grads, gfloors):
        if t is not None:
            _check(f"{tag} {nm}", g, t, f)


@pytest.mark.parametrize("kind,case", FIT_PARAMS, ids=[f"{k}-{c['name']}" for k, c in FIT_PARAMS])
def test_fit_class_a_vs_fp64(kind, case):
    """class A, N = 1: M, dx, dy (and dw where weighted) against fp64.  Observed on gfx950 (worst over the table, in units of
    eps32 max|truth|): affine M 0.48, dx 0.45, dy 0.44; rigid M 0.48, dx 0.50, dy 0.46, dw 0.45 -- one rounding of an fp64
    result.  Affine at offset 1000, where the floor carries the bar: dx 0.37, dw 0.46 of the bar."""
    cot = R.cotangent(zlib.crc32(case["name"].encode()))
    x, y, w = case["x"], case["y"], case["w"]
    got = _run_fit(kind, x[None], y[None], None if w is None else w[None], cot[None])
    _check_sample(f"{kind} {case['name']}", kind, x, y, w, cot, case["grad"], [None if g is None else _np(g)[0] for g in got])
    if case["note"] == "affine interpolates" and kind == "affine":
        res = np.abs(R.affine_points(_np(got[0])[0], x) - y).max()
        assert res <= 8 * EPS * np.abs(y).max(), res


@pytest.mark.parametrize("kind", ["affine", "rigid"])
def test_fit_batch_of_37_is_bit_identical_to_one_at_a_time(kind):
    """N = 37 at K = 64 mixing every class-A cloud: each sample against fp64, and the batch bit-identical to 37 launches of N = 1
    (one workgroup per sample: nothing of a sample may depend on its neighbours)"""
    x, y, w, modes, names = R.batch_case()
    cot = R.cotangent(370, (37, 3, 4))
    got = _run_fit(kind, x, y, w, cot)
    for n in range(37):
        one = _run_fit(kind, x[n:n + 1], y[n:n + 1], w[n:n + 1], cot[n:n + 1])
        for nm, a, b in zip(("M", "dx", "dy", "dw"), got, one):
            assert torch.equal(a[n:n + 1], b), f"{kind} {names[n]} (sample {n}) {nm}: the batch differs from the single launch"
        _check_sample(f"{kind} batch[{n}] {names[n]}", kind, x[n], y[n], w[n], cot[n], modes[n], [_np(g)[n] for g in got])


def _rigid_properties(c):
    x, y, w = c["x"], c["y"], c["w"]
    cot = R.cotangent(9)
    M, dx, dy, dw = (None if g is None else _np(g)[0] for g in
                     _run_fit("rigid", x[None], y[None], None if w is None else w[None], cot[None]))
    assert np.isfinite(M).all(), c["name"]
    Rm = M[:, :3].astype(np.float64)
    orth = np.abs(Rm @ Rm.T - np.eye(3)).sum(1).max()
    c1, c2 = R.rigid_centroids(x, y, w)
    t_err = np.abs(M[:, 3] - (c2 - Rm @ c1)).max()
    t_bar = 8 * EPS * max(1.0, np.abs(c2).max() + np.abs(c1).sum())
    print(f"{c['name']}: |R R^T - I|_inf {orth:.2e}, det {np.linalg.det(Rm):+.6f}, T error {t_err:.2e} (bar {t_bar:.2e})")
    assert orth <= 8 * EPS, (c["name"], orth)
    assert t_err <= t_bar, (c["name"], t_err)
    for g in (dx, dy, dw):
        assert g is None or np.isfinite(g).all(), c["name"]
    return Rm


CLASS_B = [c for c in R.property_cases() if c["cls"] == "B"]
CLASS_C = [c for c in R.property_cases() if c["cls"] == "C"]


@pytest.mark.parametrize("case", CLASS_B, ids=[c["name"] for c in CLASS_B])
def test_rigid_rank2_properties(case):
    """class B (svd3's rank <= 2 completion): finite, orthogonal, proper, T consistent, and as good as the proper optimum"""
    Rm = _rigid_properties(case)
    assert np.linalg.det(Rm) > 0, case["name"]
    obj, scale = R.rigid_objective(Rm, case["x"], case["y"], case["w"])
    best, _ = R.rigid_objective(R.kabsch_proper(case["x"], case["y"], case["w"])[:, :3], case["x"], case["y"], case["w"])
    print(f"{case['name']}: objective {obj:.6e}, proper optimum {best:.6e}, scale {scale:.3e}")
    assert abs(obj - best) <= 1e-6 * scale, (case["name"], obj, best)


@pytest.mark.parametrize("case", CLASS_C, ids=[c["name"] for c in CLASS_C])
def test_rigid_rank1_properties(case):
    """class C (svd3's rank <= 1 completion, K = 1 and K = 2 under one wavefront): finite, orthogonal, T consistent"""
    _rigid_properties(case)


# ------------------------------------------------------------------------------------------------------------ inverse
INV = R.inverse_cases()


@pytest.mark.parametrize("name,M", INV, ids=[c[0] for c in INV])
def test_affine_inverse_vs_fp64(name, M):
    """N in {1, 64, 65} (one 64-thread block, and one thread into the second).  Observed on gfx950: forward <= 0.5 eps32
    max|truth|; backward 0.05 .. 0.13 of the bar (the fp32 torch.inverse band carries it on the scaled matrices)"""
    N = M.shape[0]
    cot = R.cotangent(N, (N, 3, 4))
    Md = torch.from_numpy(M).to(DEV).requires_grad_(True)
    out = _ops().affine_inverse(Md)
    (out * torch.from_numpy(cot).to(DEV)).sum().backward()
    out, dM = _np(out), _np(Md.grad)
    M32 = torch.from_numpy(M).requires_grad_(True)
    (torch.inverse(O.square(M32))[:, :3] * torch.from_numpy(cot)).sum().backward()
    worst = 0.0
    for n in range(N):
        _check(f"{name}[{n}] inverse", out[n], R.affine_inverse(M[n]))
        truth = R.affine_inverse_vjp(M[n], cot[n])
        bar = max(8 * EPS * np.abs(truth).max(), 1.25 * np.abs(M32.grad[n].numpy() - truth).max())
        err = np.abs(dM[n] - truth).max()
        worst = max(worst, err / bar)
        assert np.isfinite(dM[n]).all() and err <= bar, f"{name}[{n}] backward: error {err:.3e} over the bar {bar:.3e}"
    print(f"{name}: worst backward error / bar {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------- points
PTS = R.points_cases()


@pytest.mark.parametrize("name,M,pts", PTS, ids=[c[0] for c in PTS])
def test_affine_points_vs_fp64(name, M, pts):
    """P in {1, 63, 256, 257, 5000}: under one wavefront, one block of the forward, one thread past it, and 20 trips of the
    backward's strided loop.  Observed on gfx950, as fractions of the bars: forward <= 0.37, dpts <= 0.39, dM <= 0.11"""
    N, P, _ = pts.shape
    cot = R.cotangent(P, (N, P, 3))
    Md = torch.from_numpy(M).to(DEV).requires_grad_(True)
    pd = torch.from_numpy(pts).to(DEV).requires_grad_(True)
    out = _ops().affine_points(Md, pd)
    (out * torch.from_numpy(cot).to(DEV)).sum().backward()
    out, dM, dp = _np(out), _np(Md.grad), _np(pd.grad)
    u = EPS / 2
    trips = -(-P // 256)
    for n in range(N):
        A, p, g = np.abs(M[n].astype(np.float64)), np.abs(pts[n].astype(np.float64)), np.abs(cot[n].astype(np.float64))
        bar = 8 * u * (p @ A[:, :3].T + A[:, 3])
        err = np.abs(out[n] - R.affine_points(M[n], pts[n]))
        assert (err <= bar).all(), f"{name}[{n}] forward: {float((err / bar).max()):.2f} of the bar"
        tM, tp = R.affine_points_vjp(M[n], pts[n], cot[n])
        bar_p = 6 * u * (g @ A[:, :3])
        err_p = np.abs(dp[n] - tp)
        assert (err_p <= bar_p).all(), f"{name}[{n}] dpts: {float((err_p / bar_p).max()):.2f} of the bar"
        bar_M = (trips + 3) * 2 * u * np.concatenate([g.T @ p, g.sum(0)[:, None]], 1)
        err_M = np.abs(dM[n] - tM)
        print(f"{name}[{n}]: forward {float((err / bar).max()):.2f}, dpts {float((err_p / bar_p).max()):.2f}, "
              f"dM {float((err_M / bar_M).max()):.2f} of their bars")
        assert (err_M <= bar_M).all(), f"{name}[{n}] dM: {float((err_M / bar_M).max()):.2f} of the bar"


# ------------------------------------------------------------------------------------------------------ centre of mass
@pytest.mark.parametrize("content", R.COM_CONTENTS)
@pytest.mark.parametrize("shape", R.COM_SHAPES, ids=["x".join(map(str, s)) for s in R.COM_SHAPES])
def test_com3d_vs_fp64(shape, content):
    """forward and backward against fp64 with the fp32 oracle's own error as the band; dfeat exactly 0 wherever feat <= 0 (the
    reference's F.relu and the kernel's p > 0 agree there; clamp_min(0) would not), an all <= 0 channel gives pts exactly -1.
    Observed on gfx950: forward 1e-8 .. 8e-8 (fp32 oracle 3e-8 .. 2e-7; pedestal shapes 2e-8 .. 4e-8 against the oracle's
    3e-8 .. 2e-7), always under the 8 eps32 arm.  Backward: 0.03 .. 0.32 of the bar; the closest is the single hot voxel,
    whose truth 2 (lin - m) / tot cancels to ~1e-9 while either fp32 evaluation keeps eps32 |cot| / tot ~ 1e-7 of its terms: the oracle
    band carries the bar there, 1.75e-7 against 2.50e-7 at 2x3x40x33x47 (fp32 oracle 1.25e-7)."""
    f = R.com_volume(shape, content, seed=sum(shape))
    cot = R.cotangent(sum(shape), shape[:2] + (3,))
    fd = torch.from_numpy(f).to(DEV).requires_grad_(True)
    pts = _ops().com3d(fd)
    (pts * torch.from_numpy(cot).to(DEV)).sum().backward()
    pts, df = _np(pts), _np(fd.grad)
    f32 = torch.from_numpy(f).requires_grad_(True)
    o32 = O.center_of_mass(f32, "ij")
    (o32 * torch.from_numpy(cot)).sum().backward()
    truth, tgrad = R.center_of_mass(f), R.center_of_mass_vjp(f, cot)
    ref_err = float(np.abs(o32.detach().numpy() - truth).max())
    err, bar = float(np.abs(pts - truth).max()), max(8 * EPS, 1.25 * ref_err)
    ref_gerr = float(np.abs(f32.grad.numpy() - tgrad).max())
    gerr, gbar = float(np.abs(df - tgrad).max()), max(16 * EPS * float(np.abs(tgrad).max()), 2 * ref_gerr)
    print(f"com3d {shape} {content}: forward {err:.2e} (fp32 oracle {ref_err:.2e}, bar {bar:.2e}), backward {gerr:.2e} "
          f"(fp32 oracle {ref_gerr:.2e}, max|truth| {float(np.abs(tgrad).max()):.2e}, bar {gbar:.2e})")
    assert np.isfinite(pts).all() and np.isfinite(df).all()
    assert (df[f <= 0] == 0).all(), f"{int((df[f <= 0] != 0).sum())} voxels with feat <= 0 receive a gradient"
    if content == "dead_channel":
        assert (pts[0, 0] == -1).all() and (df[0, 0] == 0).all()
    assert err <= bar, f"forward error {err:.3e} over the bar {bar:.3e}"
    assert gerr <= gbar, f"backward error {gerr:.3e} over the bar {gbar:.3e}"
