"""GPU: csrc/grids.hip (the implicit lattice, affine grid forward and adjoint, the thin-plate-spline evaluators on the grid and on
explicit points with every gradient, the augmentation matrix) and the Jacobian-determinant and argmax kernels of csrc/losses.hip
against the fp64 restatement of tests/grids_ref.py, at the shapes where each kernel changes its path.
tests/test_grids_reference_cpu.py pins the restatement, the bars and the case tables.

Every assertion is a bit equality or a bar derived in grids_ref's docstring (u = eps32 / 2): an arithmetic bound counted from the
kernel's own operations, plus -- for the outputs that pass through the hardware log2 / sqrt / rcp -- 2 x the worst error of the fp32
CPU oracle on the same case.  Each test prints error and bar; the docstrings carry the worst ratio error / bar observed on gfx950
(MI355X)."""
import numpy as np
import pytest
import torch

from tests import grids_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U


def _ops():
    from keymorph_amd import ops
    return ops


def _err():
    from keymorph_amd import _lib
    return _lib.KeymorphHipError


def _dev(a, grad=False):
    t = torch.from_numpy(np.array(a, copy=True)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {np.argwhere(bad)[0]}"


def _check(tag, got, truth, bar, quiet=False):
    """|got - truth| <= bar element by element (bar 0: exact); -> worst error / bar"""
    got, truth, bar = np.asarray(got, np.float64), np.asarray(truth, np.float64), np.broadcast_to(bar, np.shape(truth))
    err = np.abs(got - truth)
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))
    if not quiet:
        print(f"{tag}: error {float(err.max(initial=0.0)):.3e}, bar {float(bar.max(initial=0.0)):.3e}, worst error / bar {ratio:.3f}")
    assert np.isfinite(got).all() and ratio <= 1.0, f"{tag}: worst error / bar {ratio:.3f}"
    return ratio


# ======================================================================================================= lattice
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_identity_grid_is_linspace_bit_for_bit(axis):
    """affine_grid(identity) is the CPU's torch.linspace lattice flipped to xyz in every bit, one axis swept over n = 1 .. 130, 255,
    256, 257 with the other two at 2; an axis of one voxel is -1"""
    ops = _ops()
    eye = _dev(np.eye(3, 4, dtype=np.float32)[None])
    for n in R.LATTICE_N:
        shape = tuple(n if a == axis else 2 for a in range(3))
        _same_bits(f"{shape}", _np(ops.affine_grid(eye, shape))[0], R.identity_grid(shape))
    for shape in R.AFFINE_SHAPES:
        _same_bits(f"{shape}", _np(ops.affine_grid(eye, shape))[0], R.identity_grid(shape))


# =================================================================================================== affine grid
@pytest.mark.parametrize("name", R.AFFINE_MATRICES)
def test_affine_grid_vs_fp64(name):
    """forward u (3 |m0 gz| + 4 |m1 gy| + 2 |m2 gx| + |m3|), adjoint k u sum|g p| + u |truth| with a random and a cancelling
    cotangent, on both store paths, fewer than four voxels and one-voxel axes; N = 3 is three launches of N = 1 in every bit and
    a second run repeats the first.  Observed worst error / bar: forward 0.87, adjoint 0.32."""
    ops = _ops()
    wf = wb = 0.0
    for shape in R.AFFINE_SHAPES:
        M = R.affine_matrix(name)
        N, nvox = M.shape[0], int(np.prod(shape))
        for kind in ("random", "cancelling"):
            cot = R.affine_cotangent(kind, shape, N)
            Md = _dev(M, True)
            out = ops.affine_grid(Md, shape)
            out.backward(_dev(cot))
            got, dM = _np(out), _np(Md.grad)
            M2 = _dev(M, True)
            out2 = ops.affine_grid(M2, shape)
            out2.backward(_dev(cot))
            _same_bits("second run", _np(out2), got)
            _same_bits("second run dM", _np(M2.grad), dM)
            for n in range(N):
                M1 = _dev(M[n:n + 1], True)
                o1 = ops.affine_grid(M1, shape)
                o1.backward(_dev(cot[n:n + 1]))
                _same_bits(f"{shape} N = 1 [{n}]", _np(o1)[0], got[n])
                _same_bits(f"{shape} N = 1 dM[{n}]", _np(M1.grad)[0], dM[n])
                wf = max(wf, _check(f"{name} {shape}[{n}]", got[n], R.affine_grid(M[n], shape), R.affine_grid_bar(M[n], shape), True))
                truth, mag = R.affine_grid_adjoint(cot[n], shape)
                wb = max(wb, _check(f"{name} {shape} {kind} dM[{n}]", dM[n], truth, R.affine_adjoint_bar(truth, mag, nvox), True))
    print(f"{name}: worst error / bar forward {wf:.3f}, adjoint {wb:.3f}")


@pytest.mark.parametrize("kind", ["random", "cancelling"])
def test_affine_adjoint_past_one_grid_pass(kind):
    """(3, 1024, 1366) = 4 196 352 voxels, just past 1024 blocks x 4096: every lane of the first blocks takes a 17th term.
    Observed worst error / bar 0.0002 (errors add like a random walk, the bound is the worst case of 17 terms per lane)."""
    ops = _ops()
    shape = R.AFFINE_BIG
    cot = R.affine_cotangent(kind, shape, 1)
    Md = _dev(R.affine_matrix("generic", 1), True)
    ops.affine_grid(Md, shape).backward(_dev(cot))
    truth, mag = R.affine_grid_adjoint(cot[0], shape)
    _check(f"{kind} dM", _np(Md.grad)[0], truth, R.affine_adjoint_bar(truth, mag, int(np.prod(shape))))


# ====================================================================================================== TPS grid
def _tps_grid_run(theta, ctrl, cot, shape):
    ops = _ops()
    th, c = _dev(theta, True), _dev(ctrl, True)
    out = ops.tps_grid(th, c, shape)
    out.backward(_dev(cot))
    return _np(out), _np(th.grad), _np(c.grad)


def _tps_compare(tag, res, got, worst):
    truth, arith, allow, _ = res
    for k, g in got.items():
        worst[k] = max(worst.get(k, 0.0), _check(f"{tag} {k}", g, truth[k], arith[k] + allow[k], True))


@pytest.mark.parametrize("name", list(R.TPS_GRID_CASES))
def test_tps_grid_vs_fp64(name):
    """kmh_tps_grid_fwd / _bwd on every arm (W % 8 == 0, W % 4 == 0, plain; one and two blocks; one and two chunks, a ragged last
    stage, the row-hoisted backward with one and two stages per row; T = 1 .. 2048 with a second keypoint tile) and every
    keypoint class (random, on lattice nodes, twins, outside the volume, zero weights, U alone): forward, dtheta (weights and
    affine rows apart) and dctrl within arithmetic bound + allowance; N = 3 is three launches of N = 1 in every bit; a second
    run repeats the first; zero weights give dctrl == 0 exactly.  Observed worst error / bar over the table: forward 0.19,
    dtheta_w 0.12, affine rows 0.20, dctrl 0.06."""
    theta, ctrl, cot, shape = R.tps_grid_case(name)
    N, T = ctrl.shape[:2]
    out, dth, dc = _tps_grid_run(theta, ctrl, cot, shape)
    for a, b in zip(_tps_grid_run(theta, ctrl, cot, shape), (out, dth, dc)):
        _same_bits("second run", a, b)
    worst = {}
    for n in range(N):
        if N > 1:
            for tag, a, b in zip(("out", "dtheta", "dctrl"), _tps_grid_run(theta[n:n + 1], ctrl[n:n + 1], cot[n:n + 1], shape), (out, dth, dc)):
                _same_bits(f"N = 1 {tag}[{n}]", a[0], b[n])
        got = {"out": out[n].reshape(-1, 3)[:, ::-1], "dw": dth[n, :T], "daff": dth[n, T:], "dctrl": dc[n]}
        _tps_compare(f"{name}[{n}]", R.tps_grid_truth(name, n), got, worst)
    if R.TPS_GRID_CASES[name][2] == "wzero":
        assert not dc.any(), "zero weights: dctrl must be exactly 0"
    print(f"{name}: worst error / bar " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("name", list(R.TPS_GRID_CASES))
def test_tps_grid_is_tps_points_on_the_lattice_bit_for_bit(name):
    """the three implicit-grid arms (8 voxels per lane row-hoisted, 4 row-hoisted, plain) equal, in every bit, the explicit-point
    evaluator fed the same lattice as points (taken from affine_grid(identity)) and flipped: the row hoisting keeps tps_d2's
    chain"""
    ops = _ops()
    theta, ctrl, _, shape = R.tps_grid_case(name)
    N = ctrl.shape[0]
    eye = _dev(np.tile(np.eye(3, 4, dtype=np.float32), (N, 1, 1)))
    pts = ops.affine_grid(eye, shape).reshape(N, -1, 3).flip(-1).contiguous()
    th, c = _dev(theta), _dev(ctrl)
    want = ops.tps_points(th, c, pts).flip(-1).reshape(N, *shape, 3)
    _same_bits(f"{name} ({R.tps_fwd_arm(shape)})", _np(ops.tps_grid(th, c, shape)), _np(want))


def test_tps_refuses_more_keypoints_than_fit_in_lds():
    """T = 2049 needs 65 568 bytes of LDS: both evaluators answer -22 before anything is launched"""
    ops = _ops()
    th, c = torch.zeros((1, 2053, 3), device=DEV), torch.zeros((1, 2049, 3), device=DEV)
    with pytest.raises(_err(), match="-22"):
        ops.tps_grid(th, c, (2, 3, 4))
    with pytest.raises(_err(), match="-22"):
        ops.tps_points(th, c, torch.zeros((1, 5, 3), device=DEV))


# ==================================================================================================== TPS points
def _tps_points_run(theta, ctrl, pts, cot):
    ops = _ops()
    th, c, p = _dev(theta, True), _dev(ctrl, True), _dev(pts, True)
    out = ops.tps_points(th, c, p)
    out.backward(_dev(cot))
    return _np(out), _np(th.grad), _np(c.grad), _np(p.grad)


@pytest.mark.parametrize("name", list(R.TPS_POINTS_CASES))
def test_tps_points_vs_fp64(name):
    """kmh_tps_points_fwd / _bwd at P = 1, 3, 4, 70, 72, 1025 (second forward block), 8193 (second backward chunk), T up to 513,
    the keypoints through their own spline (every (p, p) pair at d2 = 1e-6) at T = P = 64 and 512, keypoints mixed with random
    points: forward, dtheta, dctrl and dpts (the raw sqrt / log / rcp kernel) within arithmetic bound + allowance; N = 3 is
    three launches of N = 1; a second run repeats the first.  Observed worst error / bar over the table: forward 0.15, dtheta_w
    0.16, affine rows 0.78 (P = 3: one term per lane, the bar is two roundings), dctrl 0.13, dpts 0.11."""
    theta, ctrl, pts, cot = R.tps_points_case(name)
    N, T = ctrl.shape[:2]
    first = _tps_points_run(theta, ctrl, pts, cot)
    for a, b in zip(_tps_points_run(theta, ctrl, pts, cot), first):
        _same_bits("second run", a, b)
    out, dth, dc, dp = first
    worst = {}
    for n in range(N):
        if N > 1:
            one = _tps_points_run(theta[n:n + 1], ctrl[n:n + 1], pts[n:n + 1], cot[n:n + 1])
            for tag, a, b in zip(("out", "dtheta", "dctrl", "dpts"), one, first):
                _same_bits(f"N = 1 {tag}[{n}]", a[0], b[n])
        got = {"out": out[n], "dw": dth[n, :T], "daff": dth[n, T:], "dctrl": dc[n], "dpts": dp[n]}
        _tps_compare(f"{name}[{n}]", R.tps_points_truth(name, n), got, worst)
    if R.TPS_POINTS_CASES[name][2] == "wzero":
        assert not dc.any(), "zero weights: dctrl must be exactly 0"
    print(f"{name}: worst error / bar " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ================================================================================================== augmentation
@pytest.mark.parametrize("B", R.AUGMENT_B)
def test_build_affine_matrix_vs_fp64(B):
    """kmh_affine_build_matrix: five nested fp32 products, cosf / sinf at 2 x the CPU oracle's own error on the same angles; B = 1
    is the identity in every bit, B = 64 holds 0, +-pi, pi / 2, +-2 pi, B = 65 takes a second block.  Observed worst error /
    bar 0.12."""
    from keymorph_amd import augmentation as A
    p = R.augment_case(B)
    got = _np(A.AffineDeformation3d(device=DEV).build_affine_matrix(B, tuple(torch.from_numpy(a.copy()) for a in p)))
    if B == 1:
        _same_bits("identity", got[0], np.eye(4, dtype=np.float32))
    _check(f"B {B}", got, R.augment_matrix(*p), R.augment_bar(*p))
    _same_bits("bottom row", got[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (B, 1)))


# ====================================================================================================== Jacobian
@pytest.mark.parametrize("name", R.JAC_CASES)
@pytest.mark.parametrize("layout", ["ncdhw", "permuted"])
def test_jacobian_determinant_vs_fp64(name, layout):
    """kmh_jacobian_det from the NCDHW tensor and from the permuted view of a (1, D, H, W, 3) grid: the map within the running-error
    bound of the 3 x 3 expansion, {mean, std} within the propagated bars, the count of det <= 0 EXACT (no truth other than an
    exact zero lies within its bar of zero: test_grids_reference_cpu.py); disp_z = -z gives a map of zeros, all counted; 106^3
    takes the grid-stride loop's second trip.  Observed worst error / bar: map 0.39, mean 0.02, std 0.02."""
    from keymorph_amd import loss_ops as L
    d = R.jacobian_case(name)
    if layout == "ncdhw":
        disp = _dev(d[None])
    else:
        disp = _dev(np.ascontiguousarray(np.moveaxis(d, 0, -1))[None]).permute(0, 4, 1, 2, 3)
        assert not disp.is_contiguous()
    jd, st = L._jacdet(disp, True)
    truth, bar = R.jacobian_det(d), R.jacobian_bar(d)
    (mean, std, neg), (bmean, bstd) = R.jacobian_stats(truth, bar)
    _check(f"{name} map", _np(jd), truth, bar)
    st = _np(st)
    _check(f"{name} mean", st[0], mean, bmean)
    _check(f"{name} std", st[1], std, bstd)
    assert st[2] == neg and st[3] == truth.size, (st, neg, truth.size)
    assert L.jdlessthan0(disp) == neg
    if name == "exact_zero":
        assert not _np(jd).any() and st[0] == 0 and st[1] == 0 and neg == truth.size
    _same_bits("stats without the map", _np(L._jacdet(disp, False)[1]), st)


def test_jacobian_refuses_an_axis_of_four():
    from keymorph_amd import loss_ops as L
    for shape in ((4, 5, 5), (5, 4, 5), (5, 5, 4)):
        with pytest.raises(_err(), match="-22"):
            L._jacdet(torch.zeros((1, 3) + shape, device=DEV), True)


# ======================================================================================================== argmax
@pytest.mark.parametrize("cls", R.ARGMAX_CLASSES)
def test_argmax_onehot_is_torch_argmax(cls):
    """kmh_argmax_onehot equals the one-hot of torch.argmax in every element: the first maximum at ties, +0 == -0, +-inf, and the
    first NaN wherever it stands (channel 0, a middle one, the last, two of them); C in {1, 2, 5}, V around one block, N = 2"""
    ops = _ops()
    for C in R.ARGMAX_C:
        for V in R.ARGMAX_V:
            x = R.argmax_case(cls, C, V)
            got = _np(ops.argmax_onehot(_dev(x)))
            _same_bits(f"{cls} C {C} V {V}", got, R.argmax_onehot(x))
            t = torch.from_numpy(x)
            _same_bits(f"{cls} C {C} V {V} torch", got, torch.zeros_like(t).scatter(1, t.argmax(dim=1, keepdim=True), 1.0).numpy())
