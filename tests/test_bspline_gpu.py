"""GPU: ops.bspline_grid / ops.bspline_bending / loss_ops.BendingLoss (csrc/bspline.hip) against the fp64 restatement of
tests/bspline_ref.py, and what is built on them (keymorph_amd.io.register_bspline, apply_bspline, the "bspline" entry of
model.IntensityRegistration).

The bars.  d32 = the distance of the restatement evaluated in fp32 on the CPU from its fp64 evaluation, on the same case: what
fp32 costs in any order; the kernel gets 4 x d32 for another order.  Forward: max abs error, and no less than one ulp of a
unit-size coordinate, 2^-23 (a float32 grid cannot be asked for more).  dctrl, the bending gradient: relative L2 per sample,
4 x d32.  The bending value: relative, 4 x d32 and no less than 2^-23.  Nothing comes from the kernel.

Measured on an MI355X: see DESIGN.md section 8e."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import bspline_ref as R
from tests import mi_ref
from tests import warp_mi_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
ULP = 2.0 ** -23

# name -> (grid shape (N, D, H, W), lattice (Cz, Cy, Cx))
SHAPES = {
    "one_cell": ((1, 5, 6, 7), (4, 4, 4)),                 # fewer voxels than a workgroup
    "more_cells_than_voxels": ((1, 5, 6, 7), (11, 7, 6)),  # more cells than voxels on z; voxel centres on knots on y
    "odd_box": ((1, 24, 20, 36), (6, 6, 8)),               # bspline_lattice_shape(., 8): cell edges between voxels
    "several_groups": ((1, 40, 40, 40), (8, 8, 8)),        # several workgroups per pass
    "batch": ((2, 16, 16, 16), (5, 5, 5)),                 # another lattice and another matrix per sample
    # the other paths of the kernels: a row longer than one staged chunk of the backward's x pass (64 rows x 32 voxels) ...
    "x_chunks": ((1, 8, 9, 70), (4, 4, 4)),
    # ... and more control points along x than one workgroup has lanes (two tiles of them, several blocks of the axis passes), on
    # a lattice so much finer than the grid that the forward has to shrink its tile to fit the lattice rows into LDS
    "x_tiles": ((1, 2, 3, 50), (4, 40, 260)),
}
CASES = [f"{s}-{m}" for s in SHAPES for m in ("none", "affine")]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(ctrl, mat | None, cotangent), float32 on the CPU."""
    from keymorph_amd import synthetic
    shape_name, kind = name.split("-")
    (N, D, H, Wd), lat = SHAPES[shape_name]
    g = torch.Generator().manual_seed(11 + len(shape_name))
    ctrl = 0.1 * torch.randn(N, 3, *lat, generator=g)
    cot = torch.randn(N, D, H, Wd, 3, generator=g)
    mat = None
    if kind == "affine":                                   # rotation + shear + scale + shift, another one per sample
        mat = torch.cat([synthetic.random_affine_matrix(5 + n, "cpu")[:, :3, :] for n in range(N)]).contiguous()
    return ctrl, mat, cot


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 and fp32 evaluations of the restatement, computed once: (grid64, dctrl64, d32 of the grid, d32 of dctrl per
    sample)."""
    ctrl, mat, cot = inputs(name)
    dims = cot.shape[1:4]
    g64, dc64 = R.evaluate_grid(ctrl, dims, mat, cot, F64)
    g32, dc32 = R.evaluate_grid(ctrl, dims, mat, cot, torch.float32)
    d_fwd = float((g32.to(F64) - g64).abs().max())
    d_bwd = [float((dc32[n].to(F64) - dc64[n]).norm() / dc64[n].norm()) for n in range(ctrl.shape[0])]
    return g64, dc64, d_fwd, d_bwd


def run(name, grad=True):
    from keymorph_amd import ops
    ctrl, mat, cot = inputs(name)
    c = ctrl.to(DEV).requires_grad_(grad)
    grid = ops.bspline_grid(c, cot.shape[1:4], None if mat is None else mat.to(DEV))
    if grad:
        grid.backward(cot.to(DEV))
    return grid.detach(), c.grad


# ---- the operator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_zero_ctrl_is_the_base(name):
    from keymorph_amd import fields, ops
    ctrl, mat, cot = inputs(name)
    dims = tuple(cot.shape[1:4])
    zero = torch.zeros_like(ctrl).to(DEV)
    if mat is None:
        assert torch.equal(ops.bspline_grid(zero, dims), fields.identity_grid((ctrl.shape[0], 1, *dims), DEV))
    else:
        assert torch.equal(ops.bspline_grid(zero, dims, mat.to(DEV)), ops.affine_grid(mat.to(DEV), dims))


@pytest.mark.parametrize("name", CASES)
def test_grid_and_dctrl_match_fp64(name):
    g64, dc64, d_fwd, d_bwd = reference(name)
    grid, dctrl = run(name)
    err = float((grid.cpu().to(F64) - g64).abs().max())
    bar = max(4 * d_fwd, ULP)
    print(f"{name}: grid max abs error {err:.3e}  d32 {d_fwd:.3e}  bar {bar:.3e}")
    assert grid.shape == g64.shape and err <= bar, (name, err, bar)
    for n in range(dc64.shape[0]):
        e = float((dctrl[n].cpu().to(F64) - dc64[n]).norm() / dc64[n].norm())
        print(f"{name}[{n}]: dctrl relative L2 {e:.3e}  d32 {d_bwd[n]:.3e}  bar {4 * d_bwd[n]:.3e}")
        assert math.isfinite(e) and e <= 4 * d_bwd[n], (name, n, e, d_bwd[n])


def test_control_points_that_touch_no_voxel_get_exactly_zero():
    """17 cells over 5 voxels on z: the voxels sit in cells 1, 5, 8, 11 and 15, so control planes 0 and 19 weigh on no voxel.
    (With the 8 cells of "more_cells_than_voxels" every plane is still inside some voxel's support of four.)"""
    from keymorph_amd import ops
    dims, lat = (5, 6, 7), (20, 7, 6)
    g = torch.Generator().manual_seed(5)
    cot = torch.randn(1, *dims, 3, generator=g)
    ctrl = torch.zeros(1, 3, *lat)
    _, dc64 = R.evaluate_grid(ctrl, dims, None, cot, F64)
    untouched = dc64 == 0
    assert untouched[0, :, 0].all() and untouched[0, :, 19].all() and not untouched[0, :, 1:19].any()
    c = ctrl.to(DEV).requires_grad_()
    ops.bspline_grid(c, dims).backward(cot.to(DEV))
    assert (c.grad.cpu()[untouched] == 0).all() and (c.grad.cpu()[~untouched] != 0).all()


@pytest.mark.parametrize("name", CASES)
def test_repeat_runs_are_bit_identical(name):
    g1, d1 = run(name)
    g2, d2 = run(name)
    assert torch.equal(g1, g2) and torch.equal(d1, d2)


@pytest.mark.parametrize("kind", ["none", "affine"])
def test_batch_equals_single_samples(kind):
    from keymorph_amd import ops
    ctrl, mat, cot = inputs(f"batch-{kind}")
    grid, dctrl = run(f"batch-{kind}")
    for n in range(ctrl.shape[0]):
        c = ctrl[n:n + 1].to(DEV).requires_grad_()
        g = ops.bspline_grid(c, cot.shape[1:4], None if mat is None else mat[n:n + 1].to(DEV))
        g.backward(cot[n:n + 1].to(DEV))
        assert torch.equal(g.detach()[0], grid[n]) and torch.equal(c.grad[0], dctrl[n])


def test_gradient_through_align_img_and_mutual_information_matches_finite_differences():
    """d(-MI)/d(ctrl) of the chain bspline_grid -> align_img -> mutual_information at 16^3 against central differences of the
    fp64 restatement on the twelve control values that carry most gradient (chosen by the restatement's own autograd), with the
    bar of tests/test_mi_gpu.py's test through align_img: 2e-3 relative + 1e-6.  Both ranges are the volumes' own, as the driver
    gives them: a trilinear, border-padded warp cannot leave them, so no step of the differences meets the clamp."""
    from keymorph_amd import ops, synthetic
    from keymorph_amd.utils import align_img
    S, lat = 16, (5, 5, 5)
    m, f = mi_ref.smooth_pair((1, 1, S, S, S), 8)
    mat = synthetic.random_affine_matrix(5, "cpu")[:, :3, :].contiguous()
    ctrl = 0.05 * torch.randn(1, 3, *lat, generator=torch.Generator().manual_seed(2))
    (ra, rb), = W.own_ranges(m, f)
    c = ctrl.to(DEV).requires_grad_()
    loss = -ops.mutual_information(align_img(ops.bspline_grid(c, (S, S, S), mat.to(DEV)), m.to(DEV)), f.to(DEV), 32, ra, rb).sum()
    loss.backward()
    m64, f64, mat64 = m.double(), f.double(), mat.double()

    def host(c64):
        warped = F.grid_sample(m64, R.bspline_grid(c64, (S, S, S), mat64), mode="bilinear", padding_mode="border",
                               align_corners=False)
        return -mi_ref.mutual_information(warped, f64, 32, ra, rb)[0]
    c64 = ctrl.double().requires_grad_()
    base = host(c64)
    base.backward()
    assert abs(float(base) - float(loss.detach())) < 1e-5
    picks = torch.topk(c64.grad.abs().reshape(-1), 12).indices.tolist()
    # One control value moves some 500 voxels, and a coordinate that crosses a lattice plane of the moving volume inside +-h meets
    # the trilinear blend's kink: with the h = 1e-5 of the per-grid-entry test one of the twelve differences does (it is 2.6e-3
    # from the restatement's own autograd, all on the CPU); with 1e-6 all twelve agree with it to 6e-9.
    h = 1e-6
    with torch.no_grad():
        for flat in picks:
            vals = []
            for sgn in (1.0, -1.0):
                cp = ctrl.double().clone()
                cp.reshape(-1)[flat] += sgn * h
                vals.append(float(host(cp)))
            fd = (vals[0] - vals[1]) / (2 * h)
            got = float(c.grad.reshape(-1)[flat])
            print(f"ctrl[{flat}]: kernel {got:.6e}  finite difference {fd:.6e}  fp64 autograd {float(c64.grad.reshape(-1)[flat]):.6e}")
            assert math.isfinite(got) and abs(got - fd) <= 2e-3 * abs(fd) + 1e-6, (flat, got, fd)


# ---- bending ---------------------------------------------------------------------------------------------------------------
BENDING = {"one_cell": (1, 3, 4, 4, 4), "odd": (1, 3, 5, 7, 6), "batch": (3, 3, 5, 7, 6)}


@functools.lru_cache(maxsize=None)
def bending_inputs(name):
    g = torch.Generator().manual_seed(31 + len(name))
    shape = BENDING[name]
    q = 2.0 * torch.randn(shape, generator=g)
    for n in range(1, shape[0]):                     # another scale per sample
        q[n] *= 10.0 ** n
    return q, torch.randn(shape[0], generator=g)


@pytest.mark.parametrize("name", list(BENDING))
def test_bending_matches_fp64(name):
    from keymorph_amd import ops
    q, cot = bending_inputs(name)
    b64, dq64 = R.evaluate_bending(q, cot, F64)
    b32, dq32 = R.evaluate_bending(q, cot, torch.float32)
    x = q.to(DEV).requires_grad_()
    out = ops.bspline_bending(x)
    out.backward(cot.to(DEV))
    assert out.shape == (q.shape[0],)
    for n in range(q.shape[0]):
        dv = abs(float(b32[n]) - float(b64[n])) / float(b64[n])
        ev = abs(float(out[n]) - float(b64[n])) / float(b64[n])
        dg = float((dq32[n].to(F64) - dq64[n]).norm() / dq64[n].norm())
        eg = float((x.grad[n].cpu().to(F64) - dq64[n]).norm() / dq64[n].norm())
        print(f"{name}[{n}]: value {ev:.3e} (d32 {dv:.3e}, bar {max(4 * dv, ULP):.3e})  gradient {eg:.3e} (d32 {dg:.3e}, bar {4 * dg:.3e})")
        assert ev <= max(4 * dv, ULP) and eg <= 4 * dg, (name, n, ev, dv, eg, dg)


def test_bending_repeats_batches_and_the_loss():
    from keymorph_amd import ops
    from keymorph_amd.loss_ops import BendingLoss
    q, cot = bending_inputs("batch")

    def once(t):
        x = t.to(DEV).requires_grad_()
        out = ops.bspline_bending(x)
        out.backward(cot[:t.shape[0]].to(DEV))
        return out.detach(), x.grad
    a, b = once(q), once(q)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for n in range(q.shape[0]):
        x = q[n:n + 1].to(DEV).requires_grad_()
        out = ops.bspline_bending(x)
        out.backward(cot[n:n + 1].to(DEV))
        assert torch.equal(out.detach()[0], a[0][n]) and torch.equal(x.grad[0], a[1][n])
    assert torch.equal(BendingLoss()(q.to(DEV)), ops.bspline_bending(q.to(DEV)).mean())
    lat = (5, 7, 6)
    idx = torch.stack(torch.meshgrid(*[torch.arange(c, dtype=torch.float32) for c in lat], indexing="ij"))
    linear = (0.5 * idx[0] - 1.5 * idx[1] + 0.25 * idx[2] + 2.0)[None, None].expand(1, 3, *lat).contiguous()
    assert float(ops.bspline_bending(linear.to(DEV))[0]) == 0.0


# ---- input checks ------------------------------------------------------------------------------------------------------------
def test_input_checks():
    from keymorph_amd import _lib, ops
    ctrl = torch.zeros(2, 3, 4, 5, 6, device=DEV)
    mat = torch.zeros(2, 3, 4, device=DEV)
    dims = (8, 9, 10)
    assert ops.bspline_grid(ctrl, dims, mat).shape == (2, 8, 9, 10, 3)
    with pytest.raises(_lib.KeymorphHipError):
        ops.bspline_grid(ctrl.cpu(), dims)
    with pytest.raises(_lib.KeymorphHipError):
        ops.bspline_grid(ctrl, dims, mat.cpu())
    with pytest.raises(_lib.KeymorphHipError):
        ops.bspline_bending(ctrl.cpu())
    with pytest.raises(ValueError):
        ops.bspline_grid(ctrl.double(), dims)
    with pytest.raises(ValueError):
        ops.bspline_grid(ctrl[0], dims)
    with pytest.raises(ValueError):
        ops.bspline_grid(ctrl[:, :2], dims)
    with pytest.raises(ValueError):
        ops.bspline_grid(torch.zeros(1, 3, 3, 5, 6, device=DEV), dims)               # C < 4
    with pytest.raises(ValueError):
        ops.bspline_bending(torch.zeros(1, 3, 4, 4, 3, device=DEV))
    with pytest.raises(ValueError):
        ops.bspline_bending(ctrl.half())
    with pytest.raises(ValueError):
        ops.bspline_grid(ctrl, dims, mat[:1])                                        # batch mismatch
    with pytest.raises(ValueError):
        ops.bspline_grid(ctrl, dims, mat.double())
    with pytest.raises(ValueError):
        ops.bspline_grid(ctrl, (8, 9))
    with pytest.raises(ValueError):
        ops.bspline_grid(ctrl, (8, 0, 10))
    with pytest.raises(RuntimeError):
        ops.bspline_grid(ctrl, dims, mat.clone().requires_grad_())
    with torch.no_grad():                                                            # ... which is data under no_grad
        ops.bspline_grid(ctrl, dims, mat.clone().requires_grad_())
    # the ABI's own limits: -22 before anything is launched
    lib = _lib.load()
    out = torch.empty(2, 8, 9, 10, 3, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    assert lib.kmh_bspline_grid_fwd(p(ctrl), None, p(out), 2, 8, 9, 10, 4, 5, 6, s) == 0
    assert lib.kmh_bspline_grid_fwd(p(ctrl), None, p(out), 2, 8, 9, 10, 3, 5, 6, s) == -22
    assert lib.kmh_bspline_grid_fwd(p(ctrl), None, p(out), 2, 8, 9, 10, 4, 5, 3, s) == -22
    assert lib.kmh_bspline_grid_fwd(p(ctrl), None, p(out), 2, 8, 0, 10, 4, 5, 6, s) == -22
    assert lib.kmh_bspline_grid_fwd(p(ctrl), None, p(out), 0, 8, 9, 10, 4, 5, 6, s) == -22
    assert lib.kmh_bspline_grid_fwd(p(ctrl), None, p(out), 2, 2048, 1024, 1024, 4, 5, 6, s) == -22      # 2^31 voxels
    assert lib.kmh_bspline_grid_bwd(p(out), p(ctrl), 2, 2048, 1024, 1024, 4, 5, 6, p(out), s) == -22
    assert lib.kmh_bspline_grid_bwd(p(out), p(ctrl), 2, 8, 9, 10, 4, 3, 6, p(out), s) == -22
    assert lib.kmh_bspline_grid_ws_bytes(2, 8, 9, 10, 4, 5, 6) >= 4 * 2 * 3 * (8 * 9 * 6 + 8 * 5 * 6)
    assert lib.kmh_bspline_grid_ws_bytes(2, 8, 9, 10, 3, 5, 6) == 0
    assert lib.kmh_bspline_bending_fwd(p(ctrl), p(out), 2, 3, 5, 6, p(out), s) == -22
    assert lib.kmh_bspline_bending_ws_bytes(2) >= 2 * 8 and lib.kmh_bspline_bending_ws_bytes(0) == 0
    assert lib.kmh_bspline_bending_bwd(p(ctrl), p(out), p(out), 2, 4, 5, 2, s) == -22
    torch.cuda.synchronize()


# ---- the driver ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recovery():
    """The pair validated in tests/test_bspline_cpu.py, and register_bspline's answer with its defaults from the identity matrix."""
    from keymorph_amd.io import register_bspline, voxel_to_mat
    fixed, moving = R.recovery_pair()
    mat = voxel_to_mat(torch.eye(3, device=DEV)[None], torch.zeros(1, 3, device=DEV), fixed.shape[2:])
    return fixed, moving, mat, register_bspline(fixed.to(DEV), moving.to(DEV), mat=mat)


def test_register_bspline_recovers_the_deformation(recovery):
    fixed, moving, _, ctrl = recovery
    dims = tuple(fixed.shape[2:])
    truth = R.true_ctrl()
    err = float(R.displacement_error(ctrl, truth, dims)[0])
    start = float(R.displacement_error(torch.zeros_like(truth), truth, dims)[0])
    ref, _ = R.recovery_run()
    print(f"register_bspline: mean displacement error {err:.3f} voxel (identity {start:.3f}; fp64 restatement {ref:.3f})")
    assert ctrl.shape == truth.shape and ctrl.dtype == torch.float32
    assert err <= 0.5 and err <= start / 3


def test_recovered_deformation_does_not_fold(recovery):
    from keymorph_amd import fields, loss_ops, ops
    fixed, _, mat, ctrl = recovery
    grid = ops.bspline_grid(ctrl, fixed.shape[2:], mat)
    assert loss_ops.jdlessthan0(fields.to_displacement(grid)) == 0


def test_apply_bspline_is_the_grid_and_the_sampler(recovery):
    from keymorph_amd import ops
    from keymorph_amd.io import apply_bspline
    from keymorph_amd.utils import align_img
    _, moving, mat, ctrl = recovery
    m = moving.to(DEV)
    for mode in ("bilinear", "nearest"):
        assert torch.equal(apply_bspline(m, ctrl, mat, mode), align_img(ops.bspline_grid(ctrl, m.shape[2:], mat), m, mode))
    assert torch.equal(apply_bspline(m, ctrl), align_img(ops.bspline_grid(ctrl, m.shape[2:]), m))


def test_intensity_registration_bspline_entry(recovery):
    from keymorph_amd import ops
    from keymorph_amd.model import IntensityRegistration
    fixed, moving, _, _ = recovery
    f, m = fixed.to(DEV), moving.to(DEV)
    with torch.no_grad():
        res = IntensityRegistration()(f, m, transform_type=["affine", "bspline"])
    r = res["bspline"]
    assert set(r) == {"grid", "matrix", "ctrl", "mi", "time"} and r["time"] > 0
    assert set(res["affine"]) == {"grid", "matrix", "mi", "time"}
    assert r["matrix"].shape == (1, 3, 4) and r["ctrl"].shape == (1, 3, 7, 7, 7) and r["mi"].shape == (1,)
    assert torch.equal(r["matrix"], res["affine"]["matrix"])                   # the affine it started from
    assert torch.equal(r["grid"], ops.bspline_grid(r["ctrl"], (32, 32, 32), r["matrix"]))
    print(f"MI: affine {float(res['affine']['mi'][0]):.4f}  bspline {float(r['mi'][0]):.4f}")
    assert float(r["mi"][0]) > float(res["affine"]["mi"][0])
