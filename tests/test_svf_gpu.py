"""GPU: ops.svf_grid (csrc/svf.hip, the displacement entry of csrc/bspline.hip) against the fp64 restatement of tests/svf_ref.py,
and what is built on it (keymorph_amd.io.register_svf, svf_grid, apply_svf, the "svf" entry of model.IntensityRegistration).

The bars.  d32 = the distance of the restatement evaluated in fp32 on the CPU from its fp64 evaluation, on the same case: what
fp32 costs in any order; the kernels get 4 x d32.  Grid: max abs error.  dctrl: relative L2 per sample.  Nothing comes from the
kernel.  The shapes are small on purpose: (5, 6, 7) is one ragged chunk of the 1024-voxel chunk walk, (9, 10, 13) two chunks with
an odd W and rows off the 16-byte grid, (16, 18, 20) with spacing 4 a lattice fine enough to fold.

The recovery pairs and their conditions are validated for the restatement alone in tests/test_svf_cpu.py."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import bspline_ref as R
from tests import mi_ref
from tests import svf_ref as S
from tests import warp_mi_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
K = 6

# name -> (dims, control spacing)
SHAPES = {"ragged": ((5, 6, 7), 8), "two_chunks": ((9, 10, 13), 8), "box": ((16, 18, 20), 4)}
BOX = SHAPES["box"][0]


def lattice(name, amplitude, seed=7):
    dims, spacing = SHAPES[name]
    return S.random_lattice(dims, spacing, amplitude, seed, n=2).float()


def mats():
    return S.random_mats(2).float()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(ctrl, mat | None, cotangent), float32 on the CPU, on the box."""
    amp, kind = case.split("-")
    cot = torch.randn(2, *BOX, 3, generator=torch.Generator().manual_seed(13))
    return lattice("box", float(amp)), (mats() if kind == "affine" else None), cot


CASES = [f"{a}-{m}" for a in ("1.5", "5") for m in ("none", "affine")]


@functools.lru_cache(maxsize=None)
def reference(case):
    ctrl, mat, cot = inputs(case)
    g64, dc64 = S.evaluate_grid(ctrl, BOX, K, mat, cot, F64)
    g32, dc32 = S.evaluate_grid(ctrl, BOX, K, mat, cot, torch.float32)
    d_fwd = float((g32.to(F64) - g64).abs().max())
    d_bwd = [float((dc32[n].to(F64) - dc64[n]).norm() / dc64[n].norm()) for n in range(ctrl.shape[0])]
    return g64, dc64, d_fwd, d_bwd


def run(case):
    from keymorph_amd import ops
    ctrl, mat, cot = inputs(case)
    c = ctrl.to(DEV).requires_grad_()
    grid = ops.svf_grid(c, BOX, K, None if mat is None else mat.to(DEV))
    grid.backward(cot.to(DEV))
    return grid.detach(), c.grad


# ---- the operator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_zero_lattice_is_the_base(name):
    from keymorph_amd import fields, ops
    dims = SHAPES[name][0]
    zero = torch.zeros_like(lattice(name, 1.0)).to(DEV)
    m = mats().to(DEV)
    assert torch.equal(ops.svf_grid(zero, dims), fields.identity_grid((2, 1, *dims), DEV))
    assert torch.equal(ops.svf_grid(zero, dims, K, m), ops.affine_grid(m, dims))


@pytest.mark.parametrize("name", list(SHAPES))
def test_zero_steps_is_the_free_form_grid(name):
    from keymorph_amd import ops
    dims = SHAPES[name][0]
    ctrl = lattice(name, 1.5).to(DEV)
    assert torch.equal(ops.svf_grid(ctrl, dims, 0), ops.bspline_grid(ctrl, dims))


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_step_is_the_chain_of_existing_operators(name):
    """u + align_img(identity_grid + u, u) after each of the K steps, bit for bit: the same blend8 on the same eight values at the
    same coordinate, and plain fp32 adds either side.  (ctrl 2^-j is exact, so stopping after j steps is steps = j on ctrl 2^-(K - j).)"""
    from keymorph_amd import fields, ops
    from keymorph_amd.utils import align_img
    dims = SHAPES[name][0]
    ctrl = lattice(name, 1.5 if name != "box" else 5.0).to(DEV)
    ids = fields.identity_grid((2, 1, *dims), DEV)
    u = ops.svf_displacement(ctrl * 2.0 ** -K, dims, 0)
    for j in range(1, K + 1):
        u = u + align_img(ids + u, u.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)
        assert torch.equal(u, ops.svf_displacement(ctrl * 2.0 ** -(K - j), dims, j)), j
    assert torch.equal(ids + u, ops.svf_grid(ctrl, dims, K))
    # the other arm of the compose kernel, a given grid: what inverse=True with a matrix uses
    first = ops.affine_grid(mats().to(DEV), dims)
    want = first + align_img(first, u.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)
    assert torch.equal(ops.svf_compose(u, first), want)


@pytest.mark.parametrize("case", CASES)
def test_grid_and_dctrl_match_fp64(case):
    g64, dc64, d_fwd, d_bwd = reference(case)
    grid, dctrl = run(case)
    err = float((grid.cpu().to(F64) - g64).abs().max())
    print(f"{case}: grid max abs error {err:.3e}  d32 {d_fwd:.3e}  bar {4 * d_fwd:.3e}")
    assert grid.shape == g64.shape and err <= 4 * d_fwd, (case, err, d_fwd)
    for n in range(dc64.shape[0]):
        e = float((dctrl[n].cpu().to(F64) - dc64[n]).norm() / dc64[n].norm())
        print(f"{case}[{n}]: dctrl relative L2 {e:.3e}  d32 {d_bwd[n]:.3e}  bar {4 * d_bwd[n]:.3e}")
        assert math.isfinite(e) and e <= 4 * d_bwd[n], (case, n, e, d_bwd[n])


@pytest.mark.parametrize("case", CASES)
def test_repeat_runs_are_bit_identical(case):
    g1, d1 = run(case)
    g2, d2 = run(case)
    assert torch.equal(g1, g2) and torch.equal(d1, d2)


@pytest.mark.parametrize("case", ["5-none", "5-affine"])
def test_batch_equals_single_samples(case):
    """Forward and backward: the test a chain through the sampler's float-atomic volume gradient fails."""
    from keymorph_amd import ops
    ctrl, mat, cot = inputs(case)
    grid, dctrl = run(case)
    for n in range(ctrl.shape[0]):
        c = ctrl[n:n + 1].to(DEV).requires_grad_()
        g = ops.svf_grid(c, BOX, K, None if mat is None else mat[n:n + 1].to(DEV))
        g.backward(cot[n:n + 1].to(DEV))
        assert torch.equal(g.detach()[0], grid[n]) and torch.equal(c.grad[0], dctrl[n])
    # ... also where the samples' cotangents differ by orders of magnitude (the fixed-point scale is per sample)
    big = cot.clone()
    big[1] *= 1.0e6
    c = ctrl.to(DEV).requires_grad_()
    ops.svf_grid(c, BOX, K).backward(big.to(DEV))
    c0 = ctrl[:1].to(DEV).requires_grad_()
    ops.svf_grid(c0, BOX, K).backward(big[:1].to(DEV))
    assert torch.equal(c.grad[0], c0.grad[0])


def test_a_nan_velocity_stays_where_it_can_reach():
    """A NaN in one control value of sample 0.  Sample 1 is untouched, bit for bit.  Inside sample 0 a NaN travels at most one voxel
    plus the displacement per squaring step, forwards and backwards: with two steps and displacements under half a voxel it stays
    within 6 voxels of the support of its control point (the first cell of every axis), so the control points whose own support
    begins at voxel 11 or later -- index 6 and up on any axis -- keep finite gradients.  With the default six steps the NaN may
    reach the whole sample; nothing faults either way."""
    from keymorph_amd import ops
    ctrl = lattice("box", 1.5)
    cot = torch.randn(2, *BOX, 3, generator=torch.Generator().manual_seed(3))
    clean = ctrl.to(DEV).requires_grad_()
    g_clean = ops.svf_grid(clean, BOX, 2)
    g_clean.backward(cot.to(DEV))
    bad = ctrl.clone()
    bad[0, 1, 0, 0, 0] = float("nan")
    for steps in (2, K):
        for mat in (None, mats().to(DEV)):
            c = bad.to(DEV).requires_grad_()
            g = ops.svf_grid(c, BOX, steps, mat)
            g.backward(cot.to(DEV))
            torch.cuda.synchronize()
            assert torch.isnan(g[0, 0, 0, 0, 1])
            assert torch.isfinite(g[1]).all() and torch.isfinite(c.grad[1]).all()
            if steps == 2:
                d = c.grad[0]
                assert torch.isfinite(d[:, 6:]).all() and torch.isfinite(d[:, :, 6:]).all() and torch.isfinite(d[:, :, :, 6:]).all()
                assert torch.isfinite(g[0, 12:]).all() and torch.isfinite(g[0, :, 12:]).all() and torch.isfinite(g[0, :, :, 12:]).all()
                if mat is None:
                    assert torch.equal(g.detach()[1], g_clean.detach()[1]) and torch.equal(c.grad[1], clean.grad[1])


def test_the_exponential_does_not_fold_where_the_free_form_grid_does():
    """Amplitude 5 voxels on cells of 4: host check (tests/fields_ref.py::jacobian_det_central) of sample 0 of seed 14 -- the
    free-form grid has 20 folded voxels (minimum -0.17), the exponential's minimum Jacobian is 0.24 (sample 1: 0.20)."""
    from keymorph_amd import fields, loss_ops, ops
    ctrl = lattice("box", 5.0, seed=14).to(DEV)
    ffd = loss_ops.jdlessthan0(fields.to_displacement(ops.bspline_grid(ctrl[:1], BOX)))
    grid = ops.svf_grid(ctrl, BOX, K)
    svf = [loss_ops.jdlessthan0(fields.to_displacement(grid[n:n + 1])) for n in range(2)]
    print(f"folded voxels: free-form {ffd}, exponential {svf}")
    assert ffd > 0 and svf == [0, 0]


def test_inverse_consistency():
    """max |compose(svf_grid(ctrl), svf_grid(ctrl, inverse=True)) - Ids| over the voxels further than ceil(max|u|) + 1 from every
    face is at most the fp64 restatement's plus 1e-3 voxel (the restatement's own value is the trilinear discretisation of the
    flow, not rounding)."""
    from keymorph_amd import fields
    from keymorph_amd.io import svf_grid
    ctrl = lattice("box", 1.5)
    c64 = ctrl.double()
    fwd64, inv64 = S.svf_grid(c64, BOX, K), S.inverse_grid(c64, BOX, K)
    half = torch.tensor([BOX[2] / 2, BOX[1] / 2, BOX[0] / 2], dtype=F64)
    umax = float(((fwd64 - R.identity(BOX)[None]) * half).abs().max())
    ref = S.inverse_consistency(fwd64, inv64, umax)
    m = math.ceil(umax) + 1
    fwd, inv = svf_grid(ctrl.to(DEV), BOX), svf_grid(ctrl.to(DEV), BOX, inverse=True)
    assert torch.equal(inv, svf_grid(-ctrl.to(DEV), BOX))
    r = (fields.compose(inv, fwd) - fields.identity_grid((2, 1, *BOX), DEV)).cpu().double() * half
    got = float(r[:, m + 1:BOX[0] - m - 1, m + 1:BOX[1] - m - 1, m + 1:BOX[2] - m - 1].abs().max())
    print(f"max |u| {umax:.3f} voxel, margin {m + 1}: inverse consistency {got:.4e} voxel, fp64 restatement {ref:.4e}")
    assert got <= ref + 1e-3
    # with a matrix, against the restatement of P + U^-(P)
    mat = mats()
    inv_m = svf_grid(ctrl.to(DEV), BOX, mat.to(DEV), inverse=True)
    want = S.inverse_grid(c64, BOX, K, mat.double())
    # (P goes through a 3 x 3 inverse in fp32 and is an O(1) coordinate: a few ulp times the matrix' condition number; U^- has
    # slope under 1.  2e-5 is some hundred ulp of a unit coordinate, a hundredth of a voxel's 0.1.)
    assert float((inv_m.cpu().double() - want).abs().max()) <= 2e-5
    with pytest.raises(RuntimeError):
        svf_grid(ctrl.to(DEV).requires_grad_(), BOX, inverse=True)


def test_input_checks():
    from keymorph_amd import _lib, ops
    ctrl = torch.zeros(2, 3, 4, 5, 6, device=DEV)
    mat = torch.zeros(2, 3, 4, device=DEV)
    dims = (8, 9, 10)
    assert ops.svf_grid(ctrl, dims, 3, mat).shape == (2, 8, 9, 10, 3)
    assert ops.svf_grid(ctrl, dims, 12).shape == ops.svf_displacement(ctrl, dims, 0).shape == (2, 8, 9, 10, 3)
    with pytest.raises(_lib.KeymorphHipError):
        ops.svf_grid(ctrl.cpu(), dims)
    with pytest.raises(_lib.KeymorphHipError):
        ops.svf_grid(ctrl, dims, 6, mat.cpu())
    for bad in (ctrl.double(), ctrl[0], ctrl[:, :2], torch.zeros(1, 3, 3, 5, 6, device=DEV)):
        with pytest.raises(ValueError):
            ops.svf_grid(bad, dims)
    for steps in (-1, 13, 2.5, True):
        with pytest.raises(ValueError):
            ops.svf_grid(ctrl, dims, steps)
    with pytest.raises(ValueError):
        ops.svf_grid(ctrl, dims, 6, mat[:1])
    with pytest.raises(ValueError):
        ops.svf_grid(ctrl, dims, 6, mat.double())
    with pytest.raises(ValueError):
        ops.svf_grid(ctrl, (8, 9))
    with pytest.raises(ValueError):
        ops.svf_grid(ctrl, (8, 0, 10))
    with pytest.raises(ValueError):
        ops.svf_grid(ctrl, (512, 1024, 1024))                                        # 3 x 2^29 floats: past one buffer descriptor
    with pytest.raises(ValueError):
        ops.svf_grid(ctrl, (8, 1, 10), 6, mat)                                       # a matrix needs two voxels per axis
    with pytest.raises(RuntimeError):
        ops.svf_grid(ctrl, dims, 6, mat.clone().requires_grad_())
    with torch.no_grad():                                                            # ... which is data under no_grad
        ops.svf_grid(ctrl, dims, 6, mat.clone().requires_grad_())
    u = torch.zeros(2, 8, 9, 10, 3, device=DEV)
    with pytest.raises(ValueError):
        ops.svf_compose(u, u[:1])
    with pytest.raises(RuntimeError):
        ops.svf_compose(u.clone().requires_grad_(), u)
    # the ABI's own limits: -22 before anything is launched
    lib = _lib.load()
    out = torch.empty(2, 8, 9, 10, 3, device=DEV)
    am = torch.zeros(2, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.kmh_svf_square_bwd_ws_bytes(2, 8, 9, 10)), dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    assert lib.kmh_bspline_disp_fwd(p(ctrl), p(out), 2, 8, 9, 10, 4, 5, 6, s) == 0
    assert lib.kmh_bspline_disp_fwd(p(ctrl), p(out), 2, 8, 9, 10, 3, 5, 6, s) == -22
    assert lib.kmh_bspline_disp_fwd(p(ctrl), None, 2, 8, 9, 10, 4, 5, 6, s) == -22
    assert lib.kmh_bspline_disp_fwd(p(ctrl), p(out), 2, 2048, 1024, 1024, 4, 5, 6, s) == -22
    assert lib.kmh_svf_compose(p(u), None, None, p(out), 2, 8, 9, 10, s) == 0
    assert lib.kmh_svf_compose(p(u), None, None, p(u), 2, 8, 9, 10, s) == -22         # in place
    assert lib.kmh_svf_compose(p(u), p(out), None, p(out), 2, 8, 9, 10, s) == -22     # a grid without its addend
    assert lib.kmh_svf_compose(p(u), None, None, p(out), 0, 8, 9, 10, s) == -22
    assert lib.kmh_svf_compose(p(u), None, None, p(out), 2, 8, 0, 10, s) == -22
    assert lib.kmh_svf_compose(p(u), None, None, p(out), 1, 512, 1024, 1024, s) == -22
    assert lib.kmh_svf_finish_fwd(p(u), None, p(out), 2, 8, 9, 10, s) == 0
    assert lib.kmh_svf_finish_fwd(p(u), p(mat), p(out), 2, 8, 1, 90, s) == -22
    assert lib.kmh_svf_finish_fwd(None, None, p(out), 2, 8, 9, 10, s) == -22
    assert lib.kmh_svf_finish_bwd(p(u), None, p(out), p(am), 2, 8, 9, 10, s) == 0
    assert lib.kmh_svf_finish_bwd(p(u), None, p(u), p(am), 2, 8, 9, 10, s) == -22
    assert lib.kmh_svf_finish_bwd(p(u), None, p(out), p(am), 70000, 8, 9, 10, s) == -22
    assert lib.kmh_svf_square_bwd(p(u), p(out), p(out), p(am), None, 2, 8, 9, 10, p(ws), s) == 0
    assert lib.kmh_svf_square_bwd(p(u), p(out), p(out), None, None, 2, 8, 9, 10, p(ws), s) == -22
    assert lib.kmh_svf_square_bwd(p(u), p(out), p(out), p(am), None, 2, 8, 9, 10, None, s) == -22
    assert lib.kmh_svf_square_bwd(p(u), p(out), p(u), p(am), None, 2, 8, 9, 10, p(ws), s) == -22
    assert lib.kmh_svf_square_bwd_ws_bytes(2, 8, 9, 10) == 2 * 720 * 32 and lib.kmh_svf_square_bwd_ws_bytes(2, 8, 0, 10) == 0
    torch.cuda.synchronize()


def test_gradient_through_align_img_and_mutual_information_matches_finite_differences():
    """d(-MI)/d(ctrl) of the chain svf_grid -> align_img -> mutual_information at 16^3 against central differences of the fp64
    restatement on the twelve control values that carry most gradient, in the manner of tests/test_bspline_gpu.py: 2e-3 relative
    + 1e-6.  The step is h = 1e-7: every squaring step adds the kinks of its own trilinear blend, and with that test's 1e-6 two of
    the twelve differences cross one (they are 1.5e-3 and 2.1e-3 from the restatement's own autograd, all on the CPU in fp64); with
    1e-7 all twelve agree with it to 5e-8."""
    from keymorph_amd import ops, synthetic
    from keymorph_amd.utils import align_img
    Sz, lat = 16, (5, 5, 5)
    m, f = mi_ref.smooth_pair((1, 1, Sz, Sz, Sz), 8)
    mat = synthetic.random_affine_matrix(5, "cpu")[:, :3, :].contiguous()
    ctrl = 0.05 * torch.randn(1, 3, *lat, generator=torch.Generator().manual_seed(2))
    (ra, rb), = W.own_ranges(m, f)
    c = ctrl.to(DEV).requires_grad_()
    loss = -ops.mutual_information(align_img(ops.svf_grid(c, (Sz, Sz, Sz), K, mat.to(DEV)), m.to(DEV)), f.to(DEV), 32, ra, rb).sum()
    loss.backward()
    m64, f64, mat64 = m.double(), f.double(), mat.double()

    def host(c64):
        warped = F.grid_sample(m64, S.svf_grid(c64, (Sz, Sz, Sz), K, mat64), mode="bilinear", padding_mode="border",
                               align_corners=False)
        return -mi_ref.mutual_information(warped, f64, 32, ra, rb)[0]
    c64 = ctrl.double().requires_grad_()
    base = host(c64)
    base.backward()
    assert abs(float(base) - float(loss.detach())) < 1e-5
    picks = torch.topk(c64.grad.abs().reshape(-1), 12).indices.tolist()
    h = 1e-7
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


# ---- the driver ------------------------------------------------------------------------------------------------------------
def identity_mat(n=1):
    from keymorph_amd.io import voxel_to_mat
    return voxel_to_mat(torch.eye(3, device=DEV)[None].expand(n, 3, 3), torch.zeros(n, 3, device=DEV), (R.SIZE,) * 3)


@pytest.fixture(scope="module")
def recovery():
    """The default pair validated in tests/test_svf_cpu.py, and register_svf's answer with its defaults from the identity matrix."""
    from keymorph_amd.io import register_svf
    fixed, moving = S.recovery_pair()
    mat = identity_mat()
    return fixed, moving, mat, register_svf(fixed.to(DEV), moving.to(DEV), mat=mat)


def test_register_svf_recovers_the_deformation_without_folding(recovery):
    from keymorph_amd import fields, loss_ops, ops
    fixed, _, mat, ctrl = recovery
    dims = tuple(fixed.shape[2:])
    grid = ops.svf_grid(ctrl, dims, K, mat)
    err = float(S.grid_error(grid, R.AMPLITUDE, dims)[0])
    start = float(S.grid_error(R.identity(dims)[None], R.AMPLITUDE, dims)[0])
    print(f"register_svf: mean displacement error {err:.3f} voxel (identity {start:.3f}; fp64 restatement 0.287, free-form 0.285: "
          "tests/test_svf_cpu.py)")
    assert ctrl.shape == (1, 3, 7, 7, 7) and ctrl.dtype == torch.float32
    assert err <= 0.5 and err <= start / 3
    assert loss_ops.jdlessthan0(fields.to_displacement(grid)) == 0


def test_without_bending_at_amplitude_8_the_free_form_fit_folds_and_the_exponential_does_not():
    """The pair and the measure validated in tests/test_svf_cpu.py: the central-difference Jacobian determinant on the voxels one
    in from every face (svf_ref.min_jacobian).  The free-form fit folds in that outermost ring, where few voxels hold a border
    control point back -- all 60 folded voxels of the fp64 restatement lie there, and loss_ops.jdlessthan0, which looks two voxels
    in, sees none of them."""
    from keymorph_amd import ops
    from keymorph_amd.io import register_bspline, register_svf
    fixed, moving = S.recovery_pair(8.0)
    f, m, mat = fixed.to(DEV), moving.to(DEV), identity_mat()
    dims = tuple(fixed.shape[2:])
    lo_f, folded_f = S.min_jacobian(ops.bspline_grid(register_bspline(f, m, mat=mat, bending=0.0), dims, mat).cpu())
    lo_s, folded_s = S.min_jacobian(ops.svf_grid(register_svf(f, m, mat=mat, bending=0.0), dims, K, mat).cpu())
    print(f"amplitude 8, bending 0: register_bspline {folded_f} folded voxels, minimum Jacobian {lo_f:.3f}; register_svf {folded_s}, "
          f"minimum {lo_s:.3f} (fp64 restatements: 60, -0.354 and 0, 0.356)")
    assert folded_f > 0 and lo_f <= 0
    assert folded_s == 0 and lo_s > 0


def test_apply_svf_and_its_inverse(recovery):
    from keymorph_amd import ops
    from keymorph_amd.io import apply_svf, svf_grid
    from keymorph_amd.utils import align_img
    fixed, moving, mat, ctrl = recovery
    f, m = fixed.to(DEV), moving.to(DEV)
    for mode in ("bilinear", "nearest"):
        assert torch.equal(apply_svf(m, ctrl, mat, mode=mode), align_img(ops.svf_grid(ctrl, m.shape[2:], K, mat), m, mode))
    assert torch.equal(apply_svf(m, ctrl, steps=4), align_img(ops.svf_grid(ctrl, m.shape[2:], 4), m))
    assert torch.equal(apply_svf(f, ctrl, mat, inverse=True), align_img(svf_grid(ctrl, f.shape[2:], mat, inverse=True), f))
    before = float(ops.mutual_information(f, m, 32)[0])
    for mt in (None, mat):                           # the matrix is the identity: both arms of the inverse give the same map
        after = float(ops.mutual_information(apply_svf(f, ctrl, mt, inverse=True), m, 32)[0])
        print(f"mutual information with moving: fixed {before:.3f}, fixed through the inverse {after:.3f} (host: 0.71 -> 1.19)")
        assert after > before + 0.2


def test_intensity_registration_svf_entry(recovery):
    from keymorph_amd import ops
    from keymorph_amd.io import svf_grid
    from keymorph_amd.model import IntensityRegistration
    fixed, moving, _, _ = recovery
    f, m = fixed.to(DEV), moving.to(DEV)
    with torch.no_grad():
        res = IntensityRegistration()(f, m, transform_type=["affine", "svf"])
    r = res["svf"]
    assert set(r) == {"grid", "inverse_grid", "matrix", "ctrl", "mi", "time"} and r["time"] > 0
    assert set(res["affine"]) == {"grid", "matrix", "mi", "time"}
    assert r["matrix"].shape == (1, 3, 4) and r["ctrl"].shape == (1, 3, 7, 7, 7) and r["mi"].shape == (1,)
    assert torch.equal(r["matrix"], res["affine"]["matrix"])                   # the affine it started from
    assert torch.equal(r["grid"], ops.svf_grid(r["ctrl"], (32, 32, 32), K, r["matrix"]))
    assert torch.equal(r["inverse_grid"], svf_grid(r["ctrl"], (32, 32, 32), r["matrix"], K, inverse=True))
    print(f"MI: affine {float(res['affine']['mi'][0]):.4f}  svf {float(r['mi'][0]):.4f}")
    assert float(r["mi"][0]) > float(res["affine"]["mi"][0])
    with torch.no_grad():
        r2 = IntensityRegistration(metric="lncc", bspline_iters=4, svf_steps=4)(f, m, transform_type="svf")["svf"]
    assert set(r2) == {"grid", "inverse_grid", "matrix", "ctrl", "mi", "lncc", "time"}
    assert torch.equal(r2["grid"], ops.svf_grid(r2["ctrl"], (32, 32, 32), 4, r2["matrix"]))
