"""GPU: the dense displacement model (ops.displacement_grid, displacement_step_scale, displacement_update: csrc/dense.hip) against
the fp64 restatement of tests/dense_ref.py, and what is built on it (keymorph_amd.io.register_greedy, apply_greedy, the "greedy"
entry of model.IntensityRegistration).

The bars.  d32 = the distance of the restatement evaluated in fp32 on the CPU from its fp64 evaluation, on the same case: what
fp32 costs in any order; the kernels get 4 x d32 (max abs error), the rule of gauss_ref.tolerance.  The step scale: 8 x 2^-24
relative -- three roundings in the squared norm, halved by the root, plus up to 1 ulp each for the device's root and divide.
Nothing comes from the kernel.  The shapes are small on purpose: (5, 6, 7) is one ragged chunk of the 1024-voxel chunk walk,
(1, 5, 7) a single slice (the operators that take no matrix), (2, 2, 2) the smallest volume a matrix allows -- every corner pair is
the last column's -- and (9, 17, 33) five chunks, the last ragged, with an odd W and rows off the 16-byte grid; (37, 29, 1), two chunks
with W = 1, is the update kernel's instance of its own (four-byte loads, no x-pairs: the sampler's pair layout needs W >= 2); the
step scale also at N = 256 x (9, 17, 61), the smallest case in which a workgroup of its capped launch walks more than one chunk.

The recovery pairs and their conditions are validated for the restatement alone in tests/test_dense_cpu.py."""
import functools

import pytest
import torch

from tests import bspline_ref as R
from tests import dense_ref as G
from tests import lncc_ref
from tests import mind_ref
from tests import svf_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
SHAPES = {"ragged": (5, 6, 7), "slice": (1, 5, 7), "corner": (2, 2, 2), "chunks": (9, 17, 33), "column": (37, 29, 1)}
WITH_MATRIX = ["ragged", "corner", "chunks"]


def rand(shape, seed, amplitude=1.0):
    return amplitude * (2 * torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) - 1)


@functools.lru_cache(maxsize=None)
def fields_of(name):
    """(disp, delta, outward), float32 on the CPU, N = 2: disp up to 1.5 voxels, delta up to 0.8, and `outward`: 3 voxels pointing
    out of every face (towards the nearer face on every axis) plus delta -- every border voxel samples past the border."""
    dims = SHAPES[name]
    disp, delta = rand((2, 3, *dims), 21, 1.5), rand((2, 3, *dims), 22, 0.8)
    idx = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float32) for n in dims], indexing="ij"))
    mid = torch.tensor([(n - 1) / 2 for n in dims])[:, None, None, None]
    outward = 3.0 * torch.where(idx < mid, -torch.ones_like(idx), torch.ones_like(idx))[None] + delta
    return disp, delta, outward


def mats():
    return S.random_mats(2).float()


# ---- displacement_grid ---------------------------------------------------------------------------------------------------
def grid_case(name, with_mat):
    disp = fields_of(name)[0]
    cot = torch.randn(2, *SHAPES[name], 3, generator=torch.Generator().manual_seed(13))
    return disp, (mats() if with_mat else None), cot


def run_grid(disp, mat, cot):
    from keymorph_amd import ops
    d = disp.to(DEV).requires_grad_()
    grid = ops.displacement_grid(d, None if mat is None else mat.to(DEV))
    grid.backward(cot.to(DEV))
    return grid.detach(), d.grad


GRID_CASES = [(n, False) for n in SHAPES] + [(n, True) for n in WITH_MATRIX]


@pytest.mark.parametrize("name,with_mat", GRID_CASES)
def test_grid_and_its_transpose_match_fp64(name, with_mat):
    disp, mat, cot = grid_case(name, with_mat)
    g64, dd64 = G.evaluate_grid(disp, mat, cot, F64)
    g32, dd32 = G.evaluate_grid(disp, mat, cot, torch.float32)
    bar_f, bar_b = 4 * float((g32.to(F64) - g64).abs().max()), 4 * float((dd32.to(F64) - dd64).abs().max())
    grid, ddisp = run_grid(disp, mat, cot)
    err_f, err_b = float((grid.cpu().to(F64) - g64).abs().max()), float((ddisp.cpu().to(F64) - dd64).abs().max())
    print(f"{name} mat={with_mat}: grid {err_f:.3e} (bar {bar_f:.3e})  ddisp {err_b:.3e} (bar {bar_b:.3e})")
    assert grid.shape == g64.shape and ddisp.shape == dd64.shape
    assert err_f <= bar_f and err_b <= bar_b


@pytest.mark.parametrize("name", list(SHAPES))
def test_grid_without_a_matrix_is_from_displacement(name):
    from keymorph_amd import fields, ops
    disp = fields_of(name)[0].to(DEV)
    assert torch.equal(ops.displacement_grid(disp), fields.from_displacement(disp))
    assert torch.equal(ops.displacement_grid(torch.zeros_like(disp)), fields.identity_grid((2, 1, *SHAPES[name]), DEV))


@pytest.mark.parametrize("name", WITH_MATRIX)
def test_zero_field_with_a_matrix_is_the_affine_grid(name):
    from keymorph_amd import ops
    m = mats().to(DEV)
    zero = torch.zeros(2, 3, *SHAPES[name], device=DEV)
    assert torch.equal(ops.displacement_grid(zero, m), ops.affine_grid(m, SHAPES[name]))


@pytest.mark.parametrize("name,with_mat", [("chunks", False), ("chunks", True), ("corner", True)])
def test_grid_repeats_and_a_batch_equals_its_samples(name, with_mat):
    disp, mat, cot = grid_case(name, with_mat)
    g1, d1 = run_grid(disp, mat, cot)
    g2, d2 = run_grid(disp, mat, cot)
    assert torch.equal(g1, g2) and torch.equal(d1, d2)
    for n in range(2):
        g, d = run_grid(disp[n:n + 1], None if mat is None else mat[n:n + 1], cot[n:n + 1])
        assert torch.equal(g[0], g1[n]) and torch.equal(d[0], d1[n])


# ---- displacement_step_scale ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_step_scale(name):
    from keymorph_amd import ops
    delta = fields_of(name)[2].clone()
    delta[1] *= 1.0e-3                                             # every sample on its own scale
    want = G.step_scale(delta.to(F64), 0.5)
    got = ops.displacement_step_scale(delta.to(DEV), 0.5)
    rel = ((got.cpu().to(F64) - want) / want).abs()
    print(f"{name}: step scale {got.tolist()}  fp64 {want.tolist()}  relative error {rel.tolist()}  bar {8 * 2.0 ** -24:.3e}")
    assert got.shape == (2,) and got.dtype == torch.float32 and got.is_cuda
    assert float(rel.max()) <= 8 * 2.0 ** -24
    assert torch.equal(got, ops.displacement_step_scale(delta.to(DEV), 0.5))
    for n in range(2):
        assert torch.equal(ops.displacement_step_scale(delta[n:n + 1].to(DEV), 0.5)[0], got[n])
    # a zero field; a NaN and an Inf voxel do not enter
    bad = delta.clone()
    bad[1] = 0
    assert ops.displacement_step_scale(bad.to(DEV), 0.5).tolist() == [float(got[0]), 0.0]
    k = int(delta[0].pow(2).sum(0).argmin())                       # not the longest vector
    z, y, x = k // (delta.shape[3] * delta.shape[4]), (k // delta.shape[4]) % delta.shape[3], k % delta.shape[4]
    for poison in (float("nan"), float("inf"), -float("inf"), 3.0e38):      # (3e38 squared overflows: not finite either)
        bad = delta.clone()
        bad[0, 1, z, y, x] = poison
        assert torch.equal(ops.displacement_step_scale(bad.to(DEV), 0.5), got), poison


def test_step_scale_where_a_workgroup_walks_several_chunks():
    """The launch is capped at max(2048 / N, 8) workgroups per sample, each walking every such chunk: N = 256 with 10 chunks of
    1024 voxels makes two workgroups of a sample take a second, and the last a ragged, chunk."""
    from keymorph_amd import ops
    delta = rand((256, 3, 9, 17, 61), 31)
    delta[7, :, 8, 16, 60] = 5.0                                   # the longest vector in the last, ragged chunk
    delta[9, :, 8, 1, 3] = 5.0                                     # ... and in a second-round full chunk (voxel 8360)
    want = G.step_scale(delta.to(F64), 0.25)
    got = ops.displacement_step_scale(delta.to(DEV), 0.25)
    rel = ((got.cpu().to(F64) - want) / want).abs()
    print(f"N = 256: largest relative error {float(rel.max()):.3e}  bar {8 * 2.0 ** -24:.3e}")
    assert float(rel.max()) <= 8 * 2.0 ** -24
    assert float(got[7]) == float(got[9]) == pytest.approx(0.25 / 75 ** 0.5, rel=1e-6)
    for n in (0, 7, 9, 255):
        assert torch.equal(ops.displacement_step_scale(delta[n:n + 1].to(DEV), 0.25)[0], got[n])


# ---- displacement_update -------------------------------------------------------------------------------------------------
def update_inputs(name, kind, scaled):
    disp, delta, outward = fields_of(name)
    scale = torch.tensor([0.75, 1.3]) if scaled else None
    return disp, (outward if kind == "outward" else delta), scale


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("kind", ["inside", "outward"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_update_matches_fp64(name, kind, scaled):
    """`outward` is the border clamp, the case an off-by-one in the coordinate gets wrong: every voxel of the outer three layers
    reads the border value of its face."""
    from keymorph_amd import ops
    disp, delta, scale = update_inputs(name, kind, scaled)
    ref = G.update(disp.to(F64), delta.to(F64), None if scale is None else scale.to(F64))
    low = G.update(disp, delta, scale)
    bar = 4 * float((low.to(F64) - ref).abs().max())
    got = ops.displacement_update(disp.to(DEV), delta.to(DEV), None if scale is None else scale.to(DEV))
    err = float((got.cpu().to(F64) - ref).abs().max())
    print(f"{name} {kind} scale={scaled}: update max abs error {err:.3e}  bar {bar:.3e}")
    assert got.shape == ref.shape and err <= bar


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_update_is_the_chain_of_existing_operators_and_repeats(name, scaled):
    """d + align_img(fields.from_displacement(d), disp), d = delta * scale, bit for bit: the same coordinate, the same blend8 on the
    same eight values, the product and the add rounded on their own.  Two runs and a batch against its samples are bit-equal."""
    from keymorph_amd import fields, ops
    from keymorph_amd.utils import align_img
    disp, delta, scale = (None if t is None else t.to(DEV) for t in update_inputs(name, "outward", scaled))
    got = ops.displacement_update(disp, delta, scale)
    d = delta if scale is None else delta * scale[:, None, None, None, None]
    assert torch.equal(got, d + align_img(fields.from_displacement(d), disp))
    assert torch.equal(got, ops.displacement_update(disp, delta, scale))
    for n in range(2):
        one = ops.displacement_update(disp[n:n + 1], delta[n:n + 1], None if scale is None else scale[n:n + 1])
        assert torch.equal(one[0], got[n])


def test_input_checks():
    from keymorph_amd import _lib, ops
    d = torch.zeros(2, 3, 8, 9, 10, device=DEV)
    mat = torch.zeros(2, 3, 4, device=DEV)
    s = torch.ones(2, device=DEV)
    assert ops.displacement_grid(d, mat).shape == (2, 8, 9, 10, 3)
    assert ops.displacement_update(d, d, s).shape == d.shape and ops.displacement_step_scale(d, 0.5).tolist() == [0.0, 0.0]
    with pytest.raises(_lib.KeymorphHipError):
        ops.displacement_grid(d.cpu())
    with pytest.raises(_lib.KeymorphHipError):
        ops.displacement_grid(d, mat.cpu())
    big = torch.zeros(1, device=DEV).expand(1, 3, 512, 1024, 1024)               # 3 x 2^29 floats: past one buffer descriptor
    for bad in (d.double(), d[0], d[:, :2], d.permute(0, 2, 3, 4, 1), big):
        with pytest.raises(ValueError):
            ops.displacement_grid(bad)
        with pytest.raises(ValueError):
            ops.displacement_step_scale(bad, 0.5)
        with pytest.raises(ValueError):
            ops.displacement_update(bad, bad)
    for bad_mat in (mat[:1], mat.double()):
        with pytest.raises(ValueError):
            ops.displacement_grid(d, bad_mat)
    with pytest.raises(ValueError):
        ops.displacement_grid(d[:, :, :, :1], mat)                                  # a matrix needs two voxels per axis
    with pytest.raises(RuntimeError):
        ops.displacement_grid(d, mat.clone().requires_grad_())
    with pytest.raises(ValueError):
        ops.displacement_update(d, d[:1])
    with pytest.raises(ValueError):
        ops.displacement_update(d, d, s[:1])
    with pytest.raises(ValueError):
        ops.displacement_step_scale(d, float("nan"))
    for k in range(3):
        args = [d, d, s]
        args[k] = args[k].clone().requires_grad_()
        with pytest.raises(RuntimeError):
            ops.displacement_update(*args)
    # the ABI's own limits: -22 before anything is launched
    lib = _lib.load()
    grid, out = torch.empty(2, 8, 9, 10, 3, device=DEV), torch.empty_like(d)
    p = lambda t: t.data_ptr()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    assert lib.kmh_disp_grid_fwd(p(d), None, p(grid), 2, 8, 9, 10, st) == 0
    assert lib.kmh_disp_grid_fwd(p(d), p(mat), p(grid), 2, 8, 1, 90, st) == -22
    assert lib.kmh_disp_grid_fwd(None, None, p(grid), 2, 8, 9, 10, st) == -22
    assert lib.kmh_disp_grid_fwd(p(d), None, p(grid), 1, 512, 1024, 1024, st) == -22
    assert lib.kmh_disp_grid_bwd(p(grid), None, p(out), 2, 8, 9, 10, st) == 0
    assert lib.kmh_disp_grid_bwd(p(grid), None, p(out), 70000, 8, 9, 10, st) == -22
    assert lib.kmh_disp_step_scale(p(d), 0.5, p(s), 2, 8, 0, 10, st) == -22
    assert lib.kmh_disp_step_scale(p(d), 0.5, None, 2, 8, 9, 10, st) == -22
    assert lib.kmh_disp_update(p(d), p(d), None, p(out), 2, 8, 9, 10, st) == 0
    assert lib.kmh_disp_update(p(d), p(out), None, p(d), 2, 8, 9, 10, st) == -22   # in place over the gathered field
    assert lib.kmh_disp_update(p(d), p(d), None, p(out), 0, 8, 9, 10, st) == -22
    torch.cuda.synchronize()


# ---- the driver ------------------------------------------------------------------------------------------------------------
def identity_mat(n=1):
    from keymorph_amd.io import voxel_to_mat
    return voxel_to_mat(torch.eye(3, device=DEV)[None].expand(n, 3, 3), torch.zeros(n, 3, device=DEV), (R.SIZE,) * 3)


@pytest.fixture(scope="module")
def recovery():
    """bspline_ref.recovery_pair() and register_greedy's answer with its defaults from the identity matrix."""
    from keymorph_amd.io import register_greedy
    fixed, moving = R.recovery_pair()
    mat = identity_mat()
    return fixed, moving, mat, register_greedy(fixed.to(DEV), moving.to(DEV), mat=mat)


def test_recovery(recovery):
    """Mean error at most half the identity's and no folded voxel; and the figure lies within 4 x d32 of the fp64 restatement's
    0.559081, d32 = dense_ref.fp32_distance(): the distance between the fp32 and the fp64 run of the restatement, measured on the
    CPU of the host that runs this test (3 s) because it is a property of the host -- 6.73e-4 where this test was written (bar
    2.69e-3), 1.93e-4 on a second host (bar 7.7e-4).  io.register_greedy on an MI355X: 0.559784, 7.03e-4 from the fp64 figure."""
    from keymorph_amd import loss_ops, ops
    fixed, _, mat, disp = recovery
    dims = tuple(fixed.shape[2:])
    grid = ops.displacement_grid(disp, mat)
    err = float(S.grid_error(grid, R.AMPLITUDE, dims)[0])
    start = float(S.grid_error(R.identity(dims)[None], R.AMPLITUDE, dims)[0])
    ref, ref_jac = G.RECOVERY_FP64[R.AMPLITUDE]
    jmin, folds = G.folded(disp)
    d32, e32 = G.fp32_distance()
    print(f"register_greedy: mean error {err:.6f} voxels (restatement: fp64 {ref:.6f}, fp32 on this host {e32:.6f}; distance "
          f"{abs(err - ref):.3e}, bar 4 x {d32:.3e} = {4 * d32:.3e}; identity {start:.4f}); minimum Jacobian {jmin:.4f} "
          f"(restatement {ref_jac:.4f}), {folds} folded")
    assert disp.shape == (1, 3, *dims) and disp.dtype == torch.float32
    assert err <= 0.5 * start
    assert loss_ops.jdlessthan0(disp) == 0 and folds == 0
    assert abs(err - ref) <= 4 * d32


def test_amplitude_8_does_not_fold():
    """svf_ref.min_jacobian reports no folded voxel and a positive minimum: the two conditions stated for this pair.  The distance
    bar of test_recovery belongs to the first pair's mean error: this pair's conditions are a count and a sign, which have no
    distance, and its mean error is printed beside the restatement's without a bar -- the fp32 and fp64 runs of the restatement
    happen to end 5.5e-7 voxels apart here (0.9914718 and 0.9914713), which measures a coincidence of two chaotic runs and not what
    fp32 costs (the same runs are 6.7e-4 apart on the other pair)."""
    from keymorph_amd import ops
    from keymorph_amd.io import register_greedy
    fixed, moving = S.recovery_pair(8.0)
    mat = identity_mat()
    dims = tuple(fixed.shape[2:])
    disp = register_greedy(fixed.to(DEV), moving.to(DEV), mat=mat)
    grid = ops.displacement_grid(disp, mat)
    lo, folded = S.min_jacobian(grid.cpu())
    err = float(S.grid_error(grid, 8.0, dims)[0])
    ref, ref_jac = G.RECOVERY_FP64[8.0]
    print(f"amplitude 8: register_greedy {folded} folded voxels, minimum Jacobian {lo:.4f} (fp64 restatement 0, {ref_jac:.4f}); "
          f"grid error {err:.7f} (restatement {ref:.6f})")
    assert folded == 0 and lo > 0


def test_batch_equals_single_runs_and_does_not_wait_for_the_gpu(recovery):
    from keymorph_amd.io import register_greedy
    fixed, moving, mat, _ = recovery
    f, m = fixed.to(DEV), moving.to(DEV)
    f2, m2 = (t.to(DEV) for t in R.recovery_pair(seed=4))
    kw = dict(shrink=(2, 1), iters=(4, 3))
    both = register_greedy(torch.cat([f, f2]), torch.cat([m, m2]), mat=identity_mat(2), **kw)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one = register_greedy(f, m, mat=mat, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(both[0], one[0]) and torch.equal(both[1], register_greedy(f2, m2, mat=mat, **kw)[0])
    assert torch.isfinite(both).all() and float(both.abs().max()) > 0


@pytest.mark.parametrize("metric", ["lncc", "mind"])
def test_local_metrics_improve(metric):
    from keymorph_amd import ops
    from keymorph_amd.io import apply_greedy, register_greedy
    fixed, moving = lncc_ref.biased_pair() if metric == "lncc" else mind_ref.inverted_pair()
    f, m, mat = fixed.to(DEV), moving.to(DEV), identity_mat()
    disp = register_greedy(f, m, mat=mat, iters=5, metric=metric)

    def measure(warped):                                            # higher is better
        if metric == "lncc":
            return float(ops.local_ncc(warped, f, 9)[0])
        return -float(ops.mind_ssc_loss(warped, f, 1, 2, ops.mind_bounds(m, f, 1, 2))[0])
    before, after = measure(apply_greedy(m, torch.zeros_like(disp), mat)), measure(apply_greedy(m, disp, mat))
    print(f"{metric}: similarity {before:.5f} -> {after:.5f} after 5 iterations per level")
    assert after > before


def test_refusals(recovery):
    from keymorph_amd.io import register_greedy
    fixed, moving, mat, _ = recovery
    f, m = fixed.to(DEV), moving.to(DEV)
    ones = torch.ones_like(f, dtype=torch.uint8)
    for metric in ("lncc", "mind"):
        for masks in (dict(fixed_mask=ones), dict(moving_mask=ones), dict(inside=True)):
            with pytest.raises(ValueError):
                register_greedy(f, m, mat=mat, metric=metric, iters=1, **masks)
    masked = register_greedy(f, m, mat=mat, iters=2, fixed_mask=ones, moving_mask=ones, inside=True)      # "mi" takes them
    assert torch.isfinite(masked).all()
    for kwargs in (dict(metric="ncc"), dict(step=0.0), dict(sigma_update=-1.0), dict(iters=(3, 3)), dict(iters=2.5),
                   dict(mat=identity_mat(2))):
        with pytest.raises(ValueError):
            register_greedy(f, m, **{"mat": mat, **kwargs})
    with pytest.raises(ValueError):
        register_greedy(f, m[..., :-1], mat=mat)


def test_apply_greedy(recovery):
    from keymorph_amd import ops
    from keymorph_amd.io import apply_greedy
    from keymorph_amd.utils import align_img
    fixed, moving, mat, disp = recovery
    f, m = fixed.to(DEV), moving.to(DEV)
    for mt in (None, mat):
        for mode in ("bilinear", "nearest", "cubic"):
            assert torch.equal(apply_greedy(m, disp, mt, mode), align_img(ops.displacement_grid(disp, mt), m, mode))
        labels = (m * 7).to(torch.int16)
        assert torch.equal(apply_greedy(labels, disp, mt, "label"), align_img(ops.displacement_grid(disp, mt), labels, "label"))
    before, after = float(ops.mutual_information(m, f, 32)[0]), float(ops.mutual_information(apply_greedy(m, disp, mat), f, 32)[0])
    print(f"mutual information with fixed: moving {before:.3f}, moving through the field {after:.3f}")
    assert after > before + 0.2


def test_intensity_registration_greedy_entry(recovery):
    from keymorph_amd import fields, ops
    from keymorph_amd.model import IntensityRegistration
    fixed, moving, _, _ = recovery
    f, m = fixed.to(DEV), moving.to(DEV)
    assert "greedy" in IntensityRegistration.supported_transform_type
    with torch.no_grad():
        res = IntensityRegistration(greedy_iters=20)(f, m, transform_type=["affine", "greedy"])
    r = res["greedy"]
    assert set(r) == {"grid", "inverse_grid", "matrix", "disp", "mi", "time"} and r["time"] > 0
    assert set(res["affine"]) == {"grid", "matrix", "mi", "time"}
    assert r["matrix"].shape == (1, 3, 4) and r["disp"].shape == (1, 3, 32, 32, 32) and r["mi"].shape == (1,)
    assert torch.equal(r["matrix"], res["affine"]["matrix"])                   # the affine it started from
    assert torch.equal(r["grid"], ops.displacement_grid(r["disp"], r["matrix"]))
    assert torch.equal(r["inverse_grid"], fields.invert(r["grid"]))
    print(f"MI: affine {float(res['affine']['mi'][0]):.4f}  greedy {float(r['mi'][0]):.4f}")
    assert float(r["mi"][0]) > float(res["affine"]["mi"][0])
    with torch.no_grad():
        r2 = IntensityRegistration(metric="lncc", greedy_iters=3, greedy_step=0.25, greedy_sigmas=(1.5, 0.5))(
            f, m, transform_type="greedy")["greedy"]
    assert set(r2) == {"grid", "inverse_grid", "matrix", "disp", "mi", "lncc", "time"}
    with pytest.raises(ValueError):
        IntensityRegistration(greedy_sigmas=1.0)
