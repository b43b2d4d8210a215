"""GPU: ops.warp_mutual_information / ops.mi_ranges / loss_ops.WarpMILoss (csrc/warp_mi.hip) and what is built on them
(keymorph_amd.io.register_intensity, model.IntensityRegistration).

Forward.  The fused pass builds the joint table from the same quantised products as the chain affine_grid -> align_img ->
mutual_information with given ranges, and integer sums do not depend on the order: MI and G are torch.equal to the chain's.

Backward.  dmat against fp64 autograd of the restatement (tests/warp_mi_ref.py) with the ranges held fixed, relative L2 over the
12 entries.  The bar is the larger of 4 x d32 (the restatement evaluated in fp32 on the CPU against its fp64 evaluation, same
case: what fp32 costs in any order, times 4 for another order) and the accumulation format's floor (tests/test_mi_gpu.py's
per-voxel bound on dMI/da_v pushed through |da_v / dmat| and normalised by the fp64 gradient's norm).  Both come from the
restatement; nothing comes from the kernel.  The identity matrix is left out of THIS comparison only: every coordinate is a
lattice point there, where the trilinear blend has a kink, and which side fp32 and fp64 rounding fall on is not a property of
the operator.  There dmat (floor()'s side, the clamp mask at the first and last voxel centre) is held against the unfused
chain's dmat instead, which samples at the same coordinates bit for bit, within a bound for fp32 summation order
(test_identity_matrix_gradient_equals_the_chains); its forward, repeat and batch properties are tested like the others'.

Measured on an MI355X (relative L2 of dmat: kernel / unfused chain / d32 / floor):
  see DESIGN.md section 8d."""
import functools
import math

import pytest
import torch

from tests import mi_ref
from tests import warp_mi_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

SHAPES = {
    "tiny_ragged": (1, 1, 5, 6, 7),            # fewer voxels than one workgroup
    "odd_box": (1, 1, 24, 20, 36),
    "two_flushes": (1, 1, 40, 40, 40),         # several workgroups, two flushes of the LDS tables each
    "batch": (2, 1, 16, 16, 16),               # another matrix and another intensity range per sample
}
MATS = ("identity", "affine", "outside")
# name -> (shape, matrix, bins)
CASES = {f"{s}-{m}": (s, m, 32) for s in SHAPES for m in MATS}
CASES.update({"odd_box-affine-bins8": ("odd_box", "affine", 8), "odd_box-affine-bins64": ("odd_box", "affine", 64),
              "two_flushes-outside-bins64": ("two_flushes", "outside", 64)})
GRAD_CASES = [c for c in CASES if CASES[c][1] != "identity"]


def _pair(shape, seed):
    a, b = mi_ref.smooth_pair(shape, seed)
    for n in range(1, shape[0]):                       # another range per sample
        a[n] = a[n] * (3.0 * n) - 7.0
        b[n] = b[n] * 0.125 + 100.0 * n
    return a, b


def _matrix(kind, dims, n):
    """Sample n's (3, 4) matrix, float32 on the CPU."""
    from keymorph_amd import synthetic
    eye = torch.eye(3, dtype=F64)[None]
    if kind == "identity":                             # every coordinate a lattice point
        return W.voxel_to_mat(eye, torch.zeros(1, 3, dtype=F64), dims)[0].float()
    if kind == "affine":                               # rotation + shear + scale + shift
        return synthetic.random_affine_matrix(5 + n, "cpu")[0, :3, :].contiguous()
    # a third of the lattice pushed outside [-1, 1] (border clamp, zero multipliers), slightly turned
    t = torch.zeros(1, 3, dtype=F64)
    t[0, 2 - n] = dims[2 - n] / 3.0 * (1 if n == 0 else -1)
    t[0, n] += 0.3
    return W.voxel_to_mat(W.rotation([0.03, -0.02, 0.04])[None], t, dims)[0].float()


@functools.lru_cache(maxsize=None)
def inputs(name):
    shape_name, kind, bins = CASES[name]
    shape = SHAPES[shape_name]
    moving, fixed = _pair(shape, 3 + len(shape_name))
    mat = torch.stack([_matrix(kind, shape[2:], n) for n in range(shape[0])])
    return moving, fixed, mat, bins


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 and fp32 evaluations of the restatement and the bars of one case, computed once."""
    moving, fixed, mat, bins = inputs(name)
    ranges = W.own_ranges(moving, fixed)
    mi64, g64 = W.evaluate(moving, fixed, mat, bins, F64, ranges)
    _, g32 = W.evaluate(moving, fixed, mat, bins, torch.float32, ranges)
    floors = W.dmat_floor(moving, fixed, mat, bins, ranges, g64)
    d32 = [float((g32[n].to(F64) - g64[n]).norm() / g64[n].norm()) for n in range(mat.shape[0])]
    return mi64, g64, d32, floors


def fused(moving, fixed, mat, bins, grad=True):
    from keymorph_amd import ops
    m = mat.to(DEV).requires_grad_(grad)
    mi, G = ops._warp_mi_table(moving.to(DEV), fixed.to(DEV), m, bins)
    out = ops.warp_mutual_information(moving.to(DEV), fixed.to(DEV), m, bins)
    if grad:
        out.sum().backward()
    return out.detach(), G, m.grad


def chain(moving, fixed, mat, bins, grad=True):
    """The unfused operators, sample by sample with the volumes' own ranges: (mi (N,), G (N, B, B), dmat (N, 3, 4))."""
    from keymorph_amd import ops
    from keymorph_amd.utils import align_img
    dims = moving.shape[2:]
    ranges = W.own_ranges(moving, fixed)
    mis, Gs, gs = [], [], []
    for n in range(moving.shape[0]):
        m = mat[n:n + 1].to(DEV).requires_grad_(grad)
        mo, fi = moving[n:n + 1].to(DEV), fixed[n:n + 1].to(DEV)
        mi, G = ops._mi_table(align_img(ops.affine_grid(m.detach(), dims), mo), fi, bins, ranges[n][0], ranges[n][1])
        if grad:
            ops.mutual_information(align_img(ops.affine_grid(m, dims), mo), fi, bins, ranges[n][0], ranges[n][1]).sum().backward()
            gs.append(m.grad)
        mis.append(mi)
        Gs.append(G)
    return torch.cat(mis), torch.cat(Gs), (torch.cat(gs) if grad else None)


# ---- the operator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_forward_equals_the_unfused_chain_bit_for_bit(name):
    moving, fixed, mat, bins = inputs(name)
    mi, G, _ = fused(moving, fixed, mat, bins, grad=False)
    mi_c, G_c, _ = chain(moving, fixed, mat, bins, grad=False)
    assert mi.dtype == torch.float32 and mi.shape == (moving.shape[0],) and G.shape == (moving.shape[0], bins, bins)
    assert float(mi.min()) > 0 and torch.equal(mi, mi_c) and torch.equal(G, G_c)


def test_ranges_are_those_of_the_volumes():
    from keymorph_amd import ops
    moving, fixed, mat, bins = inputs("batch-affine")
    rng = ops.mi_ranges(moving.to(DEV), fixed.to(DEV), bins).cpu()
    assert rng.shape == (2, 4) and rng.dtype == torch.float32
    for n, ((lo_a, hi_a), (lo_b, hi_b)) in enumerate(W.own_ranges(moving, fixed)):
        assert float(rng[n, 0]) == lo_a and float(rng[n, 2]) == lo_b
        # s = (bins - 3) / (hi - lo): the difference of two floats is rounded once, the device's quotient to within an ulp
        for got, lo, hi in ((float(rng[n, 1]), lo_a, hi_a), (float(rng[n, 3]), lo_b, hi_b)):
            want = (bins - 3) / float(torch.tensor(hi) - torch.tensor(lo))
            assert abs(got - want) <= 2.0 ** -22 * want
    given = ops.warp_mutual_information(moving.to(DEV), fixed.to(DEV), mat.to(DEV), bins, rng.to(DEV))
    assert torch.equal(given, ops.warp_mutual_information(moving.to(DEV), fixed.to(DEV), mat.to(DEV), bins))


@pytest.mark.parametrize("name", GRAD_CASES)
def test_matrix_gradient_matches_fp64(name):
    moving, fixed, mat, bins = inputs(name)
    mi64, g64, d32, floors = reference(name)
    mi, _, dmat = fused(moving, fixed, mat, bins)
    _, _, dchain = chain(moving, fixed, mat, bins)
    assert dmat.shape == mat.shape and dmat.dtype == torch.float32
    for n in range(mat.shape[0]):
        err = float((dmat[n].cpu().to(F64) - g64[n]).norm() / g64[n].norm())
        err_c = float((dchain[n].cpu().to(F64) - g64[n]).norm() / g64[n].norm())
        bar = max(4 * d32[n], floors[n])
        print(f"{name}[{n}]: MI {float(mi64[n]):.6f}  relL2 dmat: kernel {err:.3e}  unfused chain {err_c:.3e}  fp32-CPU distance "
              f"{d32[n]:.3e}  format floor {floors[n]:.3e}  bar {bar:.3e}")
        assert abs(float(mi[n]) - float(mi64[n])) <= 1e-4
        assert err <= bar, (name, n, err, d32[n], floors[n])


@pytest.mark.parametrize("name", [c for c in CASES if CASES[c][1] == "identity"])
def test_identity_matrix_gradient_equals_the_chains(name):
    """voxel_to_mat(I, 0): every coordinate is a lattice point, so the cell floor() picks and the clamp mask at the first and last
    voxel centre decide the gradient.  The fused pass and the chain sample at the same coordinates bit for bit (the forward test),
    so both pick the same cells and masks and add the same per-voxel terms; they differ in the order of the fp32 sums and in how
    each call site rounds a term.  Per entry, with S and X of warp_mi_ref.lattice_term_sums (from the fp64 restatement):
      |dmat - chain| <= 2^-24 ((2 (n - 1) + 4) S + 16 X)
    n = 16 terms per lane in both reductions at these sizes (ceil(V / 4096) workgroups of 256 lanes, then fp64): each path's
    fp32 sum is within (n - 1) 2^-24 of sum |term|; four roundings in a term's product chain, both paths; and the blend's
    derivative subtracts eight corner values of size <= max |moving|, each path within 8 roundings of THAT size.  A wrong mask or
    cell changes whole terms: the border voxels alone carry about 2 / n_r of S."""
    moving, fixed, mat, bins = inputs(name)
    S, X = W.lattice_term_sums(moving, fixed, bins, W.own_ranges(moving, fixed))
    _, _, dmat = fused(moving, fixed, mat, bins)
    _, _, dchain = chain(moving, fixed, mat, bins)
    tol = 2.0 ** -24 * ((2 * 15 + 4) * S + 16 * X)
    for n in range(mat.shape[0]):
        diff = (dmat[n].cpu().to(F64) - dchain[n].cpu().to(F64)).abs()
        print(f"{name}[{n}]: |dmat| {float(dchain[n].norm()):.3e}  max |fused - chain| {float(diff.max()):.3e}  "
              f"max of bound {float(tol[n].max()):.3e}  largest ratio {float((diff / tol[n]).max()):.3e}")
        assert float(dchain[n].norm()) > 0 and bool((diff <= tol[n]).all()), (name, n, diff, tol[n])


def test_matrix_gradient_matches_finite_differences():
    """All 12 entries of dmat at 16^3 against central differences of the fp64 restatement with the ranges held fixed; the bar of
    test_mi_gpu.py::test_gradient_through_align_img_matches_finite_differences.  The step is 1e-7: an entry of the matrix moves
    all 4096 coordinates at once, and a coordinate that crosses a lattice plane inside the step meets the trilinear blend's kink,
    which costs the difference quotient an error proportional to the step (against the restatement's own autograd gradient:
    3.4 bars at 1e-5, 5e-5 of a bar at 1e-7; rounding of the fp64 differences is 1e-9 there)."""
    from keymorph_amd import synthetic
    S = 16
    moving, fixed = _pair((1, 1, S, S, S), 8)
    mat = synthetic.random_affine_matrix(5, "cpu")[:, :3, :].contiguous()
    _, _, dmat = fused(moving, fixed, mat, 32)
    ranges = W.own_ranges(moving, fixed)
    m64, f64 = moving.to(F64), fixed.to(F64)
    h = 1e-7
    for r in range(3):
        for k in range(4):
            vals = []
            for sgn in (1.0, -1.0):
                mp = mat.to(F64).clone()
                mp[0, r, k] += sgn * h
                vals.append(float(W.warp_mi(m64, f64, mp, 32, ranges)[0]))
            fd = (vals[0] - vals[1]) / (2 * h)
            got = float(dmat[0, r, k])
            print(f"mat[{r}][{k}]: kernel {got:.6e}  finite difference {fd:.6e}")
            assert math.isfinite(got) and abs(got - fd) <= 2e-3 * abs(fd) + 1e-6, (r, k, got, fd)


@pytest.mark.parametrize("name", ["two_flushes-affine", "batch-outside", "tiny_ragged-identity"])
def test_repeat_runs_are_bit_identical(name):
    moving, fixed, mat, bins = inputs(name)
    first = fused(moving, fixed, mat, bins)
    again = fused(moving, fixed, mat, bins)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_batch_equals_single_samples():
    moving, fixed = _pair((3, 1, 24, 20, 36), 11)
    mat = torch.stack([_matrix(k, (24, 20, 36), n) for n, k in enumerate(("affine", "outside", "identity"))])
    mi, G, dmat = fused(moving, fixed, mat, 32)
    for n in range(3):
        mi1, G1, d1 = fused(moving[n:n + 1], fixed[n:n + 1], mat[n:n + 1], 32)
        assert torch.equal(mi[n:n + 1], mi1) and torch.equal(G[n:n + 1], G1) and torch.equal(dmat[n:n + 1], d1)


def test_constant_volume_gives_exact_zeros():
    moving, fixed, mat, bins = inputs("odd_box-affine")
    for mo, fi in ((torch.full_like(moving, 0.75), fixed), (moving, torch.full_like(fixed, -2.0))):
        mi, G, dmat = fused(mo, fi, mat, bins)
        assert torch.equal(mi, torch.zeros_like(mi)) and torch.equal(G, torch.zeros_like(G))
        assert torch.equal(dmat, torch.zeros_like(dmat))


def test_no_gradient_unless_asked_and_the_loss_is_minus_the_mean():
    from keymorph_amd import ops
    from keymorph_amd.loss_ops import WarpMILoss
    moving, fixed, mat, bins = inputs("batch-affine")
    mo, fi, m = moving.to(DEV), fixed.to(DEV), mat.to(DEV)
    out = ops.warp_mutual_information(mo, fi, m, bins)
    assert not out.requires_grad and m.grad is None
    mo.requires_grad_(True)                            # the volumes are data: no gradient reaches them
    mg = m.clone().requires_grad_(True)
    loss = WarpMILoss(bins)(mo, fi, mg)
    loss.backward()
    assert mo.grad is None and mg.grad is not None
    assert loss.shape == () and torch.equal(loss.detach(), -out.mean())
    _, _, dmat = fused(moving, fixed, mat, bins)
    assert torch.allclose(mg.grad, -dmat / 2, rtol=1e-6, atol=0)


def test_input_checks():
    from keymorph_amd import _lib, ops
    moving, fixed, mat, _ = inputs("batch-affine")
    mo, fi, m = moving.to(DEV), fixed.to(DEV), mat.to(DEV)
    with pytest.raises(_lib.KeymorphHipError):
        ops.warp_mutual_information(moving, fi, m)
    with pytest.raises(_lib.KeymorphHipError):
        ops.warp_mutual_information(mo, fi, mat)
    with pytest.raises(_lib.KeymorphHipError):
        ops.mi_ranges(mo, fixed)
    with pytest.raises(ValueError):
        ops.warp_mutual_information(mo.double(), fi, m)
    with pytest.raises(ValueError):
        ops.warp_mutual_information(mo, fi, m.double())
    with pytest.raises(ValueError):
        ops.warp_mutual_information(mo, fi[:1], m)
    with pytest.raises(ValueError):
        ops.warp_mutual_information(mo[:, 0], fi[:, 0], m)
    with pytest.raises(ValueError):
        ops.warp_mutual_information(mo[..., :1], fi[..., :1], m)                       # W >= 2
    for bins in (7, 65, 8.5):
        with pytest.raises(ValueError):
            ops.warp_mutual_information(mo, fi, m, bins)
        with pytest.raises(ValueError):
            ops.mi_ranges(mo, fi, bins)
    for bad in (m[:1], m[:, :, :3], m.reshape(2, 12), torch.eye(4, device=DEV).expand(2, 4, 4)):
        with pytest.raises(ValueError):
            ops.warp_mutual_information(mo, fi, bad)
    with pytest.raises(ValueError):
        ops.warp_mutual_information(mo, fi, m, 32, torch.zeros(2, 3, device=DEV))
    lib = _lib.load()                                   # the ABI's own checks
    rng = ops.mi_ranges(mo, fi)
    ws = torch.empty(int(lib.kmh_warp_mi_ws_bytes(2, 32, 16, 16, 16)), dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for D, H, Wd, bins in ((16, 16, 1, 32), (16, 16, 16, 7), (16, 16, 16, 65), (1024, 1024, 1024, 32)):
        assert lib.kmh_warp_mi_hist(mo.data_ptr(), fi.data_ptr(), m.data_ptr(), rng.data_ptr(), 2, D, H, Wd, bins, ws.data_ptr(),
                                    s) == -22


# ---- the driver ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rigid_runs():
    """The pairs validated in tests/test_warp_mi_cpu.py at 32^3 and register_intensity's answers with its defaults."""
    from keymorph_amd.io import register_intensity
    out = {}
    for name in W.RIGID_CASES:
        fixed, moving, L, t = W.rigid_pair(name, 32)
        out[name] = (fixed, moving, L, t, register_intensity(fixed.to(DEV), moving.to(DEV), "rigid").cpu())
    return out


@pytest.mark.parametrize("name", list(W.RIGID_CASES))
def test_rigid_registration_recovers_the_motion(rigid_runs, name):
    from keymorph_amd.io import mat_to_voxel
    fixed, moving, L, t, mat = rigid_runs[name]
    err = float(W.mean_displacement(mat, L, t, fixed.shape[2:])[0])
    start = float(W.mean_displacement(W.voxel_to_mat(torch.eye(3)[None], torch.zeros(1, 3), fixed.shape[2:]), L, t,
                                      fixed.shape[2:])[0])
    print(f"{name}: mean displacement {err:.3f} voxel (identity: {start:.3f})")
    assert mat.shape == (1, 3, 4) and err <= 0.5
    Le = mat_to_voxel(mat.double(), fixed.shape[2:])[0][0]                  # a rotation: spacing (1, 1, 1)
    assert float((Le @ Le.t() - torch.eye(3, dtype=F64)).abs().max()) <= 1e-5


def test_translation_registration_recovers_the_shift():
    from keymorph_amd.io import register_intensity
    fixed, moving = mi_ref.recovery_pair(32)
    mat = register_intensity(fixed.to(DEV), moving.to(DEV), "translation").cpu()
    t = torch.tensor([mi_ref.RECOVERY_SHIFT], dtype=F64)
    err = float(W.mean_displacement(mat, torch.eye(3, dtype=F64)[None], t, fixed.shape[2:])[0])
    print(f"translation: mean displacement {err:.3f} voxel")
    assert err <= 0.5


def test_affine_registration_recovers_the_scale_too():
    from keymorph_amd.io import estimate_affine
    fixed, moving, L, t = W.affine_pair(32)
    mat = estimate_affine(fixed.to(DEV), moving.to(DEV)).cpu()
    err = float(W.mean_displacement(mat, L, t, fixed.shape[2:])[0])
    print(f"affine: mean displacement {err:.3f} voxel")
    assert err <= 0.5


def test_registration_batch_equals_single_runs(rigid_runs):
    from keymorph_amd.io import estimate_rigid
    a, b = (rigid_runs[name] for name in W.RIGID_CASES)
    mat = estimate_rigid(torch.cat([a[0], b[0]]).to(DEV), torch.cat([a[1], b[1]]).to(DEV)).cpu()
    assert torch.equal(mat[0], a[4][0]) and torch.equal(mat[1], b[4][0])


def test_registration_does_not_wait_for_the_gpu(rigid_runs):
    """One full-resolution level of every stage up to rigid under torch's synchronisation check, after a first call that
    allocates."""
    from keymorph_amd.io import register_intensity
    fixed, moving = rigid_runs["rigid_a"][:2]
    f, m = fixed.to(DEV), moving.to(DEV)
    first = register_intensity(f, m, "rigid", shrink=(1,), iters=3)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = register_intensity(f, m, "rigid", shrink=(1,), iters=3)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(first, again)


def test_apply_mat_is_the_grid_and_the_sampler():
    from keymorph_amd import ops
    from keymorph_amd.io import apply_mat
    from keymorph_amd.utils import align_img
    moving, _, mat, _ = inputs("odd_box-affine")
    out = apply_mat(moving.to(DEV), mat.to(DEV))
    assert torch.equal(out, align_img(ops.affine_grid(mat.to(DEV), moving.shape[2:]), moving.to(DEV)))
    near = apply_mat(moving.to(DEV), mat.to(DEV), "nearest")
    assert torch.equal(near, align_img(ops.affine_grid(mat.to(DEV), moving.shape[2:]), moving.to(DEV), "nearest"))


def test_voxel_to_mat_of_the_identity_is_translate():
    """translate(x, t) is the case L = I: the same matrix, hence the same output bit for bit, in both modes."""
    from keymorph_amd.io import apply_mat, translate, voxel_to_mat
    x = torch.rand(2, 2, 9, 12, 10, generator=torch.Generator().manual_seed(0)).to(DEV)
    t = torch.tensor([[1.25, -2.5, 0.75], [-0.4, 3.0, -1.1]], device=DEV)
    mat = voxel_to_mat(torch.diag_embed(torch.ones_like(t)), t, x.shape[2:])
    for mode in ("bilinear", "nearest"):
        assert torch.equal(apply_mat(x, mat, mode), translate(x, t, mode))


# ---- the model-shaped wrapper ------------------------------------------------------------------------------------------------
def test_intensity_registration_has_keymorphs_call_surface(rigid_runs, monkeypatch):
    from keymorph_amd import ops
    from keymorph_amd.model import IntensityRegistration
    from keymorph_amd.utils import align_img
    fixed, moving = rigid_runs["rigid_a"][:2]
    f, m = fixed.to(DEV), moving.to(DEV)
    model = IntensityRegistration()
    assert len(list(model.parameters())) == 0
    with torch.no_grad():
        res = model(f, m, transform_type=["translation", "rigid", "affine"], return_aligned_points=False, aff_f=None)
    before = float(ops.mutual_information(m, f)[0])
    for kind in ("translation", "rigid", "affine"):
        r = res[kind]
        assert set(r) == {"grid", "matrix", "mi", "time"} and r["time"] > 0
        assert r["matrix"].shape == (1, 3, 4) and r["grid"].shape == (1, 32, 32, 32, 3) and r["mi"].shape == (1,)
        assert torch.equal(r["grid"], ops.affine_grid(r["matrix"], (32, 32, 32)))
        after = float(ops.mutual_information(align_img(r["grid"], m), f)[0])
        print(f"{kind}: MI {before:.4f} -> {after:.4f}")
        assert after > before
    assert torch.equal(res["rigid"]["matrix"].cpu(), rigid_runs["rigid_a"][4])
    with pytest.raises(AssertionError):
        model(f, m, transform_type="tps_1")
    # num_resolutions_for_itkelastix = k: the pyramid 2^(k-1) .. 1, one mi_ranges call per level
    calls = []
    real = ops.mi_ranges
    monkeypatch.setattr(ops, "mi_ranges", lambda a, b, bins=32: calls.append(tuple(a.shape[2:])) or real(a, b, bins))
    quick = IntensityRegistration(iters=2)
    quick(f, m, transform_type="translation", num_resolutions_for_itkelastix=2)
    assert calls == [(16, 16, 16), (32, 32, 32)]
    calls.clear()
    quick(f, m, transform_type="translation", num_resolutions_for_itkelastix=1)
    assert calls == [(32, 32, 32)]
