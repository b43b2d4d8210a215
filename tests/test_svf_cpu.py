"""CPU: the restatement of the velocity-field exponential (tests/svf_ref.py) is itself pinned -- its limits (zero lattice, zero
steps), fp32 against fp64, its autograd against finite differences, its inverse -- and the conditions of the recovery pairs that
the GPU tests (tests/test_svf_gpu.py) rely on are validated for the fp64 restatement of the driver alone."""
import os
import re

import torch

from tests import bspline_ref as R
from tests import svf_ref as S
from tests import warp_mi_ref as W

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("kmh_bspline_disp_fwd", "kmh_svf_compose", "kmh_svf_finish_fwd", "kmh_svf_finish_bwd", "kmh_svf_square_bwd_ws_bytes",
           "kmh_svf_square_bwd")


def test_header_declares_and_library_exports_the_entries():
    from keymorph_amd import _lib, build
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "keymorph_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kmh_[a-z0-9_]+)\s*\(", txt))
    if not os.path.exists(build.LIBPATH):
        build.build()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.PROTOS and hasattr(lib, name), name
    assert lib.kmh_svf_square_bwd_ws_bytes(2, 5, 6, 7) == 2 * 5 * 6 * 7 * 32
    assert lib.kmh_svf_square_bwd_ws_bytes(0, 5, 6, 7) == 0 and lib.kmh_svf_square_bwd_ws_bytes(1, 1024, 1024, 512) == 0


def test_zero_lattice_is_the_base_and_zero_steps_is_the_free_form_grid():
    dims = (5, 6, 7)
    zero = torch.zeros(2, 3, 4, 4, 4, dtype=F64)
    mat = S.random_mats(2, 5)
    assert torch.equal(S.svf_grid(zero, dims, 6), R.identity(dims)[None].expand(2, *dims, 3))
    assert torch.equal(S.svf_grid(zero, dims, 6, mat), W.grid_of(mat, dims))
    ctrl = S.random_lattice(dims, 8, 1.5, 1, n=2)
    assert torch.equal(S.svf_grid(ctrl, dims, 0), R.bspline_grid(ctrl, dims))
    # with a matrix: the matrix applied to the deformed point, base + L (s * u); bspline_grid adds u to the base instead
    want = W.grid_of(mat, dims) + torch.einsum("nrk,ndhwk->ndhwr", mat[:, :, :3],
                                               R.displacement(ctrl, dims).flip(-1) * torch.tensor([5 / 4, 6 / 5, 7 / 6], dtype=F64)).flip(-1)
    assert torch.allclose(S.svf_grid(ctrl, dims, 0, mat), want, atol=1e-15)


def test_a_constant_velocity_is_a_translation():
    """v constant: every u_k is constant (the border clamp extends it), u_K = 2^K u_0 = v exactly."""
    dims = (9, 10, 13)
    ctrl = torch.zeros(1, 3, *R.lattice_shape(dims, 8), dtype=F64)
    ctrl[0, 0], ctrl[0, 1], ctrl[0, 2] = 0.25, -0.125, 0.0625
    d = S.displacements(ctrl, dims, 5)[-1]
    assert torch.allclose(d, torch.tensor([0.25, -0.125, 0.0625], dtype=F64).expand_as(d), atol=1e-14)


def test_fp32_restatement_is_close_to_fp64():
    dims = (16, 18, 20)
    for amp in (1.5, 5.0):
        ctrl = S.random_lattice(dims, 4, amp, 7, n=2)
        for mat in (None, S.random_mats(2, 5)):
            g64 = S.svf_grid(ctrl, dims, 6, mat)
            g32 = S.svf_grid(ctrl.float(), dims, 6, None if mat is None else mat.float())
            d = float((g32.double() - g64).abs().max())
            print(f"amplitude {amp} mat {mat is not None}: fp32 restatement max abs distance from fp64 {d:.3e}")
            assert d <= 1e-5


def test_more_steps_converge():
    dims = (16, 18, 20)
    ctrl = S.random_lattice(dims, 4, 5.0, 7)
    half = torch.tensor([dims[2] / 2, dims[1] / 2, dims[0] / 2], dtype=F64)
    g = {k: S.svf_grid(ctrl, dims, k) for k in (5, 6, 7, 8)}
    for k in (5, 7, 8):
        d = float(((g[k] - g[6]) * half).abs().max())
        print(f"K = {k} against K = 6: {d:.4f} voxel")
        assert d <= 0.05


def test_autograd_matches_finite_differences():
    dims, steps = (5, 6, 7), 3
    ctrl = S.random_lattice(dims, 8, 1.0, 3)
    mat = S.random_mats(1, 5)
    cot = torch.randn(1, *dims, 3, dtype=F64, generator=torch.Generator().manual_seed(4))
    for m in (None, mat):
        c = ctrl.clone().requires_grad_()
        (dc,) = torch.autograd.grad((S.svf_grid(c, dims, steps, m) * cot).sum(), c)
        picks = torch.topk(dc.abs().reshape(-1), 8).indices.tolist()
        h = 1e-6
        with torch.no_grad():
            for flat in picks:
                vals = []
                for sgn in (1.0, -1.0):
                    cp = ctrl.clone()
                    cp.reshape(-1)[flat] += sgn * h
                    vals.append(float((S.svf_grid(cp, dims, steps, m) * cot).sum()))
                fd = (vals[0] - vals[1]) / (2 * h)
                assert abs(fd - float(dc.reshape(-1)[flat])) <= 1e-6 * abs(fd) + 1e-8, (flat, fd, float(dc.reshape(-1)[flat]))


def test_inverse_grid_composes_to_the_identity_away_from_the_border():
    dims = (16, 18, 20)
    ctrl = S.random_lattice(dims, 4, 1.5, 7)
    fwd, inv = S.svf_grid(ctrl, dims, 6), S.inverse_grid(ctrl, dims, 6)
    half = torch.tensor([dims[2] / 2, dims[1] / 2, dims[0] / 2], dtype=F64)
    umax = float(((fwd - R.identity(dims)[None]) * half).abs().max())
    r = S.inverse_consistency(fwd, inv, umax)
    print(f"max |u| {umax:.3f} voxel, inverse consistency {r:.2e} voxel")
    assert r <= 0.05
    # with a matrix: P + U^-(P) undoes the matrix applied to the deformed point, exactly where nothing is clamped
    mat = W.voxel_to_mat(torch.eye(3, dtype=F64)[None] * 0.9, torch.tensor([[0.5, -0.25, 0.75]], dtype=F64), dims)
    from tests import fields_ref
    back = fields_ref.compose(S.inverse_grid(ctrl, dims, 6, mat), S.svf_grid(ctrl, dims, 6, mat))
    res = ((back - R.identity(dims)[None]) * half)[:, 4:-4, 4:-4, 4:-4].abs().max()
    assert float(res) <= 0.05


def test_default_recovery_pair_conditions_hold_for_the_fp64_restatement():
    """Size 32^3, lattice 7^3, amplitude 4, the defaults of io.register_svf, identity matrix: the mean displacement error of the final
    dense grid is at most 0.5 voxel and a third of the identity's, and no Jacobian is non-positive.
    (The restatement gives 0.287 voxel, the free-form restatement 0.285, the identity 1.786; minimum Jacobian 0.90.)"""
    fixed, moving = S.recovery_pair()
    f0, m0 = R.recovery_pair()
    assert torch.equal(fixed, f0) and torch.equal(moving, m0)                     # amplitude 4: bspline_ref's own pair
    dims = tuple(fixed.shape[2:])
    grid = S.svf_grid(S.recovery_run(), dims, 6)
    err = float(S.grid_error(grid, R.AMPLITUDE, dims)[0])
    start = float(S.grid_error(R.identity(dims)[None], R.AMPLITUDE, dims)[0])
    ffd, _ = R.recovery_run()
    lo, folded = S.min_jacobian(grid)
    print(f"fp64 restatement: error {err:.3f} voxel (free-form {ffd:.3f}, identity {start:.3f}); minimum Jacobian {lo:.3f}")
    assert err <= 0.5 and err <= start / 3 and folded == 0 and lo > 0


def test_amplitude_8_without_bending_folds_the_free_form_grid_and_not_the_exponential():
    """The same pair at amplitude 8 with bending = 0: the free-form restatement folds (60 voxels, minimum -0.35), the exponential of
    the lattice the SVF restatement finds does not (minimum 0.356)."""
    fixed, _ = S.recovery_pair(8.0)
    dims = tuple(fixed.shape[2:])
    lo_f, folded_f = S.min_jacobian(R.bspline_grid(S.ffd_run(8.0, 0.0), dims))
    lo_s, folded_s = S.min_jacobian(S.svf_grid(S.recovery_run(8.0, 0.0), dims, 6))
    print(f"free-form: {folded_f} folded voxels, minimum {lo_f:.3f}; exponential: {folded_s} folded, minimum {lo_s:.3f}")
    assert folded_f > 0 and lo_f <= 0
    assert folded_s == 0 and lo_s > 0


def test_the_inverse_brings_fixed_onto_moving():
    """apply_svf(fixed, ctrl, inverse=True) restated: the mutual information with moving rises (0.71 -> 1.19)."""
    import torch.nn.functional as F
    from tests import mi_ref
    fixed, moving = S.recovery_pair()
    dims = tuple(fixed.shape[2:])
    inv = S.inverse_grid(S.recovery_run(), dims, 6)
    back = F.grid_sample(fixed.double(), inv, mode="bilinear", padding_mode="border", align_corners=False)
    before = float(mi_ref.mutual_information(fixed.double(), moving.double(), 32)[0])
    after = float(mi_ref.mutual_information(back, moving.double(), 32)[0])
    print(f"mutual information with moving: fixed {before:.3f}, fixed through the inverse {after:.3f}")
    assert after > before + 0.2
