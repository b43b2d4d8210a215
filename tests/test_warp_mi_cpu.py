"""CPU: the parameterisations of keymorph_amd.io.intensity (plain torch) and the inputs of the GPU recovery tests, validated on the
fp64 restatement of tests/warp_mi_ref.py alone."""
import math

import pytest
import torch

from tests import mi_ref
from tests import warp_mi_ref as W

F64 = torch.float64


def test_voxel_to_mat_of_the_identity_is_translates_matrix():
    """The formula of translate()'s docstring (io/centering.py), diag((n - 1) / n) and offsets 2 t / n in fp32: the same numbers,
    bit for bit.  translate() itself runs only on the GPU: tests/test_warp_mi_gpu.py compares its output with apply_mat's."""
    from keymorph_amd.io import voxel_to_mat
    dims = (9, 12, 10)
    t = torch.tensor([[1.25, -2.5, 0.75], [-0.4, 3.0, -1.1]])
    lin = t.new_zeros((2, 3, 3))
    for k, n in enumerate(dims):
        lin[:, k, k] = (n - 1) / n
    off = torch.stack([t[:, k] * (2.0 / n) for k, n in enumerate(dims)], dim=1)
    want = torch.cat([lin, off.unsqueeze(-1)], dim=2)
    got = voxel_to_mat(torch.eye(3).expand(2, 3, 3), t, dims)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.allclose(got.double(), W.voxel_to_mat(torch.eye(3, dtype=F64).expand(2, 3, 3), t, dims), rtol=0, atol=1e-7)


def test_integer_shift_is_an_exact_voxel_shift():
    from keymorph_amd.io import voxel_to_mat
    x = torch.rand(1, 1, 6, 7, 8, dtype=F64, generator=torch.Generator().manual_seed(0))
    mat = voxel_to_mat(torch.eye(3, dtype=F64)[None], torch.tensor([[1.0, -2.0, 3.0]], dtype=F64), (6, 7, 8))
    out = W.warp(x, mat)
    assert torch.allclose(out[0, 0, :5, 2:, :5], x[0, 0, 1:, :5, 3:], rtol=0, atol=1e-14)
    assert torch.allclose(out, mi_ref.translate(x, torch.tensor([[1.0, -2.0, 3.0]], dtype=F64)), rtol=0, atol=1e-14)


def test_general_map_reads_where_it_says():
    """voxel_to_mat(L, t) makes output voxel v read c + L (v - c) + t: the grid's voxel coordinates are that map."""
    from keymorph_amd.io import voxel_to_mat
    dims = (7, 9, 11)
    g = torch.Generator().manual_seed(1)
    L = torch.eye(3, dtype=F64)[None] + 0.2 * (torch.rand(2, 3, 3, generator=g, dtype=F64) - 0.5)
    t = 3 * (torch.rand(2, 3, generator=g, dtype=F64) - 0.5)
    mat = voxel_to_mat(L, t, dims)
    assert torch.allclose(mat, W.voxel_to_mat(L, t, dims), rtol=0, atol=1e-14)
    assert float((W.mat_voxel_map(mat, dims) - W.voxel_map(L, t, dims)).abs().max()) <= 1e-12


def test_mat_to_voxel_inverts_voxel_to_mat():
    from keymorph_amd.io import mat_to_voxel, voxel_to_mat
    dims = (5, 8, 13)
    g = torch.Generator().manual_seed(2)
    L, t = torch.rand(3, 3, 3, generator=g, dtype=F64), torch.rand(3, 3, generator=g, dtype=F64)
    L2, t2 = mat_to_voxel(voxel_to_mat(L, t, dims), dims)
    assert torch.allclose(L2, L, rtol=0, atol=1e-14) and torch.allclose(t2, t, rtol=0, atol=1e-14)
    with pytest.raises(ValueError):
        voxel_to_mat(L[:, :2], t, dims)
    with pytest.raises(ValueError):
        mat_to_voxel(torch.zeros(1, 3, 4), (1, 4, 4))


def test_rotation_vector_gives_a_rotation():
    from keymorph_amd.io import rotation_matrix
    omega = torch.tensor([[0.3, -0.2, 0.5], [0.0, 0.0, 0.0], [1e-7, 0.0, 0.0], [0.0, 2.0, -1.0]], dtype=F64)
    R = rotation_matrix(omega)
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=F64)).abs().max()) <= 1e-14
    assert torch.allclose(torch.linalg.det(R), torch.ones(4, dtype=F64), rtol=0, atol=1e-14)
    for n in range(4):
        assert torch.allclose(R[n], W.rotation(omega[n].tolist()), rtol=0, atol=1e-12)
    # differentiable at zero: the generators
    w = torch.zeros(1, 3, dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(rotation_matrix(w)[0, 2, 1], w)
    assert torch.allclose(g, torch.tensor([[1.0, 0.0, 0.0]], dtype=F64), rtol=0, atol=1e-12)


def test_anisotropic_spacing_still_rotates_in_millimetres():
    from keymorph_amd.io import rigid_params_to_voxel
    spacing = (1.0, 1.0, 3.0)
    omega = torch.tensor([[0.2, -0.4, 0.1]], dtype=F64)
    t = torch.tensor([[0.5, 1.0, -2.0]], dtype=F64)
    L, t2 = rigid_params_to_voxel(omega, t, spacing)
    S = torch.diag(torch.tensor(spacing, dtype=F64))
    P = S @ L[0] @ torch.linalg.inv(S)                       # the physical map
    assert float((P @ P.t() - torch.eye(3, dtype=F64)).abs().max()) <= 1e-14 and abs(float(torch.linalg.det(P)) - 1) <= 1e-14
    assert torch.allclose(P, W.rotation(omega[0].tolist()), rtol=0, atol=1e-12) and torch.equal(t2, t)
    assert float((L[0] @ L[0].t() - torch.eye(3, dtype=F64)).abs().max()) > 1e-2        # and not a rotation of the voxel lattice


def _mi_at(f64, m64, L, t, ranges):
    return float(W.warp_mi(m64, f64, W.voxel_to_mat(L, t, f64.shape[2:]), 32, ranges)[0])


def _assert_peak(fixed, moving, L, t):
    """MI at the true transform exceeds MI at the transform perturbed by +-1 voxel-equivalent in each of the six rigid parameters:
    a shift of one voxel per axis, a rotation of 1 / h radians per axis, h = (n - 1) / 2 the half-extent."""
    f64, m64 = fixed.to(F64), moving.to(F64)
    ranges = W.own_ranges(moving, fixed)
    h = (fixed.shape[2] - 1) / 2
    top = _mi_at(f64, m64, L, t, ranges)
    for k in range(3):
        for sgn in (1.0, -1.0):
            e = [0.0, 0.0, 0.0]
            e[k] = sgn
            shifted = _mi_at(f64, m64, L, t + torch.tensor([e], dtype=F64), ranges)
            turned = _mi_at(f64, m64, (W.rotation([v / h for v in e]) @ L[0])[None], t, ranges)
            print(f"axis {k} {sgn:+.0f}: MI true {top:.5f}  shifted {shifted:.5f}  turned {turned:.5f}")
            assert top > shifted and top > turned


@pytest.mark.parametrize("name", list(W.RIGID_CASES))
def test_rigid_recovery_inputs(name):
    """The inputs of the GPU recovery tests at 32^3, validated on the restatement alone: what makes 'mean displacement <= 0.5
    voxel' a reachable bar."""
    fixed, moving, L, t = W.rigid_pair(name, 32)
    assert fixed.shape == moving.shape == (1, 1, 32, 32, 32) and fixed.dtype == torch.float32
    _assert_peak(fixed, moving, L, t)


def test_affine_recovery_inputs():
    """The affine pair: the six rigid parameters as above, and a scale of +-1 voxel-equivalent (1 / h) along each axis.  The
    texture has no background: over the rigid pairs' blobs the maximum of MI sits at a scale 4 % below the true one (it rewards
    zooming in on the structure), which no optimiser can be asked to miss."""
    fixed, moving, L, t = W.affine_pair(32)
    _assert_peak(fixed, moving, L, t)
    f64, m64 = fixed.to(F64), moving.to(F64)
    ranges = W.own_ranges(moving, fixed)
    top = _mi_at(f64, m64, L, t, ranges)
    h = (fixed.shape[2] - 1) / 2
    for k in range(3):
        for sgn in (1.0, -1.0):
            D = torch.eye(3, dtype=F64)
            D[k, k] += sgn / h
            scaled = _mi_at(f64, m64, L @ D[None], t, ranges)
            print(f"scale axis {k} {sgn:+.0f}: MI true {top:.5f}  scaled {scaled:.5f}")
            assert top > scaled
    # and the scale is visible: undoing it (the rigid part alone) scores lower
    rigid = L @ torch.diag(1 / torch.tensor(W.AFFINE_SCALE, dtype=F64))[None]
    assert top > _mi_at(f64, m64, rigid, t, ranges)


def test_moved_pair_with_a_shift_is_the_translation_pair():
    f, m = W.moved_pair(24, torch.eye(3, dtype=F64), torch.tensor(mi_ref.RECOVERY_SHIFT, dtype=F64), 5)
    f0, m0 = mi_ref.recovery_pair(24)
    assert torch.allclose(f, f0, rtol=0, atol=1e-6) and torch.allclose(m, m0, rtol=0, atol=1e-6)
