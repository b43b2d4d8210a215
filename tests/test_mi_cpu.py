"""CPU: properties of the fp64 restatement of the mutual information (tests/mi_ref.py), the yardstick of tests/test_mi_gpu.py,
and the validation of the translation-recovery inputs on the restatement alone."""
import math

import pytest
import torch

from tests import mi_ref

F64 = torch.float64


@pytest.fixture(scope="module")
def pair():
    a, b = mi_ref.smooth_pair((1, 1, 12, 10, 14), seed=3)
    return a.to(F64), b.to(F64)


def test_self_information_is_the_entropy_of_the_marginal(pair):
    a, _ = pair
    bins = 16
    # computed separately: the 1-D Parzen histogram of a, and the joint table of (a, a) reduced by hand
    lo, hi = a.min(), a.max()
    w = mi_ref.window_matrix(a.reshape(-1), lo, hi, bins)
    p = w.t() @ w / a.numel()
    pa = w.sum(0) / a.numel()
    assert torch.allclose(p.sum(1), pa, rtol=0, atol=1e-15)
    pos = p > 0
    expect = (p[pos] * torch.log(p[pos])).sum() - 2 * (pa[pa > 0] * torch.log(pa[pa > 0])).sum()
    got = mi_ref.mutual_information(a, a, bins)[0]
    assert abs(float(got - expect)) < 1e-12
    # 2 H(marginal) - H(joint) <= H(marginal), with equality only for windows that do not overlap
    ent = -(pa[pa > 0] * torch.log(pa[pa > 0])).sum()
    assert 0.0 < float(got) <= float(ent)


def test_invariant_under_positive_affine_intensity_maps(pair):
    a, b = pair
    base = mi_ref.mutual_information(a, b, 32)[0]
    # powers of two and a shift that keeps every operation exact up to fp64 round-off of (x - lo) s
    for alpha, beta in ((4.0, 0.0), (0.5, 3.0), (3.7, -11.25)):
        got = mi_ref.mutual_information(alpha * a + beta, b, 32)[0]
        assert abs(float(got - base)) < 1e-11, (alpha, beta, float(got - base))


def test_symmetric_in_its_inputs(pair):
    a, b = pair
    for bins in (8, 32, 64):
        ab, ba = mi_ref.mutual_information(a, b, bins)[0], mi_ref.mutual_information(b, a, bins)[0]
        assert abs(float(ab - ba)) < 1e-13
        assert float(ab) > 0.05


def test_constant_input_gives_zero(pair):
    a, _ = pair
    c = torch.full_like(a, 0.37)
    a = a.clone().requires_grad_(True)
    mi = mi_ref.mutual_information(a, c, 32)[0]
    assert abs(float(mi)) < 1e-13
    (g,) = torch.autograd.grad(mi, a)
    assert float(g.abs().max()) < 1e-13
    assert abs(float(mi_ref.mutual_information(c, c, 32)[0])) < 1e-13


@pytest.mark.parametrize("bins", [8, 32, 64])
def test_end_taps_stay_inside_the_table_and_sum_to_one(bins):
    x = torch.tensor([0.0, 1.0, 0.5, 1.0 - 1e-16, 1e-300], dtype=F64)
    k0, w = mi_ref.taps(x, x.min(), x.max(), bins)
    assert int(k0.min()) >= 0 and int(k0.max()) + 3 <= bins - 1
    assert torch.allclose(w.sum(1), torch.ones(5, dtype=F64), rtol=0, atol=1e-15)
    assert int(k0[0]) == 0 and torch.allclose(w[0], torch.tensor([1 / 6, 4 / 6, 1 / 6, 0], dtype=F64), atol=1e-15)      # u = 1
    assert int(k0[1]) == bins - 4 and torch.allclose(w[1], torch.tensor([0, 1 / 6, 4 / 6, 1 / 6], dtype=F64), atol=1e-15)  # u = B-2
    assert float(w.min()) >= 0.0


def test_gradient_matches_the_closed_form(pair):
    """dMI/da_v = (s_a / V) sum_ij G_ij b3'(u_a - i) b3(u_b - j): what the kernel evaluates, against autograd."""
    a, b = pair
    bins = 16
    a = a.clone().requires_grad_(True)
    mi = mi_ref.mutual_information(a, b, bins)[0]
    (g,) = torch.autograd.grad(mi, a)
    with torch.no_grad():
        G = mi_ref.log_ratio(mi_ref.joint(a, b, bins))
        av, bv = a.reshape(-1), b.reshape(-1)
        s = (bins - 3) / (av.max() - av.min())
        wb = mi_ref.window_matrix(bv, bv.min(), bv.max(), bins)
        u = (av - av.min()) * s + 1
        k0 = (torch.floor(u).long() - 1).clamp(0, bins - 4)
        t = u - (k0 + 1)
        d = torch.stack([-0.5 * (1 - t) ** 2, 1.5 * t * t - 2 * t, -1.5 * t * t + t + 0.5, 0.5 * t * t], dim=1)
        da = torch.zeros(av.numel(), bins, dtype=F64).scatter(1, k0[:, None] + torch.arange(4)[None, :], d)
        closed = s / av.numel() * ((da @ G) * wb).sum(1)
    assert float((closed - g.reshape(-1)).norm() / g.norm()) < 1e-12


@pytest.mark.parametrize("shift, seed", [(mi_ref.RECOVERY_SHIFT, 5), ((-1.4, 2.2, 1.7), 9)])
def test_translation_recovery_inputs(shift, seed):
    """The inputs of the GPU recovery tests, validated on the restatement alone: 24^3, one level, 60 Adam steps of 0.25 voxel
    from zero.  The bound is the condition 'sub-voxel', not a measurement."""
    fixed, moving = mi_ref.recovery_pair(24, shift, seed)
    t = mi_ref.estimate(fixed.to(F64), moving.to(F64), bins=32, shrink=(1,), iters=60, lr=0.25, init=torch.zeros(1, 3))
    err = (t[0] - torch.tensor(shift, dtype=F64)).abs()
    print("recovered", t[0].tolist(), "error", err.tolist())
    assert float(err.max()) <= 0.5


def test_reference_translate_shifts_by_whole_voxels():
    x = torch.rand(1, 1, 6, 7, 8, dtype=F64, generator=torch.Generator().manual_seed(0))
    out = mi_ref.translate(x, torch.tensor([[1.0, -2.0, 3.0]], dtype=F64))
    assert torch.allclose(out[0, 0, :5, 2:, :5], x[0, 0, 1:, :5, 3:], rtol=0, atol=1e-14)
    assert math.isclose(float(mi_ref.centroid(torch.ones(1, 1, 5, 7, 9, dtype=F64))[0, 2]), 4.0, abs_tol=1e-9)
