"""CPU: the fp64 restatement of Gaussian smoothing (tests/gauss_ref.py) against scipy.ndimage.gaussian_filter(mode="nearest"), its
transpose against the forward by adjointness, the host-side weights of ops.gaussian_kernel1d, the argument checks of the
smoothed pyramid (io/_pyramid.py), and the noise-recovery experiment that the GPU test's thresholds rest on.
Shapes: for a sigma with radius R, axes of length 1, 2, R, R + 1 and 2 R + 1 (shorter than, equal to and longer than the
kernel's reach on either side).  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from tests import gauss_ref as G
from tests import mi_ref

# (shape, sigma (z, y, x)): R = 2 for 0.6 (int(2.9)), 8 for 2.0, 6 for 1.5, 32 for 8.0
CASES = [((1, 1, 1), 0.6), ((1, 1, 2), 0.6), ((2, 3, 5), 0.6), ((1, 2, 8), 2.0), ((2, 8, 9), 2.0), ((9, 17, 2), 2.0),
         ((3, 4, 5), (0.0, 1.5, 0.0)), ((6, 7, 13), (2.0, 0.0, 0.6)), ((17, 1, 3), (2.0, 0.0, 0.6)), ((5, 9, 40), 8.0),
         ((2, 2, 65), (0.0, 0.0, 8.0)), ((3, 3, 3), 0.1), ((4, 5, 6), (1.0, 2.5, 0.3))]


def _x(shape, seed=0):
    return np.random.default_rng(seed + sum(shape)).standard_normal((2,) + tuple(shape))


@pytest.mark.parametrize("shape,sigma", CASES, ids=str)
def test_smooth_matches_scipy(shape, sigma):
    x = _x(shape)
    got = G.smooth(x, sigma)
    want = np.stack([ndi.gaussian_filter(v, sigma, mode="nearest", truncate=4.0) for v in x])
    err = float(np.abs(got - want).max())
    print(f"{shape} sigma {sigma}: |restatement - scipy| {err:.3e}")
    assert got.dtype == np.float64 and err <= 1e-13


@pytest.mark.parametrize("shape,sigma", CASES, ids=str)
def test_smooth_bwd_is_the_transpose(shape, sigma):
    x, g = _x(shape, 1), _x(shape, 2)
    lhs = float((G.smooth(x, sigma) * g).sum())
    rhs = float((x * G.smooth_bwd(g, sigma)).sum())
    scale = float(np.abs(G.smooth(x, sigma) * g).sum())
    print(f"{shape} sigma {sigma}: <Ax, g> {lhs:.15e}, <x, A^T g> {rhs:.15e}, relative {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 1e-12 * scale


def test_zero_radius_is_untouched():
    x = _x((3, 4, 5))
    assert G.radius(0.1) == 0 and G.radius(0.0) == 0
    assert np.array_equal(G.smooth(x, 0.1), x) and np.array_equal(G.smooth_bwd(x, (0.0, 0.1, 0.0)), x)


@pytest.mark.parametrize("sigma", [0.0, 0.1, 0.6, 1.0, 1.5, 2.0, 4.0, 8.0])
def test_kernel1d_is_the_restatement_rounded_once(sigma):
    from keymorph_amd import ops
    w = ops.gaussian_kernel1d(sigma)
    ref = G.kernel1d(sigma)
    total = float(w.double().sum())
    print(f"sigma {sigma}: R {G.radius(sigma)}, {len(w)} taps, |sum - 1| {abs(total - 1.0):.3e}")
    assert w.dtype == torch.float32 and not w.is_cuda and len(w) == 2 * G.radius(sigma) + 1 == len(ref)
    assert ops.gaussian_radius(sigma) == G.radius(sigma)
    assert np.array_equal(w.numpy(), ref.astype(np.float32))
    assert abs(total - 1.0) <= 2.0 ** -23      # each weight moves by at most 2^-24 of itself, and they sum to 1
    assert torch.equal(w, w.flip(0))


def test_kernel1d_sigma_2():
    from keymorph_amd import ops
    w = ops.gaussian_kernel1d(2.0)
    total = float(w.double().sum())
    print(f"sigma 2: {len(w)} taps, sum - 1 = {total - 1.0:.3e}")
    assert len(w) == 17 and abs(total - 1.0) <= 2.0 ** -23


def test_kernel1d_refusals():
    from keymorph_amd import ops
    for bad in (-1.0, float("nan"), float("inf"), 8.1, (1.0, 1.0, 1.0), True):
        with pytest.raises(ValueError):
            ops.gaussian_kernel1d(bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ops.gaussian_kernel1d(1.0, truncate=bad)
    assert ops.GAUSS_MAX_RADIUS == 32 and len(ops.gaussian_kernel1d(8.0)) == 65


def test_pyramid_smoothing_arguments():
    from keymorph_amd.io import _pyramid as P
    assert P.resolve_smoothing("who", (4, 2, 1), None) is None
    assert P.resolve_smoothing("who", (4, 2, 1), "auto") == (2.0, 1.0, 0.0)
    assert P.resolve_smoothing("who", (8, 1), "auto") == (4.0, 0.0)
    assert P.resolve_smoothing("who", (4, 2), (2, (0.0, 1.5, 1))) == (2.0, (0.0, 1.5, 1.0))
    # a dropped level drops its entry: 32 // 4 = 8 < MIN_AXIS
    assert P.level_dims((32, 32, 32), (4, 2, 1)) == [(16, 16, 16), (32, 32, 32)]
    assert P.level_smoothing("who", (32, 32, 32), (4, 2, 1), (2.0, 1.0, 0.5)) == [1.0, 0.5]
    assert P.level_smoothing("who", (32, 32, 32), (4, 2, 1), "auto") == [1.0, 0.0]
    assert P.level_smoothing("who", (32, 32, 32), (4, 2, 1), None) is None
    f = torch.zeros(1, 1, 32, 32, 32)
    for bad in ((1.0,), (1.0, 1.0, 1.0, 1.0), (2.0, -1.0, 0.0), (2.0, float("nan"), 0.0), (2.0, (1.0, 1.0), 0.0), "gauss", 1.0,
                (2.0, "a", 0.0)):
        with pytest.raises(ValueError, match="some_driver"):
            list(P.levels(f, f, (4, 2, 1), bad, "some_driver"))
    with pytest.raises(ValueError, match="2 entries for the 3 levels"):
        P.resolve_smoothing("who", (4, 2, 1), (1.0, 0.0))


def test_drivers_name_themselves_on_a_wrong_length():
    """the check comes before any GPU work: CPU tensors reach it"""
    from keymorph_amd.io import estimate_translation
    f = torch.zeros(1, 1, 32, 32, 32)
    with pytest.raises(ValueError, match="estimate_translation"):
        estimate_translation(f, f, shrink=(2, 1), smoothing_sigmas=(1.0,))


def test_noise_recovery_restatement():
    """The experiment behind the smoothed pyramid: recovery_pair(64) (true shift (2.3, -1.6, 0.8)) plus 0.3 randn voxel noise
    (seed 100), shrink (4, 2), 30 iterations, lr 0.25, in fp64.  Unsmoothed the estimate ends 3.743 voxels from the truth (worse
    than the 2.914 of doing nothing); with sigma (2, 1) before the resize it ends 0.593 away.  The GPU test's thresholds (1.0
    and 2.0) separate these two values, so they are pinned here to +- 0.01."""
    f, m = G.noisy_pair()
    true = torch.tensor([mi_ref.RECOVERY_SHIFT], dtype=torch.float64)
    out = {}
    for name, sm in (("as today", None), ("smoothed", G.NOISE_SIGMAS)):
        t, trace = G.estimate(f, m, shrink=G.NOISE_SHRINK, iters=30, lr=0.25, smoothing=sm)
        out[name] = [float((v - true).norm()) for v in trace]
        assert float((t - torch.tensor([G.NOISE_ANSWERS[name]], dtype=torch.float64)).abs().max()) <= 1e-3, (name, t)
        print(f"{name}: Euclidean error after level 4 / level 2: {out[name][0]:.3f} / {out[name][1]:.3f}, largest per-axis error "
              f"{float((t - true).abs().max()):.3f}; |shift| {float(true.norm()):.3f}")
    assert abs(out["as today"][1] - 3.743) <= 0.01
    assert abs(out["smoothed"][1] - 0.593) <= 0.01
