"""CPU: the fp64 restatement of cubic B-spline resampling (tests/cubic_ref.py) against scipy's independent implementation, its
analytic grid gradient against central differences, and the clamp rule."""
import numpy as np
import pytest
from scipy import ndimage as ndi

from tests import cubic_ref as R

SHAPES = [(5, 6, 7), (2, 3, 9), (1, 4, 5), (3, 3, 3)]


def _volume(shape, seed):
    return np.random.default_rng(seed).random(shape)


def _grid_of(coords, shape):
    """voxel coordinates (P, 3) in (z, y, x) order -> the normalised grid (1, 1, 1, P, 3), xyz, float32, and the fp32 source
    coordinates the sampler derives from it (P, 3) in (z, y, x) order"""
    from tests.sampler_ref import source_coord
    g = np.stack([(2.0 * coords[:, 2 - k] + 1.0) / shape[2 - k] - 1.0 for k in range(3)], -1).astype(np.float32)
    back = np.stack([source_coord(g[:, 2 - k], shape[k])[0] for k in range(3)], -1)
    return g.reshape(1, 1, 1, -1, 3), back


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_coefficients_match_scipy(shape):
    x = _volume(shape, 1)
    ref = x.copy()
    for axis in range(3):
        if shape[axis] > 1:                                      # (an axis of length 1 is left as it is)
            ref = ndi.spline_filter1d(ref, order=3, axis=axis, mode="mirror")
    err = np.abs(R.coefficients(x) - ref).max()
    print(f"coefficients {shape}: {err:.3e}")
    assert err <= 1e-12
    if min(shape) > 1:
        assert np.abs(ref - ndi.spline_filter(x, order=3, mode="mirror")).max() <= 1e-12


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_values_match_scipy(shape):
    x = _volume(shape, 2)
    rng = np.random.default_rng(3)
    coords = rng.random((200, 3)) * (np.array(shape) - 1.0)
    g, back = _grid_of(coords, shape)
    got = R.resample(x[None, None], g)[0, 0, 0, 0]
    # scipy at the coordinates the sampler actually uses (the grid is fp32); depth-1 axes need at least 2 samples in scipy's
    # mirror mode, so such an axis is sampled as a constant one
    xs, cs = x, back
    for axis in range(3):
        if shape[axis] == 1:
            xs = np.repeat(xs, 2, axis=axis)
    ref = ndi.map_coordinates(xs, cs.T, order=3, mode="mirror")
    err = np.abs(got - ref).max()
    print(f"values {shape}: {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_interpolates_the_lattice(shape):
    """at every lattice point whose fp32 grid coordinate maps back to the integer exactly (the others sit 1e-7 voxels off it)"""
    x = _volume(shape, 4)
    coords = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    g, back = _grid_of(coords, shape)
    exact = (back == coords).all(-1)
    assert exact.sum() * 2 >= len(coords)
    got = R.resample(x[None, None], g)[0, 0, 0, 0]
    err = np.abs(got - x.reshape(-1))[exact].max()
    print(f"lattice {shape}: {err:.3e} at {int(exact.sum())} of {len(coords)} points")
    assert err <= 1e-12


def test_float32_restatement_runs_in_float32():
    x = _volume((5, 6, 7), 5).astype(np.float32)[None, None]
    g = (np.random.default_rng(6).random((1, 2, 3, 5, 3)) * 2.2 - 1.1).astype(np.float32)
    ref, bound = R.tolerance(R.resample, x, g)
    assert ref.dtype == np.float64 and 0.0 < bound < 1e-5


def test_grid_gradient_matches_central_differences():
    shape = (6, 7, 8)
    x = _volume((2, 2) + shape, 7)
    rng = np.random.default_rng(8)
    # interior points (no axis clamped at g +- h); the interpolant is C2, so a difference across a lattice plane is as good
    g = (rng.random((2, 3, 4, 5, 3)) * 1.5 - 0.75).astype(np.float32)
    gout = rng.standard_normal((2, 2, 3, 4, 5))
    coef = R.coefficients(x)
    ana = R.sample_bwd_grid(coef, g, gout)
    h = np.float32(2.0 ** -8)                                     # exactly representable steps of fp32 coordinates
    for k in range(3):
        gp, gm = g.copy(), g.copy()
        gp[..., k] += h
        gm[..., k] -= h
        step = (gp[..., k].astype(np.float64) - gm[..., k].astype(np.float64))
        num = ((R.sample(coef, gp) - R.sample(coef, gm)) * gout).sum(1) / step
        # central differences of a C2 piecewise cubic: error <= h^2 / 6 * max|f'''| ~ h^2 * (size / 2)^3 * |c| * |gout|
        scale = (shape[2 - k] / 2.0) ** 3 * np.abs(coef).max() * np.abs(gout).sum(1).max()
        err = np.abs(num - ana[..., k]).max()
        print(f"axis {k}: {err:.3e} (bar {float(h) ** 2 * scale:.3e})")
        assert err <= float(h) ** 2 * scale


def test_clamped_axes_pass_exactly_zero():
    x = _volume((1, 2, 4, 5, 6), 9)
    rng = np.random.default_rng(10)
    g = (rng.random((1, 3, 4, 5, 3)) * 1.2 - 0.6).astype(np.float32)
    g[0, 0, ..., 0] = 1.5                       # x clamped high
    g[0, 1, ..., 1] = -1.0                      # y clamped low (exactly -1 is outside the first voxel centre)
    g[0, 2, ..., 2] = np.inf                    # z clamped
    g[0, 2, 0, 0, 0] = np.nan                   # a NaN coordinate: no gradient on any axis
    gout = rng.standard_normal((1, 2, 3, 4, 5))
    d = R.resample_bwd_grid(x, g, gout)
    assert (d[0, 0, ..., 0] == 0).all() and (d[0, 1, ..., 1] == 0).all() and (d[0, 2, ..., 2] == 0).all()
    assert (d[0, 2, 0, 0] == 0).all()
    assert (d[0, 0, ..., 1] != 0).all() and (d[0, 1, ..., 0] != 0).all()
    out = R.resample(x, g)
    assert np.isfinite(out).all()
    # clamped high in x: the value at the last voxel centre, which the spline interpolates
    far = R.resample(x, np.concatenate([np.full_like(g[:, :1, ..., :1], 1.0 - 1.0 / 6), g[:, :1, ..., 1:]], -1))
    assert np.abs(out[:, :, :1] - far).max() <= 1e-12
