"""GPU: Gaussian smoothing (csrc/gauss.hip; ops.gaussian_smooth, fields.smooth, the smoothed pyramid of io/_pyramid.py and the
smoothing_sigmas argument of every intensity driver) against the fp64 restatement of tests/gauss_ref.py.

Tolerances are measured, not chosen: for each comparison the bound is 4 times the largest distance of the restatement evaluated in
float32 from itself in float64 on the same inputs (gauss_ref.tolerance): one volume and one sigma.  One stated exception
(references()), as in tests/test_cubic_gpu.py: where a set's own bound is 0 although its reference is not -- the float32
restatement happens to reproduce the float64 one, which measures nothing and which no other association of the same sums could
be asked to meet -- the bound is the largest one among that volume's sets.  "0" here includes the float64 sum's own rounding: on
the one-voxel volume the float32 restatement returns the voxel exactly and the float64 one returns it times (1 +- 2e-16), a
distance that is float64's, not float32's; anything under 2^-40 of the reference's magnitude is read as that (a float32 distance
is 2^-25 of it or more).  Every test prints its figures before it asserts.
Shapes: axes of length 1 and 2 (shorter than any kernel), odd sizes, W = 67, 130 and 300 in planes of 8040, 17160 and 1800 voxels
(the x pass has no second arm for long rows: it works on 1024-voxel tiles of the flat plane, and with these W a row straddles every
tile edge; the last tile is ragged), H = 40 and D = 33 (three 16-output segments of the y / z walk, the last
one of 8 outputs and of 1), D = H = 25 (one past the walk's ring of 2 R + 8 = 24 rows at sigma 2), and (1, 1, 5, 9, 40) at
sigma 8 (R = 32: every axis but W shorter than R, so both ends fold at once)."""
import functools

import numpy as np
import pytest
import torch

from tests import gauss_ref as G
from tests import mi_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32

VOLUMES = [(1, 1, 1, 1, 1), (1, 1, 1, 1, 2), (1, 2, 2, 3, 4), (2, 3, 5, 6, 7), (1, 1, 3, 40, 67), (1, 1, 33, 4, 130),
           (1, 1, 2, 3, 300), (1, 2, 25, 25, 9)]
SIGMAS = [0.6, 2.0, (0.0, 1.5, 0.0), (2.0, 0.0, 0.6)]
WIDE = ((1, 1, 5, 9, 40), 8.0)
CASES = [(v, s) for v in VOLUMES for s in SIGMAS] + [WIDE]


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def volume(shape, seed=1):
    return np.random.default_rng(sum(shape) * 7 + seed).standard_normal(shape).astype(F32)


@functools.lru_cache(maxsize=None)
def references(shape):
    """{sigma: (value, value bound, gradient, gradient bound)} of one volume and its cotangent, fp64: each set's own bound, except
    that a bound of 0 (to float64's own rounding: under 2^-40 max|reference|) under a reference that is not 0 everywhere is replaced
    by the largest bound among the volume's sets"""
    x, g = volume(shape), volume(shape, 2)
    refs = {}
    for sigma in SIGMAS + ([WIDE[1]] if shape == WIDE[0] else []):
        refs[sigma] = G.tolerance(G.smooth, x, sigma) + G.tolerance(G.smooth_bwd, g, sigma)
    pooled = [max(r[j] for r in refs.values()) for j in (1, 3)]
    for sigma, (ref, b, dref, db) in refs.items():
        if b <= 2.0 ** -40 * float(np.abs(ref).max()) and np.any(ref):
            b = pooled[0]
        if db <= 2.0 ** -40 * float(np.abs(dref).max()) and np.any(dref):
            db = pooled[1]
        refs[sigma] = (ref, b, dref, db)
    return refs


@functools.lru_cache(maxsize=None)
def gpu(shape, sigma):
    """(out, dx) of ops.gaussian_smooth on volume(shape) with the cotangent volume(shape, 2), as numpy"""
    from keymorph_amd import ops
    x = torch.from_numpy(volume(shape)).to(DEV).requires_grad_(True)
    out = ops.gaussian_smooth(x, sigma)
    (out * torch.from_numpy(volume(shape, 2)).to(DEV)).sum().backward()
    return _np(out), _np(x.grad)


@pytest.mark.parametrize("shape,sigma", CASES, ids=str)
def test_value_and_gradient_vs_fp64(shape, sigma):
    ref, bound, dref, dbound = references(shape)[sigma]
    out, dx = gpu(shape, sigma)
    err, derr = float(np.abs(out - ref).max()), float(np.abs(dx - dref).max())
    print(f"{shape} sigma {sigma}: value error {err:.3e} (bound {bound:.3e}, ratio {err / bound if bound else 0:.2f}), gradient error "
          f"{derr:.3e} (bound {dbound:.3e}, ratio {derr / dbound if dbound else 0:.2f})")
    assert out.dtype == F32 and out.shape == shape and dx.shape == shape
    assert np.isfinite(out).all() and np.isfinite(dx).all()
    assert err <= bound
    assert derr <= dbound


@pytest.mark.parametrize("shape,sigma", CASES, ids=str)
def test_adjointness_on_the_device(shape, sigma):
    """sum(out g) against sum(x dx), both accumulated in fp64 on the host.  The restatement's pair is adjoint to 1e-12, so the
    two sums differ by at most sum |out - ref| |g| + sum |x| |dx - dref| <= bound sum |g| + gradient bound sum |x|."""
    x, g = volume(shape).astype(np.float64), volume(shape, 2).astype(np.float64)
    ref, bound, dref, dbound = references(shape)[sigma]
    out, dx = gpu(shape, sigma)
    lhs, rhs = float((out.astype(np.float64) * g).sum()), float((x * dx.astype(np.float64)).sum())
    allowed = bound * float(np.abs(g).sum()) + dbound * float(np.abs(x).sum()) + 1e-12 * float(np.abs(ref * g).sum())
    print(f"{shape} sigma {sigma}: <A x, g> {lhs:.9e}, <x, A^T g> {rhs:.9e}, difference {abs(lhs - rhs):.3e}, allowed {allowed:.3e}")
    assert abs(lhs - rhs) <= allowed


def test_zero_radius_is_the_input_itself():
    from keymorph_amd import ops
    x = torch.from_numpy(volume((2, 3, 5, 6, 7))).to(DEV)
    for sigma in (0.0, 0.1, (0.0, 0.1, 0.12)):                     # R = int(4 sigma + 0.5) = 0
        assert ops.gaussian_smooth(x, sigma) is x
    xr = x.clone().requires_grad_(True)
    out = ops.gaussian_smooth(xr, (0.1, 0.6, 0.0))                 # only H is smoothed
    out.sum().backward()
    assert torch.equal(out, ops.gaussian_smooth(x, (0.0, 0.6, 0.0)))
    # every ROW of the operator sums to 1, so its columns sum to the number of voxels in all (a replicated border moves weight
    # between columns, it loses none): 2 R + 1 = 5 roundings of at most 2^-24 each and the weights' own sum within 2^-24 of 1
    total = float(xr.grad.double().sum())
    print(f"gradient of the sum: sum(dx) {total:.6f} for {x.numel()} voxels, largest column {float(xr.grad.max()):.4f}")
    assert abs(total - x.numel()) <= x.numel() * 4 * 2.0 ** -23
    assert float(xr.grad.max()) > 1.001 and float(xr.grad.min()) < 0.999      # the border columns, not all ones


def test_refusals():
    from keymorph_amd import _lib, ops
    x = torch.zeros(1, 1, 5, 9, 40, device=DEV)
    assert ops.gaussian_smooth(x, 8.0).shape == x.shape           # R = 32, the largest
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    for sigma in (8.1, (0.0, 8.1, 0.0), -1.0, (1.0, -0.5, 1.0), float("nan"), float("inf"), (1.0, 1.0), "a", None, True):
        with pytest.raises(ValueError):
            ops.gaussian_smooth(x, sigma)
    for bad in (x[0], x[:, :, :, :, :0]):
        with pytest.raises(ValueError):
            ops.gaussian_smooth(bad, 1.0)
    with pytest.raises(ValueError):
        ops.gaussian_smooth(x.double(), 1.0)
    with pytest.raises(ValueError):
        ops.gaussian_smooth(x, 1.0, truncate=0.0)
    with pytest.raises(_lib.KeymorphHipError):
        ops.gaussian_smooth(x.cpu(), 1.0)
    # views of one element: nothing that large exists before or after the refusal
    huge = torch.zeros(1, device=DEV).expand(1, 1, 1 << 9, 1 << 10, 1 << 10)          # a channel plane of 2^29 voxels
    many = torch.zeros(1, device=DEV).expand(256, 256, 1, 1, 2)                        # N C = 65536
    for bad in (huge, many):
        with pytest.raises(ValueError):
            ops.gaussian_smooth(bad, 1.0)
    assert torch.cuda.max_memory_allocated() < before + (1 << 28)
    assert (ops.GAUSS_MAX_RADIUS, ops.GAUSS_MAX_PLANE, ops.GAUSS_MAX_PLANES) == (32, 1 << 29, 65535)
    # the C ABI refuses the same
    lib = _lib.load()
    out = torch.empty_like(x)
    w = ops._gauss_host(1.0, 4.0)[1]
    import ctypes
    p, o, wp = x.data_ptr(), out.data_ptr(), ctypes.addressof(w)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.kmh_gauss_fwd(p, o, None, 1, 1, 5, 9, 40, 0, 0, 33, None, None, wp, s) == -22      # R > 32
    assert lib.kmh_gauss_fwd(p, p, None, 1, 1, 5, 9, 40, 0, 0, 4, None, None, wp, s) == -22       # out aliases x
    assert lib.kmh_gauss_fwd(p, o, None, 1, 1, 5, 9, 40, 0, 0, 4, None, None, None, s) == -22     # no weights
    assert lib.kmh_gauss_fwd(p, o, None, 1, 1, 5, 9, 40, 0, 4, 4, None, wp, wp, s) == -22         # two axes, no workspace
    assert lib.kmh_gauss_fwd(p, o, None, 1, 1, 0, 9, 40, 0, 0, 4, None, None, wp, s) == -22       # empty
    assert lib.kmh_gauss_fwd(p, o, None, 256, 256, 1, 1, 2, 0, 0, 4, None, None, wp, s) == -22    # N C past the grid
    assert lib.kmh_gauss_bwd(p, o, None, 1, 1, 5, 9, 40, 0, 0, 4, None, None, wp, None, None, None, s) == -22      # no tails
    assert lib.kmh_gauss_ws_bytes(1, 1, 5, 9, 40, 0, 0, 4) == 0 and lib.kmh_gauss_ws_bytes(1, 1, 5, 9, 40, 0, 4, 4) == 4 * 1800


def test_exactness():
    """two runs, a batch against its samples, a channel against itself alone: bit for bit"""
    from keymorph_amd import ops
    rng = np.random.default_rng(21)
    x = torch.from_numpy(rng.standard_normal((2, 3, 19, 21, 70)).astype(F32)).to(DEV)
    g = torch.from_numpy(rng.standard_normal((2, 3, 19, 21, 70)).astype(F32)).to(DEV)

    def run(xs, gs, sigma):
        xs = xs.clone().requires_grad_(True)
        out = ops.gaussian_smooth(xs, sigma)
        (out * gs).sum().backward()
        return out.detach(), xs.grad

    for sigma in (1.0, (2.0, 0.0, 0.6)):
        out, dx = run(x, g, sigma)
        out2, dx2 = run(x, g, sigma)
        assert torch.equal(out, out2) and torch.equal(dx, dx2)
        for n in range(2):
            o1, d1 = run(x[n:n + 1].contiguous(), g[n:n + 1].contiguous(), sigma)
            assert torch.equal(out[n:n + 1], o1) and torch.equal(dx[n:n + 1], d1), n
        for c in range(3):
            o1, d1 = run(x[:, c:c + 1].contiguous(), g[:, c:c + 1].contiguous(), sigma)
            assert torch.equal(out[:, c:c + 1], o1) and torch.equal(dx[:, c:c + 1], d1), c


def test_one_axis_leaves_no_trace_of_the_others():
    """gaussian_smooth(x, (0, 1.5, 0)) equals the same call on every [z, :, x] line, forward and backward"""
    from keymorph_amd import ops
    shape = (2, 3, 5, 6, 7)
    x = torch.from_numpy(volume(shape)).to(DEV).requires_grad_(True)
    g = torch.from_numpy(volume(shape, 2)).to(DEV)
    out = ops.gaussian_smooth(x, (0.0, 1.5, 0.0))
    (out * g).sum().backward()
    for z in range(shape[2]):
        for i in range(shape[4]):
            line = x.detach()[:, :, z:z + 1, :, i:i + 1].contiguous().requires_grad_(True)
            o = ops.gaussian_smooth(line, (0.0, 1.5, 0.0))
            (o * g[:, :, z:z + 1, :, i:i + 1]).sum().backward()
            assert torch.equal(o, out[:, :, z:z + 1, :, i:i + 1]), (z, i)
            assert torch.equal(line.grad, x.grad[:, :, z:z + 1, :, i:i + 1]), (z, i)


# ---- fields.smooth ---------------------------------------------------------------------------------------------------------
def test_fields_smooth_keeps_the_identity():
    from keymorph_amd import fields
    ids = fields.identity_grid((2, 1, 9, 17, 33), DEV)
    for sigma in (1.0, (2.0, 0.0, 0.6)):
        assert torch.equal(fields.smooth(ids, sigma), ids)


def test_fields_smooth_keeps_a_constant_displacement():
    """A grid that is the identity plus one offset per component has a constant displacement d (up to the rounding of the grid
    itself), and smoothing leaves a constant alone.  Bound per component k of size S: [the smoothing bound on the displacement the
    kernel was given + the distance of its fp64 smoothing from it] * 2 / S (displacement to grid units) + 4 * 2^-24 max|grid| for
    the four roundings of to_displacement and from_displacement (a subtraction and a product each way)."""
    from keymorph_amd import fields
    dims = (9, 17, 33)
    ids = fields.identity_grid((2, 1) + dims, DEV)
    grid = ids + torch.tensor([0.11, -0.07, 0.05], device=DEV)
    sigma = (1.0, 2.0, 0.6)
    got = fields.smooth(grid, sigma)
    d = _np(fields.to_displacement(grid))
    ref, bound = G.tolerance(G.smooth, d, sigma)
    drift = np.abs(ref - d).reshape(2, 3, -1).max(2).max(0)                      # per channel (z, y, x)
    assert got.shape == grid.shape
    for k, size in enumerate(reversed(dims)):                                    # grid component k = x, y, z
        err = float((got[..., k] - grid[..., k]).abs().max())
        allowed = (bound + float(drift[2 - k])) * 2.0 / size + 4 * 2.0 ** -24 * float(grid.abs().max())
        print(f"component {k}: |smooth(grid) - grid| {err:.3e}, allowed {allowed:.3e}")
        assert err <= allowed


def test_fields_smooth_is_differentiable():
    """the gradient is the smoothing's transpose on every component: against ops.gaussian_smooth's own backward"""
    from keymorph_amd import fields, ops
    dims = (5, 6, 7)
    rng = np.random.default_rng(3)
    grid = (fields.identity_grid((2, 1) + dims, DEV) + torch.from_numpy(rng.normal(0, 0.05, (2,) + dims + (3,)).astype(F32)).to(DEV))
    grid.requires_grad_(True)
    go = torch.from_numpy(rng.standard_normal((2,) + dims + (3,)).astype(F32)).to(DEV)
    (fields.smooth(grid, 1.0) * go).sum().backward()
    c = go.permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    (ops.gaussian_smooth(c, 1.0) * go.permute(0, 4, 1, 2, 3)).sum().backward()      # d/dc of <A c, go> = A^T go
    assert torch.equal(grid.grad, c.grad.permute(0, 2, 3, 4, 1))
    with pytest.raises(ValueError):
        fields.smooth(grid.detach(), -1.0)
    with pytest.raises(ValueError):
        fields.smooth(grid.detach()[..., :2], 1.0)


# ---- the pyramid and the drivers -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean():
    f, m = mi_ref.recovery_pair(32)
    return f.to(DEV), m.to(DEV)


@pytest.fixture(scope="module")
def noisy():
    f, m = G.noisy_pair()
    return f.float().to(DEV), m.float().to(DEV)


def test_levels_are_resize_of_smooth():
    from keymorph_amd import ops
    from keymorph_amd.io._pyramid import levels
    from keymorph_amd.utils import resize_trilinear
    f, m = (torch.from_numpy(volume((1, 1, 64, 64, 64), s)).to(DEV) for s in (1, 2))
    got = list(levels(f, m, (4, 2, 1), smoothing=(2, 1, 0)))
    assert [g[0] for g in got] == [(16, 16, 16), (32, 32, 32), (64, 64, 64)]
    for (ldims, f_l, m_l, ratio), sigma in zip(got[:2], (2, 1)):
        assert torch.equal(f_l, resize_trilinear(ops.gaussian_smooth(f, sigma), size=ldims))
        assert torch.equal(m_l, resize_trilinear(ops.gaussian_smooth(m, sigma), size=ldims))
        assert not torch.equal(f_l, resize_trilinear(f, size=ldims))
        assert ratio == [64 / ldims[0]] * 3
    assert got[2][1] is f and got[2][2] is m
    full = list(levels(f, m, (1,), smoothing=((0.0, 1.0, 0.0),)))
    assert torch.equal(full[0][1], ops.gaussian_smooth(f, (0.0, 1.0, 0.0)))
    plain = list(levels(f, m, (4, 2, 1)))
    auto = list(levels(f, m, (4, 2, 1), smoothing="auto"))
    assert all(torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) for a, b in zip(auto, got))
    assert plain[2][1] is f and not torch.equal(plain[0][1], got[0][1])


def test_zero_sigmas_are_the_unsmoothed_drivers(clean):
    from keymorph_amd.io import estimate_translation, register_bspline, register_intensity, register_svf
    f, m = clean
    z = (0, 0, 0)
    assert torch.equal(estimate_translation(f, m, smoothing_sigmas=z), estimate_translation(f, m))
    mat = register_intensity(f, m, "rigid")
    assert torch.equal(register_intensity(f, m, "rigid", smoothing_sigmas=z), mat)
    assert torch.equal(register_bspline(f, m, iters=5, smoothing_sigmas=z), register_bspline(f, m, iters=5))
    assert torch.equal(register_svf(f, m, mat, iters=5, smoothing_sigmas=z), register_svf(f, m, mat, iters=5))
    for driver in (estimate_translation, register_bspline, register_svf):
        with pytest.raises(ValueError, match=driver.__name__):
            driver(f, m, smoothing_sigmas=(1.0, 0.0))
    with pytest.raises(ValueError, match="register_intensity"):
        register_intensity(f, m, "rigid", smoothing_sigmas=(1.0, 0.0))


def test_smoothing_reaches_every_driver(clean):
    """with sigmas that are not 0 every driver's answer moves (the argument is not dropped on the way), and stays finite"""
    from keymorph_amd.io import register_bspline, register_intensity, register_svf
    f, m = clean
    mat = register_intensity(f, m, "rigid", iters=5)
    mats = register_intensity(f, m, "rigid", iters=5, smoothing_sigmas="auto")
    assert torch.isfinite(mats).all() and not torch.equal(mat, mats)
    for driver in (register_bspline, register_svf):
        a, b = driver(f, m, mat, iters=3), driver(f, m, mat, iters=3, smoothing_sigmas="auto")
        assert torch.isfinite(b).all() and not torch.equal(a, b), driver.__name__


def test_noise_recovery(noisy):
    """The experiment of tests/test_gauss_cpu.py::test_noise_recovery_restatement on the device: recovery_pair(64) plus 0.3 randn
    voxel noise (seed 100), shrink (4, 2), 30 iterations, lr 0.25.  The fp64 restatement ends 0.593 voxels (Euclidean) from the
    true shift with sigma (2, 1) and 3.743 without; the thresholds 1.0 and 2.0 separate the two."""
    from keymorph_amd.io import estimate_translation
    f, m = noisy
    true = torch.tensor([mi_ref.RECOVERY_SHIFT], dtype=torch.float64)
    dist = {}
    for name, sm in (("smoothed", G.NOISE_SIGMAS), ("as today", None)):
        t = estimate_translation(f, m, shrink=G.NOISE_SHRINK, iters=30, lr=0.25, smoothing_sigmas=sm).double().cpu()
        t_ref = torch.tensor([G.NOISE_ANSWERS[name]], dtype=torch.float64)      # recomputed by the CPU test
        dist[name] = float((t - true).norm())
        print(f"{name}: GPU {t.tolist()}, {dist[name]:.3f} voxels from the true shift (restatement {float((t_ref - true).norm()):.3f}); "
              f"|GPU - restatement| {float((t - t_ref).norm()):.3f}")
    assert dist["smoothed"] <= 1.0
    assert dist["as today"] > 2.0


def test_auto_smoothing_on_the_clean_pair(clean):
    from keymorph_amd.io import estimate_translation
    f, m = clean
    t = estimate_translation(f, m, smoothing_sigmas="auto").double().cpu()
    err = (t - torch.tensor([mi_ref.RECOVERY_SHIFT], dtype=torch.float64)).abs()
    print(f"clean 32^3 pair, 'auto': t {t.tolist()}, per-axis error {err.tolist()}")
    assert float(err.max()) <= 0.5


def test_smoothed_translation_does_not_wait_for_the_gpu(clean):
    from keymorph_amd.io import estimate_translation
    f, m = clean
    first = estimate_translation(f, m, shrink=(1,), smoothing_sigmas=(1.0,), iters=3)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = estimate_translation(f, m, shrink=(1,), smoothing_sigmas=(1.0,), iters=3)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(first, again) and torch.isfinite(first).all()


def test_model_takes_smoothing_sigmas(clean):
    from keymorph_amd.io import register_bspline, register_intensity
    from keymorph_amd.model import IntensityRegistration
    f, m = clean
    kw = dict(iters=5, bspline_iters=3)
    res = IntensityRegistration(smoothing_sigmas="auto", **kw)(f, m, ["rigid", "bspline"])
    assert set(res) == {"rigid", "bspline"}
    assert set(res["rigid"]) == {"grid", "matrix", "mi", "time"}
    assert set(res["bspline"]) == {"grid", "matrix", "ctrl", "mi", "time"}
    for entry in res.values():
        assert all(torch.isfinite(entry[k]).all() for k in entry if k != "time")
    # None is the driver's own default path
    plain = IntensityRegistration(smoothing_sigmas=None, **kw)(f, m, ["rigid", "bspline"])
    assert torch.equal(plain["rigid"]["matrix"], register_intensity(f, m, "rigid", iters=5))
    affine = register_intensity(f, m, "affine", iters=5)
    assert torch.equal(plain["bspline"]["matrix"], affine)
    assert torch.equal(plain["bspline"]["ctrl"], register_bspline(f, m, affine, iters=3, lr=0.1))
    assert not torch.equal(plain["rigid"]["matrix"], res["rigid"]["matrix"])
    same = IntensityRegistration(smoothing_sigmas=(2, 1, 0), **kw)(f, m, "rigid")      # 'auto' spelled out
    assert torch.equal(same["rigid"]["matrix"], res["rigid"]["matrix"])
    with pytest.raises(ValueError, match="IntensityRegistration"):
        IntensityRegistration(smoothing_sigmas=(1.0, 0.0))(f, m, "rigid")
    with pytest.raises(ValueError, match="IntensityRegistration"):
        IntensityRegistration(smoothing_sigmas=(2, 1, 0))(f, m, "rigid", num_resolutions_for_itkelastix=2)
