"""GPU: cubic B-spline resampling (csrc/cubic.hip; ops.cubic_coefficients, ops.cubic_sample, grid_sample3d(..., "cubic") and
everything that hands a mode to align_img) against the fp64 restatement of tests/cubic_ref.py.

Tolerances are measured, not chosen: for each comparison the bound is 4 times the largest distance of the restatement evaluated in
float32 from itself in float64 on the same inputs (cubic_ref.tolerance): one volume and one coordinate set.  One stated exception
(references()): where a set's own bound is 0 although its reference is not -- on the two-voxel volume the float32 restatement of
the identity, lattice and border sets reproduces the float64 one bit for bit, which measures nothing and which no other
association of the same sums could be asked to meet -- the bound is the largest one among that volume's sets.  A reference that
is 0 everywhere (every axis clamped) keeps its bound of 0.  Every test prints its figures before it asserts.
Shapes: axes of length 1 and 2 (shorter than the tap support and than the prefilter's 20-term start), odd sizes, axes past the
start's horizon, W past one and two wavefronts and no multiple of 4, W = 771 (past the x pass's LDS tile: the line-per-lane arm)."""
import functools

import numpy as np
import pytest
import torch

from tests import cubic_ref as R
from tests import sampler_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32

VOLUMES = [(1, 1, 1, 1, 1), (1, 1, 1, 1, 2), (1, 2, 2, 3, 4), (2, 3, 5, 6, 7), (1, 1, 3, 40, 67), (1, 1, 33, 4, 130),
           (1, 1, 1, 2, 771)]
KINDS = ["identity", "interior", "lattice", "border", "outside", "nonfinite", "ragged"]


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def volume(shape):
    return np.random.default_rng(sum(shape) * 7 + 1).random(shape, dtype=F32)


def _centres(rng, size, out):
    """random coordinates between the first and the last voxel centre"""
    return ((rng.random(out) * 2.0 - 1.0) * (1.0 - 1.0 / size)).astype(F32)


@functools.lru_cache(maxsize=None)
def grid(shape, kind):
    """(N, Do, Ho, Wo, 3) float32, seeded"""
    N, _, D, H, W = shape
    sizes = (W, H, D)
    rng = np.random.default_rng(KINDS.index(kind) * 100 + sum(shape))
    if kind == "identity":
        return S.identity(N, (D, H, W))
    out = {"interior": (3, 5, 7), "lattice": (2, 3, 7), "border": (2, 3, 5), "outside": (3, 5, 7), "nonfinite": (2, 5, 7),
           "ragged": (3, 19, 37)}[kind]                      # 105, 42, 30, 105, 70 and 2109 voxels: none a multiple of 4 or 1024
    g = np.empty((N,) + out + (3,), F32)
    for k, size in enumerate(sizes):
        if kind == "lattice":                                # exactly on lattice points
            g[..., k] = ((2.0 * rng.integers(0, size, (N,) + out) + 1.0) / size - 1.0).astype(F32)
        elif kind == "border":                               # the first and last voxel centres, and exactly +-1
            g[..., k] = rng.choice(np.array([-1.0, -(1.0 - 1.0 / size), 1.0 - 1.0 / size, 1.0], F32), (N,) + out)
        elif kind == "ragged":                               # two chunks and a ragged third, inside and past the borders
            g[..., k] = (rng.random((N,) + out) * 2.3 - 1.15).astype(F32)
        else:
            g[..., k] = _centres(rng, size, (N,) + out)
    if kind == "outside":                                    # outside [-1, 1] on one, two and three axes
        flat = g.reshape(-1, 3)
        for j in range(len(flat)):
            bits = j % 7 + 1
            for k in range(3):
                if bits >> k & 1:
                    flat[j, k] = F32((1.0 + rng.random() * 2.0) * (1 if rng.random() < 0.5 else -1))
    if kind == "nonfinite":
        flat = g.reshape(-1, 3)
        bad = np.array([np.nan, np.inf, -np.inf], F32)
        for j in range(0, len(flat), 2):
            for k in range(3):
                if (j // 2 + k) % 3 != 2:
                    flat[j, k] = bad[(j // 2 + 2 * k) % 3]
    return np.ascontiguousarray(g)


@functools.lru_cache(maxsize=None)
def references(shape):
    """{kind: (value, value bound, grid gradient, gradient bound)} of one volume, fp64: each set's own bound, except that a bound of
    0 under a reference that is not 0 everywhere is replaced by the largest bound among the volume's sets"""
    x = volume(shape)
    refs = {}
    for kind in KINDS:
        g = grid(shape, kind)
        refs[kind] = R.tolerance(R.resample, x, g) + R.tolerance(R.resample_bwd_grid, x, g, S.cotangent(x, g, 11))
    pooled = [max(r[j] for r in refs.values()) for j in (1, 3)]
    for kind, (ref, b, dref, db) in refs.items():
        if b == 0.0 and np.any(ref):
            b = pooled[0]
        if db == 0.0 and np.any(dref):
            db = pooled[1]
        refs[kind] = (ref, b, dref, db)
    return refs


def _gpu(x, g, gout=None):
    """grid_sample3d(x, g, "cubic") and, with gout, its grid gradient"""
    from keymorph_amd import ops
    xd = torch.from_numpy(x).to(DEV)
    gd = torch.from_numpy(g).to(DEV).requires_grad_(gout is not None)
    out = ops.grid_sample3d(xd, gd, "cubic")
    if gout is None:
        return _np(out)
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    return _np(out), _np(gd.grad)


@pytest.mark.parametrize("shape", VOLUMES, ids=str)
def test_coefficients_vs_fp64(shape):
    from keymorph_amd import ops
    x = volume(shape)
    ref, bound = R.tolerance(R.coefficients, x)
    got = _np(ops.cubic_coefficients(torch.from_numpy(x).to(DEV)))
    err = float(np.abs(got - ref).max())
    print(f"coefficients {shape}: error {err:.3e}, bound {bound:.3e}, max|c| {float(np.abs(ref).max()):.3f}")
    assert got.dtype == np.float32 and got.shape == x.shape
    assert err <= bound


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", VOLUMES, ids=str)
def test_values_and_grid_gradient_vs_fp64(shape, kind):
    x, g = volume(shape), grid(shape, kind)
    gout = S.cotangent(x, g, 11)
    ref, bound, dref, dbound = references(shape)[kind]
    out, dgrid = _gpu(x, g, gout)
    err, derr = float(np.abs(out - ref).max()), float(np.abs(dgrid - dref).max())
    print(f"{shape} {kind}: value error {err:.3e} (bound {bound:.3e}), grid gradient error {derr:.3e} (bound {dbound:.3e})")
    assert np.isfinite(out).all() and np.isfinite(dgrid).all()
    assert err <= bound
    assert derr <= dbound
    if kind == "identity":                                   # gives back x (the fp32 grid sits up to 1e-7 voxels off the lattice)
        back = float(np.abs(out - x).max())
        print(f"    identity: |out - x| {back:.3e}")
        assert back <= bound + float(np.abs(ref - x).max())
    # exactly 0 on a clamped axis, and on all three for a voxel with a NaN coordinate
    N, _, D, H, W = shape
    nan = np.isnan(g).any(-1)
    for k, size in enumerate((W, H, D)):
        clamped = S.source_coord(g[..., k], size)[1] == 0
        assert (dgrid[..., k][clamped | nan] == 0).all(), (shape, kind, k)
    if kind == "interior" and min(D, H, W) > 1:
        assert (dgrid != 0).all()


def test_align_img_4d_path():
    """(N, C, H, W) + (N, Ho, Wo, 2): a depth-1 volume sampled at z = 0"""
    from keymorph_amd.utils import align_img
    x = volume((2, 3, 1, 9, 70))
    g2 = (np.random.default_rng(5).random((2, 7, 33, 2)) * 2.3 - 1.15).astype(F32)
    g3 = np.concatenate([g2, np.zeros_like(g2[..., :1])], -1)[:, None]
    ref, bound = R.tolerance(R.resample, x, g3)
    got = _np(align_img(torch.from_numpy(g2).to(DEV), torch.from_numpy(x[:, :, 0]).to(DEV), "cubic"))
    err = float(np.abs(got - ref[:, :, 0]).max())
    print(f"4-D path: error {err:.3e}, bound {bound:.3e}")
    assert got.shape == (2, 3, 7, 33) and err <= bound


def test_no_gradient_to_the_volume():
    from keymorph_amd import ops
    x = torch.from_numpy(volume((1, 2, 2, 3, 4))).to(DEV)
    g = torch.from_numpy(grid((1, 2, 2, 3, 4), "interior")).to(DEV)
    with pytest.raises(NotImplementedError):
        ops.grid_sample3d(x.clone().requires_grad_(True), g, "cubic").sum().backward()
    with pytest.raises(NotImplementedError):
        ops.cubic_sample(ops.cubic_coefficients(x).requires_grad_(True), g).sum().backward()
    assert not ops.cubic_coefficients(x.clone().requires_grad_(True)).requires_grad      # no graph through the prefilter


def test_exactness():
    """two runs, a batch against its samples, channels against one-channel calls, and the two spellings: bit for bit"""
    from keymorph_amd import ops
    rng = np.random.default_rng(21)
    x = torch.from_numpy(rng.random((2, 3, 9, 10, 70), dtype=F32)).to(DEV)
    g = torch.from_numpy((rng.random((2, 3, 19, 37, 3)) * 2.3 - 1.15).astype(F32)).to(DEV)
    gout = torch.from_numpy(rng.standard_normal((2, 3, 3, 19, 37)).astype(F32)).to(DEV)

    def run(xs, gs, go):
        gs = gs.clone().requires_grad_(True)
        out = ops.grid_sample3d(xs, gs, "cubic")
        (out * go).sum().backward()
        return out.detach(), gs.grad

    out, dg = run(x, g, gout)
    out2, dg2 = run(x, g, gout)
    assert torch.equal(out, out2) and torch.equal(dg, dg2)
    coef = ops.cubic_coefficients(x)
    assert torch.equal(coef, ops.cubic_coefficients(x))
    for n in range(2):
        o1, d1 = run(x[n:n + 1].contiguous(), g[n:n + 1].contiguous(), gout[n:n + 1].contiguous())
        assert torch.equal(out[n:n + 1], o1) and torch.equal(dg[n:n + 1], d1), n
        assert torch.equal(coef[n:n + 1], ops.cubic_coefficients(x[n:n + 1].contiguous()))
    for c in range(3):
        assert torch.equal(out[:, c:c + 1], ops.grid_sample3d(x[:, c:c + 1].contiguous(), g, "cubic")), c
        assert torch.equal(coef[:, c:c + 1], ops.cubic_coefficients(x[:, c:c + 1].contiguous())), c
    gs = g.clone().requires_grad_(True)
    two = ops.cubic_sample(coef, gs)
    (two * gout).sum().backward()
    assert torch.equal(out, two) and torch.equal(dg, gs.grad)


def test_translate_by_whole_voxels_is_a_shift():
    """translate(x, t, "cubic") with integer t: out[v] = x[v + t] wherever v + t is inside, within the value bound at the grid that
    translate samples (the fp32 grid's distance from the lattice, about 1e-6 voxels, is printed, not allowed for)."""
    from keymorph_amd import ops
    from keymorph_amd.io import translate
    shape = (1, 2, 6, 7, 9)
    x = volume(shape)
    t = (1, -2, 3)                                               # (z, y, x)
    xd = torch.from_numpy(x).to(DEV)
    got = _np(translate(xd, torch.tensor([t], dtype=torch.float32, device=DEV), "cubic"))
    mat = torch.zeros(1, 3, 4, device=DEV)
    for k, n in enumerate(shape[2:]):                            # translate's matrix (ops.affine_grid acts on (z, y, x))
        mat[0, k, k] = (n - 1) / n
        mat[0, k, 3] = 2.0 * t[k] / n
    g = _np(ops.affine_grid(mat, shape[2:]))
    _, bound = R.tolerance(R.resample, x, g)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape[2:]], indexing="ij"), -1) + np.array(t)
    inside = np.all((idx >= 0) & (idx < np.array(shape[2:])), -1)
    dp = 0.0
    for k, n in enumerate(shape[2:]):
        p = S.source_coord(g[0, ..., 2 - k], n)[0]
        dp += float(np.abs(p - idx[..., k])[inside].max())
    want = x[:, :, np.clip(idx[..., 0], 0, 5), np.clip(idx[..., 1], 0, 6), np.clip(idx[..., 2], 0, 8)]
    err = float(np.abs(got - want)[:, :, inside].max())
    print(f"translate: error {err:.3e}, value bound {bound:.3e}, lattice distance {dp:.3e} voxels")
    assert inside.sum() == 5 * 5 * 6
    assert err <= bound


@functools.lru_cache(maxsize=None)
def smooth_volume():
    """32^3 Gaussian-smoothed noise (sigma = 1 voxel, mirrored ends), scaled to [0, 1]; fixed seed, no scipy"""
    v = np.random.default_rng(2024).standard_normal((32, 32, 32))
    k = np.exp(-0.5 * (np.arange(-4, 5) / 1.0) ** 2)
    k /= k.sum()
    for axis in range(3):
        p = np.pad(v, [(4, 4) if a == axis else (0, 0) for a in range(3)], mode="reflect")
        v = sum(k[j] * np.take(p, np.arange(j, j + 32), axis=axis) for j in range(9))
    v = (v - v.min()) / (v.max() - v.min())
    return v.astype(F32)[None, None]


def test_round_trip_rotation_keeps_what_trilinear_blurs():
    """The reason for the mode: +17 degrees about z and back through io.apply_mat, scored by RMS error inside the centred disc of
    radius 0.4 * 32.  scipy's pair for this construction is 0.0199 (linear) against 0.0027 (cubic).  Each GPU figure equals the
    restatement's within the bound of its round-tripped volume (| rms(a - x) - rms(b - x) | <= rms(a - b) <= max|a - b|), and
    the cubic error is at most a quarter of the trilinear one."""
    from keymorph_amd import ops
    from keymorph_amd.io import apply_mat
    x = smooth_volume()
    n = 32
    yy, xx = np.meshgrid(np.arange(n) - 15.5, np.arange(n) - 15.5, indexing="ij")
    disc = np.broadcast_to((yy * yy + xx * xx <= (0.4 * n) ** 2)[None], (n, n, n))

    def rms(v):
        return float(np.sqrt(np.mean((np.asarray(v, np.float64)[0, 0] - x[0, 0].astype(np.float64))[disc] ** 2)))

    def rot(deg):      # about z through the volume's centre, in voxel space: (n - 1) / n cancels the linspace(-1, 1) base grid;
        c, s = np.cos(np.deg2rad(deg)) * (n - 1) / n, np.sin(np.deg2rad(deg)) * (n - 1) / n      # ops.affine_grid acts on (z, y, x)
        return torch.tensor([[[(n - 1) / n, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0]]], dtype=torch.float32, device=DEV)

    xd = torch.from_numpy(x).to(DEV)
    grids = [_np(ops.affine_grid(rot(d), (n, n, n))) for d in (17.0, -17.0)]
    figures = {}
    for mode, f in (("bilinear", lambda v, g, dtype: S.grid_sample(v, g).astype(dtype)), ("cubic", R.resample)):
        got = _np(apply_mat(apply_mat(xd, rot(17.0), mode), rot(-17.0), mode))
        chain = lambda v, dtype: f(f(v, grids[0], dtype=dtype), grids[1], dtype=dtype)      # noqa: E731
        ref, bound = R.tolerance(chain, x)
        if mode == "bilinear":      # sampler_ref is fp64 only: the trilinear sampler's own forward bar (sampler_ref.assert_fwd,
            bound = 2e-6 * float(np.abs(x).max())      # 1e-6 max|x|) once per pass -- the second pass's convex weights add nothing
        figures[mode] = (rms(got), rms(ref), bound, float(np.abs(got - ref).max()))
        print(f"round trip {mode}: RMS {figures[mode][0]:.5f} (restatement {figures[mode][1]:.5f}), bound {bound:.3e}, "
              f"max |gpu - restatement| {figures[mode][3]:.3e}; std inside the disc {float(x[0, 0][disc].std()):.3f}")
    for mode, (a, b, bound, _) in figures.items():
        assert abs(a - b) <= bound, (mode, a, b, bound)
    assert figures["cubic"][0] <= 0.25 * figures["bilinear"][0]


def test_surface_is_align_img_of_the_same_grid():
    from keymorph_amd import augmentation as A
    from keymorph_amd import ops
    from keymorph_amd.io import apply_bspline, apply_mat, apply_svf, svf_grid, translate
    from keymorph_amd.transformations import AffineTransform
    from keymorph_amd.utils import align_img
    rng = np.random.default_rng(31)
    dims = (9, 10, 12)
    x = torch.from_numpy(rng.random((2, 2) + dims, dtype=F32)).to(DEV)
    mat = torch.tensor(np.eye(3, 4)[None] + rng.normal(0, 0.05, (2, 3, 4)), dtype=torch.float32, device=DEV)
    ctrl = torch.tensor(rng.normal(0, 0.03, (2, 3) + ops.bspline_lattice_shape(dims, 4)), dtype=torch.float32, device=DEV)
    assert torch.equal(apply_mat(x, mat, "cubic"), align_img(ops.affine_grid(mat, dims), x, "cubic"))
    assert torch.equal(apply_bspline(x, ctrl, mat, "cubic"), align_img(ops.bspline_grid(ctrl, dims, mat), x, "cubic"))
    for inverse in (False, True):
        assert torch.equal(apply_svf(x, ctrl, mat, 4, inverse, "cubic"),
                           align_img(svf_grid(ctrl, dims, mat, 4, inverse), x, "cubic")), inverse
    params = (torch.tensor([[1.1, 0.95, 1.05]]), torch.tensor([[0.05, -0.08, 0.03]]), torch.tensor([[0.2, -0.1, 0.15]]),
              torch.tensor([[0.02, -0.03, 0.01, 0.02, -0.01, 0.03]]))
    aug = A.AffineDeformation3d(device=DEV)
    phi = AffineTransform(matrix=aug.build_affine_matrix(2, params)).get_flow_field(x.size())
    assert torch.equal(aug.deform_img(x, params, interp_mode="cubic"), align_img(phi, x, "cubic"))
    assert torch.equal(aug(x, params=params, interp_mode="cubic"), align_img(phi, x, "cubic"))
    assert not torch.equal(align_img(phi, x, "cubic"), align_img(phi, x))
    with pytest.raises(ValueError):
        translate(x, torch.zeros(2, 3, device=DEV), "bicubic")


def test_refusals():
    from keymorph_amd import _lib, ops
    x = torch.zeros(1, 1, 3, 4, 5, device=DEV)
    g = torch.zeros(1, 2, 2, 2, 3, device=DEV)
    for bad in (x[0], x[:, :, :, :, :0]):
        with pytest.raises(ValueError):
            ops.cubic_coefficients(bad)
        with pytest.raises(ValueError):
            ops.grid_sample3d(bad, g, "cubic")
    for bad in (g[0], g[..., :2], torch.zeros(2, 2, 2, 2, 3, device=DEV)):
        with pytest.raises(ValueError):
            ops.cubic_sample(x, bad)
        with pytest.raises(ValueError):
            ops.grid_sample3d(x, bad, "cubic")
    with pytest.raises(_lib.KeymorphHipError):
        ops.cubic_coefficients(x.cpu())
    with pytest.raises(_lib.KeymorphHipError):
        ops.cubic_sample(x, g.cpu())
    with pytest.raises(_lib.KeymorphHipError):
        ops.grid_sample3d(x.cpu(), g, "cubic")
    # a channel plane of 2^29 voxels: a view of one element, so nothing that large exists before or after the refusal
    huge = torch.zeros(1, device=DEV).expand(1, 1, 1 << 9, 1 << 10, 1 << 10)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    for call in (lambda: ops.cubic_coefficients(huge), lambda: ops.cubic_sample(huge, g),
                 lambda: ops.grid_sample3d(huge, g, "cubic")):
        with pytest.raises(ValueError):
            call()
    assert torch.cuda.max_memory_allocated() < before + (1 << 28)      # (a copy of it would be 2 GiB)
    assert ops.CUBIC_MAX_PLANE == 1 << 29
    many = torch.zeros(1, device=DEV).expand(65536, 1, 1, 1, 1)      # one sample past the batch limit
    for call in (lambda: ops.cubic_coefficients(many), lambda: ops.cubic_sample(many, g.expand(65536, 2, 2, 2, 3)),
                 lambda: ops.grid_sample3d(many, g.expand(65536, 2, 2, 2, 3), "cubic")):
        with pytest.raises(ValueError):
            call()
    assert torch.cuda.max_memory_allocated() < before + (1 << 28)
