"""GPU: keymorph_amd.fields (csrc/fields.hip) -- compose, invert, identity_grid and the displacement hand-over -- against the
existing sampler (bit for bit) and against the fp64 restatement of tests/fields_ref.py (pinned by tests/test_fields_cpu.py).

Shapes: (5, 6, 7) is less than one 1024-voxel chunk, (12, 10, 14) two chunks with a ragged tail, (24, 20, 28) fourteen; none is a
multiple of the chunk, W = 7 / 10 / 14 / 20 / 28 covers W % 4 != 0.  n = 2 with another transform per sample (fields_ref.case_grid).

The bars.  ULP = 2^-23.
  compose vs fp64: the kernel's coordinate is off by a few 2^-24 S voxels, the blend is 8 fmas: 16 ULP of max |then|.
  displacement: Ids = (2i+1-S)/S is one rounding (2^-24 for |Ids| < 1), g - Ids another (2^-24 for |g - Ids| < 2), the product
    with S/2 a third (2^-24 relative to a displacement of at most S): under 4 x 2^-24 S = 2^-22 S voxels.
  invert: the kernel stops at max |residual| <= tol in fp32; the fp64 evaluation of the same point differs from the fp32 one by
    rounding (~1e-6, the issue's fp32 floor is 4e-6): 2 tol.  For an affine grid H - M^-1 (Ids - b) = M^-1 residual."""
import functools

import pytest
import torch

from keymorph_amd import _lib, fields, loss_ops
from keymorph_amd.utils import align_img
from tests import fields_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
ULP = 2.0 ** -23
SHAPES = [(5, 6, 7), (12, 10, 14), (24, 20, 28)]
TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _case(case, dims):
    """fp32 grid on the GPU, the same values in fp64 on the CPU, the per-sample (M, b)."""
    G, mb = R.case_grid(case, dims)
    g32 = G.float()
    return g32.to(DEV), g32.to(F64), mb


@functools.lru_cache(maxsize=None)
def _ids(dims):
    return R.identity_grid(dims, 2)


@functools.lru_cache(maxsize=None)
def _ref_invert(case, dims):
    """The fp64 solve of the restatement, iterated well past the kernel's tolerance."""
    return R.invert(_case(case, dims)[1], tol=1e-10, max_iters=60)


def _residual64(G64, Hh):
    """max-norm of grid(H) - Ids per voxel, evaluated in fp64 on the CPU: independent of the kernel's own residual."""
    return (R.interp(G64, Hh.cpu().to(F64)) - _ids(tuple(G64.shape[1:4]))).abs().amax(dim=-1)


# ---- 1. compose ----------------------------------------------------------------------------------------------------------
def _first_grid(dims_first, dims_then):
    """Case D on the lattice of `first` (it reaches past [-1, 1]) with hand-placed entries: lattice points of `then`, the
    borders, far outside, NaN."""
    first = _case("D", dims_first)[0].clone()
    ids_then = R.identity_grid(dims_then)[0].float()
    flat = first.view(2, -1, 3)
    pts = ids_then.reshape(-1, 3)
    k = min(pts.shape[0], flat.shape[1] // 3)
    flat[0, :k] = pts[:k].to(DEV)                                      # on lattice points (first rows of `then`)
    flat[1, :k] = pts[-k:].to(DEV)                                     # ... and its last rows
    flat[0, k] = torch.tensor([-1.0, 1.0, -1.0], device=DEV)
    flat[0, k + 1] = torch.tensor([3.0, -2.5, 1.0], device=DEV)
    flat[1, k] = torch.tensor([float("nan"), 0.1, 0.2], device=DEV)
    flat[1, k + 1] = torch.tensor([0.3, float("nan"), float("nan")], device=DEV)
    flat[0, -1] = torch.tensor([1.0 - 1.0 / dims_then[2], float("nan"), -5.0], device=DEV)
    return first


@pytest.mark.parametrize("dims_first,dims_then", [((5, 6, 7), (12, 10, 14)), ((12, 10, 14), (24, 20, 28)),
                                                  ((24, 20, 28), (5, 6, 7)), ((24, 20, 28), (24, 20, 28)),
                                                  ((12, 10, 14), (4, 3, 1))])      # W = 1: no x-pair to load
def test_compose_is_the_sampler_bit_for_bit(dims_first, dims_then):
    first = _first_grid(dims_first, dims_then)
    then, then64, _ = _case("B", dims_then)
    got = fields.compose(first, then)
    assert got.shape == first.shape and got.dtype == torch.float32 and got.is_contiguous()
    old = align_img(first, then.permute(0, 4, 1, 2, 3).contiguous()).permute(0, 2, 3, 4, 1)
    assert torch.equal(got, old)
    ref = R.compose(first.cpu().to(F64), then64)
    err = float((got.cpu().to(F64) - ref).abs().max())
    bound = 16 * ULP * float(then64.abs().max())
    print(f"compose {dims_first} o {dims_then}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # a permuted view goes through ops._prep
    assert torch.equal(fields.compose(first, then.permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3)), got)


def test_compose_warps_like_two_samplings_of_a_linear_image():
    """align_img(compose(G1, G2), x) = align_img(G1, align_img(G2, x)) up to rounding when the blend of x is linear: x a linear
    ramp, and both images inside the voxel-centre hulls (no clamping)."""
    dims = (12, 10, 14)
    M1, b1 = R.matrix(20.0, 0.6), torch.tensor([0.05, -0.03, 0.02], dtype=F64)
    M2, b2 = R.matrix(-12.0, 0.7), torch.tensor([-0.04, 0.02, 0.03], dtype=F64)
    ids = R.identity_grid(dims, 1)
    G1, G2 = (ids @ M1.T + b1).float().to(DEV), (ids @ M2.T + b2).float().to(DEV)
    x = (ids[..., 0] * 0.5 - ids[..., 1] * 0.25 + ids[..., 2] + 2.0).unsqueeze(1).float().to(DEV)
    once = align_img(fields.compose(G1, G2), x)
    twice = align_img(G1, align_img(G2, x))
    assert float((once - twice).abs().max()) <= 32 * ULP * float(x.abs().max())


# ---- 2. identity, displacement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES)
def test_identity_grid(dims):
    got = fields.identity_grid((2, 1, *dims), DEV)
    assert got.shape == (2, *dims, 3) and got.dtype == torch.float32
    assert float((got.cpu().to(F64) - _ids(dims)).abs().max()) <= 2.0 ** -24
    assert torch.equal(fields.identity_grid(dims, DEV)[0], got[1])
    x = torch.rand(2, 1, *dims, device=DEV)
    assert float((align_img(got, x) - x).abs().max()) <= 4 * ULP * max(dims)      # fractions of at most 2^-24 S per axis


@pytest.mark.parametrize("dims", SHAPES)
def test_displacement_against_fp64(dims):
    G, G64, _ = _case("C", dims)
    d = fields.to_displacement(G)
    assert d.shape == (2, 3, *dims) and d.is_contiguous()
    err = (d.cpu().to(F64) - R.to_displacement(G64)).abs()
    for ch, S in enumerate(dims):                                # channels (z, y, x)
        e = float(err[:, ch].max())
        print(f"to_displacement {dims} channel {ch}: max err {e:.3e} voxels, bound {2.0 ** -22 * S:.3e}")
        assert e <= 2.0 ** -22 * S
    back = fields.from_displacement(d)
    assert back.shape == G.shape
    assert bool(((back - G).abs() <= 4 * ULP * (1 + G.abs())).all())
    assert float((back.cpu().to(F64) - R.from_displacement(d.cpu().to(F64))).abs().max()) <= 4 * ULP * 3
    assert float(fields.to_displacement(fields.identity_grid(dims, DEV)).abs().max()) == 0.0
    # non-contiguous input (ops._prep)
    assert torch.equal(fields.to_displacement(G.permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3)), d)


@pytest.mark.parametrize("dims", SHAPES)
def test_displacement_feeds_the_jacobian_metrics(dims):
    G, _, mb = _case("A", dims)
    d = fields.to_displacement(G)
    for s in range(2):
        assert loss_ops.jdstd(d[s:s + 1]) < 1e-5
        assert loss_ops.jdlessthan0(d[s:s + 1]) == 0
        det = loss_ops._jacobian_determinant(d[s:s + 1])
        assert float((det - float(torch.linalg.det(mb[s][0]))).abs().max()) < 1e-4
    M, b = mb[0]
    mirrored = (R.identity_grid(dims, 1) @ (M @ torch.diag(torch.tensor([-1.0, 1.0, 1.0], dtype=F64))).T + b).float().to(DEV)
    assert loss_ops.jdlessthan0(fields.to_displacement(mirrored), as_percentage=True) == 1.0


# ---- 3. invert, everything reachable --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES)
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_invert_converges_everywhere(case, dims):
    G, G64, mb = _case(case, dims)
    Hh, conv, unconv, maxres = fields.invert(G, tol=TOL, return_info=True)
    assert Hh.shape == G.shape and conv.shape == (2, *dims) and conv.dtype == torch.uint8
    assert unconv.dtype == torch.int64 and maxres.dtype == torch.float32 and unconv.shape == maxres.shape == (2,)
    res = _residual64(G64, Hh)
    print(f"invert {case} {dims}: unconverged {unconv.tolist()}, reported max residual {maxres.tolist()}, "
          f"fp64 max residual {float(res.max()):.3e}")
    assert unconv.tolist() == [0, 0] and bool((conv == 1).all())
    assert float(maxres.max()) <= TOL
    assert float(res.max()) <= 2 * TOL
    assert torch.equal(fields.invert(G), Hh)
    if case == "A":
        for s, (M, b) in enumerate(mb):
            Mi = torch.linalg.inv(M)
            want = (_ids(dims)[s] - b) @ Mi.T
            err = float((Hh[s].cpu().to(F64) - want).abs().max())
            assert err <= 2 * TOL * float(Mi.abs().sum(dim=1).max())
    # compose(H, grid) = Ids, by the kernel under test as well
    assert float((fields.compose(Hh, G).cpu().to(F64) - _ids(dims)).abs().max()) <= 2 * TOL


# ---- 4. invert, part of the targets unreachable ---------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES)
def test_invert_flags_what_it_cannot_reach(dims):
    G, G64, _ = _case("D", dims)
    Hh, conv, unconv, maxres = fields.invert(G, tol=TOL, return_info=True)
    c64, ok64, _, _ = _ref_invert("D", dims)
    inside = (c64.abs() <= 1 - 3 / torch.tensor([dims[2], dims[1], dims[0]], dtype=F64)).all(dim=-1)
    must = ok64 & inside                                  # solved in fp64, the solution at least one voxel inside the hull
    conv_c = conv.cpu().bool()
    print(f"invert D {dims}: converged {int(conv_c.sum())} of {conv_c.numel()}, fp64 solves {int(ok64.sum())}, "
          f"required {int(must.sum())}, missing {int((must & ~conv_c).sum())}")
    assert int(must.sum()) > 0 and int((~ok64).sum()) > 0
    assert int((must & ~conv_c).sum()) == 0
    res = _residual64(G64, Hh)
    assert float(res[conv_c].max()) <= 2 * TOL
    assert float(maxres.max()) <= TOL
    assert bool(torch.isfinite(Hh).all()) and float(Hh.abs().max()) <= 1.0
    assert unconv.tolist() == (conv == 0).sum(dim=(1, 2, 3)).tolist()
    assert set(conv.unique().tolist()) <= {0, 1}


@pytest.mark.parametrize("at,on_start", [((11, 9, 13), False), ((12, 10, 14), True)])
def test_invert_nan_entry_flags_its_neighbourhood_only(at, on_start):
    """One NaN entry in sample 0.  The voxels whose solution lies in a cell that touches the entry cannot be evaluated: flagged.
    An iterate strays from its solution by the start's error -- the wobble a S / 2 ||M^-1|| = 0.6 voxels here -- plus a step, so
    nothing further than 3 voxels from the entry may change.  The affine start is fitted on every second lattice point at this
    size: an entry off that subsample leaves every other voxel bit-identical, one on it (dropped from the fit) moves the
    start, and the other voxels are held to the residual bound instead."""
    dims = (24, 20, 28)
    G, G64, _ = _case("B", dims)
    H0, conv0, _, _ = fields.invert(G, tol=TOL, return_info=True)
    assert bool((conv0 == 1).all())
    G2 = G.clone()
    G2[0, at[0], at[1], at[2], 1] = float("nan")
    H2, conv2, unconv2, maxres2 = fields.invert(G2, tol=TOL, return_info=True)
    assert bool(torch.isfinite(H2).all()) and float(H2.abs().max()) <= 1.0
    # distance (voxels of the grid's lattice, max over the axes) of every voxel's solution from the entry
    vox = ((H0[0].cpu().to(F64) + 1) * torch.tensor([dims[2], dims[1], dims[0]], dtype=F64) - 1) / 2
    dist = (vox - torch.tensor([at[2], at[1], at[0]], dtype=F64)).abs().amax(dim=-1)
    flagged = conv2[0].cpu() == 0
    assert int(flagged.sum()) > 0 and int(unconv2[0]) == int(flagged.sum()) and int(unconv2[1]) == 0
    assert bool(flagged[dist < 1].all())
    assert not bool(flagged[dist > 3].any())
    far = (dist > 3).to(DEV)
    if on_start:
        G2z = torch.nan_to_num(G2.cpu().to(F64), nan=0.0)       # (the far voxels' cells do not hold the entry)
        res = (R.interp(G2z, H2.cpu().to(F64)) - _ids(dims)).abs().amax(dim=-1)
        assert float(res[0][dist > 3].max()) <= 2 * TOL and float(res[1].max()) <= 2 * TOL
        assert bool((conv2[1] == 1).all())
    else:
        assert torch.equal(H2[0][far], H0[0][far])
        assert torch.equal(H2[1], H0[1]) and torch.equal(conv2[1], conv0[1])
    assert float(maxres2.max()) <= TOL


# ---- 5. determinism -------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    dims = (24, 20, 28)
    G = _case("D", dims)[0]
    then = _case("B", (12, 10, 14))[0]
    runs = []
    for _ in range(2):
        inv = fields.invert(G, return_info=True)
        d = fields.to_displacement(G)
        runs.append((fields.identity_grid(dims, DEV), fields.compose(G, then), *inv, d, fields.from_displacement(d)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 6. errors ------------------------------------------------------------------------------------------------------------
def test_errors():
    G = _case("B", (5, 6, 7))[0]
    d = fields.to_displacement(G)
    for fn, arg in ((fields.invert, G), (fields.to_displacement, G), (fields.from_displacement, d)):
        with pytest.raises(_lib.KeymorphHipError):
            fn(arg.double())
        with pytest.raises(_lib.KeymorphHipError):
            fn(arg.cpu())
        with pytest.raises(RuntimeError, match="requires grad"):
            fn(arg.clone().requires_grad_(True))
        with torch.no_grad():
            fn(arg.clone().requires_grad_(True))
    for bad in (G.double(), G.cpu()):
        with pytest.raises(_lib.KeymorphHipError):
            fields.compose(bad, G)
        with pytest.raises(_lib.KeymorphHipError):
            fields.compose(G, bad)
    with pytest.raises(RuntimeError, match="requires grad"):
        fields.compose(G, G.clone().requires_grad_(True))
    with pytest.raises(_lib.KeymorphHipError):
        fields.identity_grid((5, 6, 7), "cpu")
    for shape in ((2, 1, 6, 7, 3), (2, 6, 1, 7, 3), (2, 6, 7, 1, 3)):
        with pytest.raises(ValueError):
            fields.invert(torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError):
        fields.to_displacement(G[..., :2])
    with pytest.raises(ValueError):
        fields.compose(G[:1], G)
