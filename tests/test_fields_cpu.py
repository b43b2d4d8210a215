"""CPU: tests/fields_ref.py, the fp64 yardstick of keymorph_amd.fields, and the test field of tests/test_fields_gpu.py -- checked
against torch's own grid_sample and against closed forms, so that the GPU tests compare with something that is itself pinned."""
import pytest
import torch
import torch.nn.functional as F

from tests import fields_ref as R

F64 = torch.float64
SHAPES = [(5, 6, 7), (12, 10, 14), (24, 20, 28)]


def _affine_on_lattice(dims, M, b, n=1):
    return (R.identity_grid(dims, n) @ M.T + b)


@pytest.mark.parametrize("dims_first,dims_then", [((5, 6, 7), (12, 10, 14)), ((12, 10, 14), (24, 20, 28)), ((24, 20, 28), (5, 6, 7))])
def test_ref_compose_is_grid_sample(dims_first, dims_then):
    first, _ = R.case_grid("D", dims_first)            # reaches past [-1, 1]: the border clamp is part of the comparison
    then, _ = R.case_grid("B", dims_then)
    first[0, 0, 0, 0] = torch.tensor([-1.0, 1.0, 1.0 - 1.0 / dims_then[0]], dtype=F64)      # borders and a voxel centre
    want = F.grid_sample(then.permute(0, 4, 1, 2, 3), first, mode="bilinear", padding_mode="border", align_corners=False)
    got = R.compose(first, then)
    assert got.shape == first.shape
    assert float((got - want.permute(0, 2, 3, 4, 1)).abs().max()) <= 1e-14


def test_ref_compose_of_affines_is_the_matrix_product():
    dims1, dims2 = (12, 10, 14), (24, 20, 28)
    M1, b1 = R.matrix(20.0, 0.6), torch.tensor([0.05, -0.03, 0.02], dtype=F64)
    M2, b2 = R.matrix(-12.0, 1.2), torch.tensor([-0.04, 0.02, 0.03], dtype=F64)
    G1, G2 = _affine_on_lattice(dims1, M1, b1), _affine_on_lattice(dims2, M2, b2)
    hull = 1 - 1 / torch.tensor([dims2[2], dims2[1], dims2[0]], dtype=F64)
    assert bool((G1.abs() < hull).all()), "the image of the first grid must stay inside the second lattice's voxel-centre hull"
    want = _affine_on_lattice(dims1, M2 @ M1, M2 @ b1 + b2)
    assert float((R.compose(G1, G2) - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("dims", SHAPES)
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_ref_invert_converges_everywhere(case, dims):
    G, mb = R.case_grid(case, dims)
    Hh, ok, its, res = R.invert(G, tol=1e-5, max_iters=20)
    assert int((~ok).sum()) == 0
    assert int(its.max()) <= 6
    ids = R.identity_grid(dims, 2)
    assert float((R.interp(G, Hh) - ids).abs().max()) <= 1e-5
    if case == "A":
        Hh, ok, _, _ = R.invert(G, tol=1e-12, max_iters=20)
        assert int((~ok).sum()) == 0
        for s, (M, b) in enumerate(mb):
            want = (ids[s] - b) @ torch.linalg.inv(M).T
            assert float((Hh[s] - want).abs().max()) <= 1e-9


@pytest.mark.parametrize("dims", SHAPES[1:])
def test_ref_invert_case_d_flags_the_unreachable(dims):
    G, _ = R.case_grid("D", dims)
    Hh, ok, _, _ = R.invert(G)
    frac = float(ok.double().mean())
    assert 0.5 < frac < 0.7                       # part of the targets is outside the image of the grid
    assert bool(torch.isfinite(Hh).all()) and float(Hh.abs().max()) <= 1.0
    ids = R.identity_grid(dims, 2)
    assert float((R.interp(G, Hh) - ids).abs().amax(dim=-1)[ok].max()) <= 1e-5


@pytest.mark.parametrize("dims", SHAPES)
def test_ref_displacement_of_an_affine_has_det_m(dims):
    G, mb = R.case_grid("A", dims)
    det = R.jacobian_det_central(R.to_displacement(G))
    for s, (M, _) in enumerate(mb):
        assert float((det[s] - torch.linalg.det(M)).abs().max()) <= 1e-12


@pytest.mark.parametrize("dims", SHAPES)
def test_ref_displacement_round_trip(dims):
    G, _ = R.case_grid("C", dims)
    d = R.to_displacement(G)
    assert d.shape == (2, 3, *dims)
    # the voxel the grid points at minus the voxel's own index, channel 0 = z
    k = torch.arange(dims[0], dtype=F64).view(-1, 1, 1)
    assert float((d[:, 0] - (((G[..., 2] + 1) * dims[0] - 1) / 2 - k)).abs().max()) <= 1e-13
    assert float((R.from_displacement(d) - G).abs().max()) <= 1e-14
    assert float(R.to_displacement(R.identity_grid(dims)).abs().max()) == 0.0
