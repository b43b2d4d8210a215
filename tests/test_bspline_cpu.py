"""CPU: the restatement of the free-form deformation (tests/bspline_ref.py) is itself pinned -- the properties of the uniform cubic
B-spline that the definition implies, the closed forms of the bending penalty, and the recovery pair's conditions for the fp64
restatement of the driver.  The GPU tests (tests/test_bspline_gpu.py) hold the kernels against this restatement."""
import torch

from tests import bspline_ref as R

F64 = torch.float64


def test_lattice_shape():
    from keymorph_amd import ops
    assert R.lattice_shape((24, 20, 36), 8) == (6, 6, 8) == ops.bspline_lattice_shape((24, 20, 36), 8)
    assert ops.bspline_lattice_shape((256, 256, 256), 8) == (35, 35, 35)
    assert ops.bspline_lattice_shape((5, 6, 7), 8) == (4, 4, 4)


def test_zero_ctrl_is_the_identity_lattice():
    dims = (5, 6, 7)
    g = R.bspline_grid(torch.zeros(2, 3, 4, 5, 6, dtype=F64), dims)
    assert torch.equal(g, R.identity(dims)[None].expand(2, *dims, 3))
    # ... which is the grid that samples every voxel at its own centre: align_corners=False coordinates ((g + 1) S - 1) / 2
    vox = ((g[0] + 1) * torch.tensor([7.0, 6.0, 5.0], dtype=F64) - 1) / 2
    assert torch.allclose(vox[2, 3, 4], torch.tensor([4.0, 3.0, 2.0], dtype=F64), atol=1e-12)


def test_partition_of_unity():
    for S, C in ((5, 4), (6, 7), (24, 6), (7, 11)):
        B = R.basis(S, C)
        assert torch.allclose(B.sum(1), torch.ones(S, dtype=F64), atol=1e-14) and (B >= 0).all()
    ctrl = torch.zeros(1, 3, 6, 5, 4, dtype=F64)
    ctrl[0, 0], ctrl[0, 1], ctrl[0, 2] = 0.25, -0.5, 0.125
    d = R.displacement(ctrl, (9, 8, 7))
    assert torch.allclose(d, torch.tensor([0.25, -0.5, 0.125], dtype=F64).expand_as(d), atol=1e-14)


def test_linear_precision():
    """sum_a B_a(t) (cell + a) = u + 1: control values linear in the index give a displacement linear in g."""
    for axis, (S, C) in enumerate(((9, 6), (8, 7), (7, 5))):
        dims, lat = (9, 8, 7), (6, 7, 5)
        ctrl = torch.zeros(1, 3, *lat, dtype=F64)
        shape = [1, 1, 1]
        shape[axis] = C
        ctrl[0, 1] = torch.arange(C, dtype=F64).reshape(shape).expand(lat)
        d = R.displacement(ctrl, dims)[0, ..., 1]
        g = (2 * torch.arange(S, dtype=F64) + 1) / S - 1
        want = (g + 1) * (C - 3) / 2 + 1
        vshape = [1, 1, 1]
        vshape[axis] = S
        assert torch.allclose(d, want.reshape(vshape).expand(dims), atol=1e-13)


def test_voxel_centre_on_a_knot_gets_the_same_value_from_either_cell():
    S, C, i = 6, 7, 1
    u = ((2 * i + 1) / S - 1 + 1) * (C - 3) / 2
    assert u == 1.0                                                   # exactly on the knot between cells 0 and 1
    c = torch.rand(C, dtype=F64, generator=torch.Generator().manual_seed(0))
    left, right = R.basis_at(S, C, i, 0), R.basis_at(S, C, i, 1)
    assert abs(float(left @ c) - float(right @ c)) <= 1e-15
    assert torch.equal(R.basis(S, C)[i], right)                       # floor(u) picks the right-hand cell, t = 0
    # C2: value, slope and curvature of the two cells' polynomials agree at the knot
    # (B(t = 1) of a cell = B(t = 0) of the next, shifted by one control point, for the weights and two derivatives)
    def poly(t):
        return [[(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6],
                [-(1 - t) ** 2 / 2, (9 * t ** 2 - 12 * t) / 6, (-9 * t ** 2 + 6 * t + 3) / 6, t ** 2 / 2],
                [(1 - t), (18 * t - 12) / 6, (-18 * t + 6) / 6, t]]
    for end, start in zip(poly(1.0), poly(0.0)):
        assert all(abs(a - b) <= 1e-15 for a, b in zip(end + [0.0], [0.0] + start))


def test_bending_closed_forms():
    lat = (5, 7, 6)
    idx = torch.stack(torch.meshgrid(*[torch.arange(c, dtype=F64) for c in lat], indexing="ij"))
    linear = (0.3 * idx[0] - 1.5 * idx[1] + 0.25 * idx[2] + 2.0)[None, None].expand(2, 3, *lat)
    assert float(R.bending(linear).abs().max()) <= 1e-24
    # q = i^2 along one axis, in one channel of three: the second difference is 2 there, the mean of its square 4 / 3
    for axis in range(3):
        q = torch.zeros(1, 3, *lat, dtype=F64)
        q[0, 1] = idx[axis] ** 2
        assert abs(float(R.bending(q)[0]) - 4.0 / 3.0) <= 1e-13
    # ... and a batch is its samples
    q = torch.rand(2, 3, *lat, dtype=F64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.bending(q)[1], R.bending(q[1:])[0])


def test_recovery_pair_conditions_hold_for_the_fp64_restatement():
    """Size 32^3, lattice 7^3, the defaults of io.register_bspline (the /4 level is skipped), identity matrix, seed 3: the mean
    displacement error after registration is at most 0.5 voxel and at most a third of the identity's.
    (The restatement gives 0.285 of 1.786 voxel.)"""
    fixed, moving = R.recovery_pair()
    assert fixed.shape == moving.shape == (1, 1, 32, 32, 32) and R.true_ctrl().shape == (1, 3, 7, 7, 7)
    assert 0.0 <= float(fixed.min()) and float(fixed.max()) <= 1.0 and float(moving.min()) == 0.0
    residual, start = R.recovery_run()
    print(f"fp64 restatement: residual {residual:.3f} voxel, identity {start:.3f} voxel")
    assert residual <= 0.5 and residual <= start / 3
