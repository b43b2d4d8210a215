"""CPU: pins tests/grids_ref.py, the fp64 restatement behind tests/test_grids_edges_gpu.py.  Run in float32 it is the oracle to
rounding and reproduces the reference's goldens; the lattice is torch.linspace bit for bit in the single-rounding form; the
approximations of common.h hold their stated bounds; every bar is positive and the fp32 CPU oracle sits inside it; the Jacobian
cases allow an exact count; and every dispatch arm of the kernels has a case."""
import numpy as np
import pytest
import torch

from oracle import keymorph_oracle as O
from tests import grids_ref as R
from tests.util import T, golden

U = R.U


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _inside(tag, err, bar, quiet=False):
    err, bar = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bar, np.float64), np.shape(err))
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))
    if not quiet:
        print(f"{tag}: oracle error / bar {ratio:.3f}")
    assert ratio <= 1.0, f"{tag}: the fp32 oracle is at {ratio:.3f} of the bar"
    return ratio


# ------------------------------------------------------------------------------------------------------------ lattice
def test_lattice_is_linspace_in_the_single_rounding_form():
    differ = 0
    for n in sorted(set(R.LATTICE_CHECKED_N + R.LATTICE_N)):
        want = torch.linspace(-1, 1, n).numpy()
        assert np.array_equal(_bits(R.lattice(n)), _bits(want))
        assert np.array_equal(_bits(R.lattice_single_rounding(n)), _bits(want)), n
        differ += int((_bits(R.lattice_two_roundings(n)) != _bits(want)).any())
    assert differ > 100, "the separately rounded product-then-sum form is not what torch computes"
    assert R.lattice(1).tolist() == [-1.0] and R.lattice_single_rounding(1).tolist() == [-1.0]
    assert R.lattice(2).tolist() == [-1.0, 1.0] and R.lattice(3).tolist() == [-1.0, 0.0, 1.0]


def test_midpoint_rule_matters():
    """i < n / 2 against i <= n / 2: the two branches differ in bits at the midpoint of some even n of the table, so a kernel with
    the wrong rule cannot pass the bit equality"""
    hit = []
    for n in R.LATTICE_N:
        if n % 2 == 0 and n > 2:
            s, i = float(R.lattice_step(n)), n // 2
            lo, hi = np.float32(s * i - 1.0), np.float32(1.0 - s * (n - 1 - i))
            if lo != hi:
                hit.append(n)
    print("n with a midpoint that tells the rules apart:", hit)
    assert len(hit) >= 3


def test_identity_grid_layout():
    g = R.identity_grid((2, 3, 4))
    assert g.shape == (2, 3, 4, 3) and g[1, 2, 0].tolist() == [-1.0, 1.0, 1.0]
    assert np.array_equal(g, O.affine_grid(torch.eye(4)[None], (2, 3, 4))[0].numpy())
    assert R.identity_grid((1, 1, 1)).tolist() == [[[[-1.0, -1.0, -1.0]]]]


# ----------------------------------------------------------------------------------------------- common.h's bounds
def _common_h_constants(path=None):
    import os
    import re
    path = path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "keymorph_amd", "csrc", "common.h")
    src = open(path).read()
    magic = int(re.search(r"__uint_as_float\((0x[0-9a-fA-F]+)u - \(__float_as_uint\(d2\) >> 1\)\)", src).group(1), 16)
    centre = np.float32(re.search(r"constexpr float kTpsRsqCentre = ([0-9.eE+-]+)f;", src).group(1))
    m = re.search(r"constexpr float kTpsEpsLog2x2 = ([0-9.eE+-]+)f \* ([0-9.eE+-]+)f / ([0-9.eE+-]+)f;", src)
    k = np.float32(m.group(1)) * np.float32(m.group(2)) / np.float32(m.group(3))
    return magic, float(centre), float(k)


def test_common_h_holds_the_constants_the_bounds_are_derived_for():
    """the bounds below belong to these constants: the magic number of the estimate, its centring factor (with 1.0 in its place the
    estimate is off by up to 6.2 % on one side) and the factor of the log correction"""
    assert _common_h_constants() == (0x5f3759df, R.RSQ_CENTRE, R.K_LOG2X2)


def test_log_correction_and_estimate_bounds():
    """the integer reciprocal-square-root estimate, centred, is within 4.8 % of 1 / r, and the log correction built on it within
    4.8e-8 / r of ln(1 + e / r), over d2 from 1e-6 (a voxel on a keypoint) to 48 (keypoints at +-3)"""
    d2 = np.exp(np.linspace(np.log(1e-6), np.log(48.0), 2_000_001)).astype(np.float32)
    d2 = np.concatenate([d2, np.float32(1e-6) * (1 + np.arange(0, 4096, dtype=np.float32) * np.float32(2.0 ** -20))])
    err, rel = R.rsq_correction_error(np.maximum(d2, np.float32(1e-6)))
    print(f"log correction: r x error <= {err.max():.3e} (stated 4.8e-8); estimate within {rel.max():.4f} of 1 / r (stated 0.048)")
    assert 4.7e-8 <= err.max() <= R.LOG_CORR and 0.047 <= rel.max() <= R.EST_REL
    r = np.sqrt(np.float64(1e-6))
    t = 1e-6 / r
    assert abs(1 / (1 + t) - (1 - t)) <= t * t <= 1.0001e-6


# -------------------------------------------------------------------------- the restatement in float32 is the oracle
def test_float32_restatement_equals_the_oracle_and_the_goldens():
    o, a = golden("ops_small.npz"), golden("augment_small.npz")
    r = np.random.default_rng(3)
    # affine grid
    shape = (6, 7, 8)
    M = torch.inverse(T(o["at_matrix"]))[0, :3].numpy()
    np.testing.assert_allclose(R.affine_grid(M, shape, np.float32), o["at_grid"][0], atol=2e-6)
    np.testing.assert_allclose(R.affine_grid(M, shape, np.float32), O.affine_grid(O.square(T(M)[None]), shape)[0].numpy(), atol=8 * U * 4)
    cot = r.standard_normal(shape + (3,)).astype(np.float32)
    Mt = T(M)[None].requires_grad_(True)
    (O.affine_grid(O.square(Mt), shape)[0] * T(cot)).sum().backward()
    np.testing.assert_allclose(R.affine_grid_adjoint(cot, shape, np.float32)[0], Mt.grad[0].numpy(), atol=1e-4)
    np.testing.assert_allclose(R.affine_grid_adjoint(cot, shape)[0], Mt.grad[0].numpy(), atol=1e-4)
    # TPS
    for k in ("k12", "k64"):
        theta, ctrl = o[f"{k}_tps0p1_theta"][0], o[f"{k}_pf"][0]
        np.testing.assert_allclose(R.tps_grid(theta, ctrl, shape, np.float32), o[f"{k}_tps0p1_grid"][0], atol=2e-5)
        np.testing.assert_allclose(R.tps_grid(theta, ctrl, shape), o[f"{k}_tps0p1_grid"][0], atol=2e-5)
        pts = r.uniform(-0.9, 0.9, (33, 3)).astype(np.float32)
        want = O.tps_transform_points(T(theta)[None], T(ctrl)[None], T(pts)[None])[0].numpy()
        np.testing.assert_allclose(R.tps_points(theta, ctrl, pts, np.float32), want, atol=1e-5)
        want = O.tps_transform_points(*(T(x, torch.float64)[None] for x in (theta, ctrl, pts)))[0].numpy()
        np.testing.assert_allclose(R.tps_points(theta, ctrl, pts), want, atol=1e-13, rtol=1e-13)
    # augmentation
    p = [a[f"params_{k}"] for k in ("scale", "offset", "theta", "shear")]
    np.testing.assert_allclose(R.augment_matrix(*p, dtype=torch.float32), a["params_matrix"], atol=1e-6)
    np.testing.assert_allclose(R.augment_matrix(*p), a["params_matrix"], atol=1e-6)
    # Jacobian determinant
    gp = np.ascontiguousarray(np.moveaxis(a["jd_grid"][0], -1, 0))
    np.testing.assert_allclose(R.jacobian_det(gp, torch.float32), a["jd_det"], atol=1e-6)
    (mean, std, neg), _ = R.jacobian_stats(R.jacobian_det(gp), R.jacobian_bar(gp))
    assert abs(std - float(a["jd_std"][0])) < 1e-6 and neg == int(a["jd_neg"][0])
    # argmax one-hot: the oracle's hard Dice expression, NaN classes included
    for cls in R.ARGMAX_CLASSES:
        for C in R.ARGMAX_C:
            x = R.argmax_case(cls, C, 257)
            t = T(x)
            want = torch.zeros_like(t).scatter(1, t.argmax(dim=1, keepdim=True), 1.0).numpy()
            assert np.array_equal(R.argmax_onehot(x), want), (cls, C)
    la = T(o["loss_a"]).reshape(2, 4, -1)
    assert np.array_equal(R.argmax_onehot(la.numpy()), torch.nn.functional.one_hot(la.argmax(1), 4).permute(0, 2, 1).float().numpy())


def test_argmax_classes_hold_what_they_are_named_after():
    for C in R.ARGMAX_C:
        x = R.argmax_case("signed_zero", C, 256)
        assert (x == 0).all() and (C == 1 or (np.signbit(x).any() and not np.signbit(x).all()))
        assert R.argmax_onehot(x)[:, 0].all()                                        # +0 == -0: the first index wins
        assert R.argmax_onehot(R.argmax_case("all_equal", C, 255))[:, 0].all()
        x = R.argmax_case("nan_two", C, 257)
        assert np.isnan(x).any()
        if C >= 3:
            assert (R.argmax_onehot(x)[:, C - 3, ::2] == 1).all() and (R.argmax_onehot(x)[:, C - 1, 1::2] == 1).all()
        x = R.argmax_case("inf", C, 257)
        assert np.isinf(x).any()


# ------------------------------------------------------------------------------------- bars: positive, and not impossible
@pytest.mark.parametrize("name", R.AFFINE_MATRICES)
def test_affine_grid_oracle_inside_the_bar(name):
    worst = 0.0
    for shape in R.AFFINE_SHAPES:
        M = R.affine_matrix(name)
        got = O.affine_grid(O.square(T(M)), shape).numpy()
        for n in range(M.shape[0]):
            bar, truth = R.affine_grid_bar(M[n], shape), R.affine_grid(M[n], shape)
            assert (bar[truth != 0] > 0).all()                                     # an exact zero has bar 0: it is demanded exactly
            worst = max(worst, _inside(f"{name} {shape}", np.abs(got[n] - truth), bar, True))
    print(f"{name}: fp32 oracle error / bar {worst:.3f}")


@pytest.mark.parametrize("kind", ["random", "cancelling"])
def test_affine_adjoint_oracle_inside_the_bar(kind):
    worst = 0.0
    for shape in R.AFFINE_SHAPES + (R.AFFINE_BIG,):
        N = 1 if shape == R.AFFINE_BIG else 3
        cot = R.affine_cotangent(kind, shape, N)
        for n in range(N):
            truth, mag = R.affine_grid_adjoint(cot[n], shape)
            bar = R.affine_adjoint_bar(truth, mag, int(np.prod(shape)))
            assert (bar > 0).all()
            worst = max(worst, _inside(f"{kind} {shape}", np.abs(R.emulate_affine_adjoint(cot[n], shape) - truth), bar, True))
            if kind == "cancelling" and np.prod(shape) > 500:
                assert (np.abs(truth[:, 3]) < 1e-2 * mag[:, 3]).all()
    print(f"{kind}: error of the float32 emulation of the kernels' order / bar {worst:.3f}")
    assert R.affine_bwd_geometry(int(np.prod(R.AFFINE_BIG))) == (1024, 17)
    assert R.affine_bwd_geometry(1024 * 4096) == (1024, 16) and R.affine_bwd_geometry(585) == (1, 3)


def _tps_inside(tag, res):
    truth, arith, allow, oerr = res
    out = {}
    for k in truth:
        assert (arith[k][truth[k] != 0] > 0).all(), (tag, k)               # an exact zero may have bar 0
        out[k] = _inside(f"{tag} {k}", oerr[k], arith[k] + allow[k] / 2, True)
    return out


@pytest.mark.parametrize("name", list(R.TPS_GRID_CASES))
def test_tps_grid_oracle_inside_the_bar(name):
    N = R.TPS_GRID_CASES[name][3]
    for n in range(N):
        res = R.tps_grid_truth(name, n)
        ratios = _tps_inside(f"{name}[{n}]", res)
        print(f"{name}[{n}]: oracle error / (arithmetic + allowance / 2) " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()),
              " allowance / max arithmetic " + "  ".join(f"{k} {res[2][k] / res[1][k].max():.2f}" for k in res[2] if res[2][k]))
    if R.TPS_GRID_CASES[name][2] == "wzero":
        assert not res[0]["dctrl"].any()


@pytest.mark.parametrize("name", list(R.TPS_POINTS_CASES))
def test_tps_points_oracle_inside_the_bar(name):
    N = R.TPS_POINTS_CASES[name][3]
    for n in range(N):
        res = R.tps_points_truth(name, n)
        ratios = _tps_inside(f"{name}[{n}]", res)
        print(f"{name}[{n}]: oracle error / (arithmetic + allowance / 2) " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def test_tps_case_classes():
    """coincident pairs sit at d2 = 1e-6; the unit case exposes U itself; identical keypoints are identical"""
    theta, ctrl, pts, _ = R.tps_points_case("self512")
    assert np.array_equal(ctrl, pts)
    theta, ctrl, cot, shape = R.tps_grid_case("plain_nodes")
    p = R.lattice_points(shape)
    for n in range(ctrl.shape[0]):
        hits = (ctrl[n][:, None, :] == p[None]).all(-1)
        assert hits.any(1).all()                                                  # every keypoint on a lattice node, bit for bit
        assert hits[0, 0] and hits[1, -1]                                         # corners
    theta, ctrl, cot, shape = R.tps_grid_case("d1_unit")
    out = R.tps_grid(theta[0], ctrl[0], shape)
    i = int(np.argmax((R.lattice_points(shape) == ctrl[0, 0]).all(-1)))
    r = np.sqrt(1e-6)
    assert np.allclose(out.reshape(-1, 3)[i], 1e-6 * np.log(r + 1e-6), rtol=1e-12)
    theta, ctrl, cot, shape = R.tps_grid_case("plain_vec_twin")
    assert np.array_equal(ctrl[:, 0], ctrl[:, 1])
    theta, ctrl, cot, shape = R.tps_grid_case("h1_outside")
    assert (np.abs(ctrl) > 2.5).all()


@pytest.mark.parametrize("B", R.AUGMENT_B)
def test_augment_oracle_inside_the_bar(B):
    p = R.augment_case(B)
    truth = R.augment_matrix(*p)
    bar = R.augment_bar(*p, trig=1.0)
    err = np.abs(R.augment_matrix(*p, dtype=torch.float32) - truth)
    if B == 1:
        assert np.array_equal(truth[0], np.eye(4)) and not err.any()
    else:
        assert (bar[:, :3] > 0).all()
    _inside(f"B {B}", err, R.augment_bar(*p, trig=0.5))
    if B == 64:
        th = p[2]
        assert np.float32(np.pi) in th and np.float32(-2 * np.pi) in th and np.float32(np.pi / 2) in th and (th[6] == 0).all()


@pytest.mark.parametrize("name", R.JAC_CASES)
def test_jacobian_oracle_inside_the_bar_and_the_count_is_decidable(name):
    d = R.jacobian_case(name)
    truth, bar = R.jacobian_det(d), R.jacobian_bar(d)
    assert truth.shape == tuple(s - 4 for s in d.shape[1:]) and (bar > 0).all()
    _inside(name, np.abs(R.jacobian_det(d, torch.float32) - truth), bar)
    # the count condition: nothing but an exact zero within its own bar of zero -- no voxel is excused
    near = (np.abs(truth) <= bar) & (truth != 0)
    assert not near.any(), f"{name}: {int(near.sum())} determinants within their bar of zero"
    (mean, std, neg), (bm, bs) = R.jacobian_stats(truth, bar)
    assert bm > 0 and bs > 0
    if name == "exact_zero":
        assert not truth.any() and neg == truth.size and mean == 0 and std == 0
    if name == "small_fold":
        assert 0 < neg < truth.size
    if name == "one_interior":
        assert truth.size == 1
    if name == "big":
        assert truth.size == 1061208 > 4096 * 256 and neg == 13688


# --------------------------------------------------------------------------------------------- every arm has a case
def test_every_dispatch_arm_has_a_case():
    geo = {k: R.tps_geometry(v[1], int(np.prod(v[0])), v[0]) for k, v in R.TPS_GRID_CASES.items()}
    has = lambda **kw: [k for k, g in geo.items() if all(g[a] == b for a, b in kw.items())]                   # noqa: E731
    assert len(has(fwd_arm="w8")) >= 2 and has(fwd_arm="w8", fwd_blocks=2)
    assert len(has(fwd_arm="w4")) >= 2 and all(R.TPS_GRID_CASES[k][0][2] % 8 for k in has(fwd_arm="w4"))
    assert has(fwd_arm="plain", vector_stores=False) and has(fwd_arm="plain", vector_stores=True)
    assert has(bwd_rows=False, chunks=2, ragged_stage=True) and has(bwd_rows=True, chunks=2) and has(bwd_rows=True, stages_per_row=2)
    assert has(ktiles=2) and has(lds_limit=True)
    assert {R.TPS_GRID_CASES[k][1] for k in geo} >= {1, 4, 5, 130, 512, 513, 2048}
    assert {R.TPS_GRID_CASES[k][2] for k in geo} >= {"random", "nodes", "twin", "outside", "wzero", "unit"}
    assert {R.TPS_GRID_CASES[k][3] for k in geo} == {1, 3}
    assert any(v[0][0] == 1 for v in R.TPS_GRID_CASES.values()) and any(v[0][1] == 1 for v in R.TPS_GRID_CASES.values())
    assert (5 * 9 * 190 - R.VCHUNK) == 358 == 256 + 102
    pg = {k: R.tps_geometry(v[0], v[1]) for k, v in R.TPS_POINTS_CASES.items()}
    assert {v[1] for v in R.TPS_POINTS_CASES.values()} >= {1, 3, 4, 70, 72, 1025, 8193}
    assert any(g["fwd_blocks"] == 2 for g in pg.values()) and any(g["chunks"] == 2 for g in pg.values())
    assert any(g["vector_stores"] for g in pg.values()) and any(not g["vector_stores"] for g in pg.values())
    assert any(g["ktiles"] == 2 for g in pg.values())
    assert {(v[0], v[1]) for v in R.TPS_POINTS_CASES.values() if v[2] == "self"} == {(64, 64), (512, 512)}
    # affine grid: both store paths, fewer than four voxels, one-voxel axes, the loop's second trip
    nv = [int(np.prod(s)) for s in R.AFFINE_SHAPES]
    assert any(n % 4 for n in nv) and any(n % 4 == 0 and n >= 4 for n in nv) and any(n < 4 for n in nv)
    assert all(any(s[a] == 1 for s in R.AFFINE_SHAPES) for a in range(3))
    assert int(np.prod(R.AFFINE_BIG)) == 4196352 > 1024 * 4096
    assert set(R.LATTICE_N) >= set(range(1, 131)) | {255, 256, 257} and len(R.lattice_shapes()) == 3 * len(R.LATTICE_N)
