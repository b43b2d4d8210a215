"""CPU: the fp64 restatement of tests/fits_ref.py pinned against oracle/keymorph_oracle.py in fp64, its finite-difference
gradients against fp64 autograd where that is finite, the reasons why neither the fp32 oracle nor fp64 autograd is the
yardstick of tests/test_fits_edges_gpu.py everywhere, and the class of every case of the table."""
import numpy as np
import pytest
import torch

from oracle import keymorph_oracle as O
from tests import fits_ref as R

CASES = R.fit_cases()
BY_NAME = {c["name"]: c for c in CASES}
T64 = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64))          # noqa: E731


def _oracle64(kind, c):
    fit = O.affine_fit if kind == "affine" else O.rigid_fit
    w = None if c["w"] is None else T64(c["w"])[None]
    return fit(T64(c["x"])[None], T64(c["y"])[None], w)[0].numpy()


def test_restatement_equals_oracle_fp64():
    """on the well-conditioned cases (no offset, no one_heavy weighting, not the near-coplanar cloud) the restatement equals the
    oracle in fp64 to 1e-12: rigid everywhere (measured <= 2e-15), the affine normal equations (<= 1e-14) and lstsq (<= 6e-14)"""
    worst = {"rigid": 0.0, "normal": 0.0, "lstsq": 0.0}
    for c in CASES:
        if "offset" in c["name"] or "one_heavy" in c["name"] or "near_coplanar" in c["name"]:
            continue
        x, y, w = c["x"], c["y"], c["w"]
        worst["rigid"] = max(worst["rigid"], np.abs(R.rigid_fit(x, y, w) - _oracle64("rigid", c)).max())
        ref = _oracle64("affine", c)
        worst["normal"] = max(worst["normal"], np.abs(R.affine_fit_normal(x, y, w) - ref).max())
        worst["lstsq"] = max(worst["lstsq"], np.abs(R.affine_fit(x, y, w) - ref).max())
    print(worst)
    assert max(worst.values()) <= 1e-12, worst


def test_small_ops_equal_oracle_fp64():
    rng = np.random.default_rng(0)
    for _, M in R.inverse_cases()[:3]:
        ref = torch.inverse(O.square(T64(M)))[:, :3].numpy()
        for n in range(M.shape[0]):
            assert np.abs(R.affine_inverse(M[n]) - ref[n]).max() <= 1e-12 * np.abs(ref[n]).max()
    M, pts = R.points_cases()[3][1:]
    ref = O.matrix_transform_points(T64(M), T64(pts)).numpy()
    assert np.abs(R.affine_points(M[0], pts[0]) - ref[0]).max() <= 1e-14
    for content in R.COM_CONTENTS:
        f = R.com_volume((2, 3, 5, 1, 7), content)
        ft = T64(f).requires_grad_(True)
        out = O.center_of_mass(ft, "ij")
        cot = rng.standard_normal(out.shape)
        (out * T64(cot)).sum().backward()
        lin32 = lambda n: torch.linspace(0, 1, n).numpy()                   # noqa: E731  (the oracle's fp32 coordinates)
        assert np.abs(R.center_of_mass(f, lin32) - out.detach().numpy()).max() <= 1e-12, content
        assert np.abs(R.center_of_mass(f) - out.detach().numpy()).max() <= 1e-7, content
        g = R.center_of_mass_vjp(f, cot, lin32)
        assert np.abs(g - ft.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(g).max()), content
        assert (ft.grad.numpy()[f <= 0] == 0).all(), content                # F.relu: nothing at exact zeros


def test_analytic_adjoints_equal_autograd_fp64():
    """the hand-written adjoints of the restatement (affine fit, inverse, points) against fp64 autograd"""
    cot = R.cotangent(2)
    for name in ("K63_generic-none", "K64_generic-quarter_zero", "K50_reflection-sum3"):
        c = BY_NAME[name]
        ref = R.oracle_vjp("affine", c["x"], c["y"], c["w"], cot)[1]
        got = R.affine_fit_vjp(c["x"], c["y"], c["w"], cot)
        for g, r in zip(got, ref):
            if r is not None:
                assert np.abs(g - r).max() <= 1e-12 * max(1.0, np.abs(r).max()), name
    M = R.inverse_cases()[1][1][0]
    Mt = T64(M)[None].requires_grad_(True)
    (torch.inverse(O.square(Mt))[0, :3] * T64(cot)).sum().backward()
    assert np.abs(R.affine_inverse_vjp(M, cot) - Mt.grad[0].numpy()).max() <= 1e-10 * Mt.grad.abs().max().item()
    _, M, pts = R.points_cases()[2]
    cp = R.cotangent(3, pts[0].shape)
    Mt, pt = T64(M[:1]).requires_grad_(True), T64(pts[:1]).requires_grad_(True)
    (O.matrix_transform_points(Mt, pt)[0] * T64(cp)).sum().backward()
    dM, dp = R.affine_points_vjp(M[0], pts[0], cp)
    assert np.abs(dM - Mt.grad[0].numpy()).max() <= 1e-12 and np.abs(dp - pt.grad[0].numpy()).max() <= 1e-14


@pytest.mark.parametrize("name", ["K50_reflection-none", "K63_generic-normalised", "K5_generic-sum3", "cube_jitter-none"])
def test_vjp_fd_equals_autograd_where_finite(name):
    """central differences of the restatement agree with fp64 autograd of the oracle's rigid fit where the singular values are
    apart (a generic case, a reflection, a tiny K, the jittered cube whose autograd divides by a 1e-3 gap): measured
    5e-10 .. 2e-9 on gradients of size ~1, the same size as the two-step-size uncertainty"""
    c = BY_NAME[name]
    cot = R.cotangent(4)
    ref = R.oracle_vjp("rigid", c["x"], c["y"], c["w"], cot)[1]
    got, unc = R.vjp_fd(R.rigid_fit, (c["x"], c["y"], c["w"]), cot)
    for g, r, u in zip(got, ref, unc):
        if r is not None:
            err = np.abs(g - r).max()
            print(name, err, u)
            assert np.isfinite(r).all() and err <= 1e-6 * np.abs(r).max() and u <= 1e-6 * np.abs(r).max()


SYMMETRIC = [c["name"] for c in CASES if c["grad"] == "fd"]


@pytest.mark.parametrize("name", SYMMETRIC)
def test_symmetric_clouds_need_finite_differences(name):
    """the stated reason the exactly symmetric clouds use vjp_fd: with two or three equal singular values fp64 autograd of the
    oracle's rigid fit is not finite (torch.linalg.svd's backward divides by s_i^2 - s_j^2), while the fit itself is smooth
    there: central differences are finite and their two step sizes agree to 1e-7 relative"""
    c = BY_NAME[name]
    cot = R.cotangent(5)
    _, s, _ = R.rigid_fit(c["x"], c["y"], c["w"], full=True)
    assert abs(s[0] - s[1]) <= 1e-12 * s[0]
    auto = R.oracle_vjp("rigid", c["x"], c["y"], c["w"], cot)[1]
    assert not np.isfinite(auto[0]).all()
    got, unc = R.vjp_fd(R.rigid_fit, (c["x"], c["y"], c["w"]), cot)
    for g, u in zip(got, unc):
        if g is not None:
            assert np.isfinite(g).all() and np.abs(g).max() > 1e-2 and u <= 1e-7 * np.abs(g).max(), (name, u)


def test_fp32_oracle_is_no_yardstick_at_offset_100():
    """real-world coordinates: the fp32 oracle's affine fit at offset 100 misses the fp64 truth by more than 1e-2 (measured
    2.5 and 2.7), while the fp64 normal equations stay within 1e-8 of lstsq"""
    for name in ("K50_offset100-none", "K300_offset100-normalised"):
        c = BY_NAME[name]
        truth = R.affine_fit(c["x"], c["y"], c["w"])
        w = None if c["w"] is None else torch.from_numpy(c["w"])[None]
        m32 = O.affine_fit(torch.from_numpy(c["x"])[None], torch.from_numpy(c["y"])[None], w)[0].numpy()
        print(name, np.abs(m32 - truth).max())
        assert np.abs(m32 - truth).max() > 1e-2
        assert np.abs(R.affine_fit_normal(c["x"], c["y"], c["w"]) - truth).max() <= 1e-7


def test_fp64_autograd_is_no_yardstick_for_affine_dw_at_an_offset():
    """why the truth of the affine gradients is the long double adjoint and not fp64 autograd of the oracle: at offset 1000 the
    oracle's dw, all cancellation, misses the long double value by 16 of a maximum of 940 (2e-2 relative; up to 85 of 1900
    over the table), 800 times the fp64 adjoint's 2e-2 -- and the kernel evaluates that adjoint"""
    c = BY_NAME["K50_offset1000-normalised"]
    cot = R.cotangent(6)
    hi = R.affine_fit_vjp(c["x"], c["y"], c["w"], cot, np.longdouble)[2]
    lo = R.affine_fit_vjp(c["x"], c["y"], c["w"], cot)[2]
    auto = R.oracle_vjp("affine", c["x"], c["y"], c["w"], cot)[1][2]
    e_auto, e_lo = float(np.abs(auto - hi).max()), float(np.abs(lo - hi).max())
    print(e_auto, e_lo, float(np.abs(hi).max()))
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:          # (a platform whose long double is fp64 measures nothing)
        assert e_auto > 1e-3 * float(np.abs(hi).max()) and e_auto > 30 * e_lo


def _class_a(name, x, y, w, kinds):
    if "rigid" in kinds:
        _, s, det0 = R.rigid_fit(x, y, w, full=True)
        assert s[2] / s[0] >= 1e-3, (name, s)
        if "reflection" in name:
            assert det0 < 0, name
    if "affine" in kinds:
        cond = np.linalg.cond(R.affine_normal_matrix(x, w))
        assert cond <= R.affine_cond_limit(name), (name, cond)
        assert np.abs(R.affine_fit_normal(x, y, w) - R.affine_fit(x, y, w)).max() <= (1e-4 if "offset1000" in name else 1e-7)


def test_every_case_sits_in_its_class():
    """a later edit of a seed cannot quietly move a case out of its regime"""
    assert len({c["name"] for c in CASES}) == len(CASES)
    for c in CASES:
        assert c["cls"] == "A" and c["kinds"]
        _class_a(c["name"], c["x"], c["y"], c["w"], c["kinds"])
        if c["w"] is not None:
            tot = float(c["w"].astype(np.float64).sum())
            want = {"sum0.5": 0.5, "sum3": 3.0}.get(c["name"].split("-")[1], 1.0)
            assert abs(tot - want) <= 1e-6 * want, c["name"]
            if "quarter_zero" in c["name"]:
                assert (c["w"] == 0).sum() == len(c["w"]) // 4
            if "one_heavy" in c["name"]:
                assert np.isclose(c["w"].max(), 0.97)
    # the tetrahedron interpolates: the affine residual is zero
    c = BY_NAME["K4_tetrahedron-none"]
    assert np.abs(R.affine_points(R.affine_fit(c["x"], c["y"]), c["x"]) - c["y"]).max() <= 1e-14
    x, y, w, modes, names = R.batch_case()
    assert x.shape == (37, 64, 3) and w.shape == (37, 64)
    for n in range(37):
        _class_a(names[n], x[n], y[n], w[n], ("affine", "rigid"))
        s = R.rigid_fit(x[n], y[n], w[n], full=True)[1]
        assert (modes[n] == "fd") == (abs(s[0] - s[1]) <= 1e-12 * s[0]), names[n]
    for c in R.property_cases():
        s = R.rigid_fit(c["x"], c["y"], c["w"], full=True)[1]
        if c["cls"] == "B":
            assert s[1] >= 1e-3 * s[0] and s[2] <= 1e-12 * s[0], (c["name"], s)
        else:
            assert c["cls"] == "C" and (s[0] == 0 or s[1] <= 1e-12 * s[0]), (c["name"], s)
