"""CPU: tests/golden/lc2.npz (the reference's LC2 / ImageLC2, keymorph/loss_ops.py:250-391, under its own fp32 autograd) against
an fp64 restatement of run() written here, and the derivative conventions csrc/lc2.hip implements, pinned from torch's autograd.
The input recipe, the case table and the restatement are shared with tests/test_lc2_gpu.py and tools/make_golden_lc2.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import golden

ALPHA, BETA = 1e-3, 1e-2

# name -> inputs (seed, N, S, one kind per sample), module (patch None = LC2 on the whole volume), radii
CASES = {
    "lc2_s15": dict(seed=1, N=2, S=15, kinds=("flat", "plain"), patch=None, radii=(2, 4, 6)),
    "lc2_s17": dict(seed=2, N=2, S=17, kinds=("plain", "sat"), patch=None, radii=(3, 5, 7)),
    "img102": dict(seed=3, N=1, S=102, kinds=("img102",), patch=51, radii=(5,)),
    "img110": dict(seed=4, N=1, S=110, kinds=("img110",), patch=51, radii=(3, 5)),
}


def lc2_pair(seed, N, S, kinds):
    """float32 (N, 1, S, S, S) numpy arrays (us, mr), identical on every machine: integer draws, 3x3x3 box sums in int64, and
    correctly rounded float64 operations before one rounding to float32.  Kinds: "plain"; "flat" (a zero block, g = 0 inside
    it, crossing the crops); "sat" (us unrelated to mr on a large offset: the raw value is negative and clamp(0, 1) saturates);
    "img102" (patch (0, 0, 0) low contrast, var < beta; a zero block across patch (1, 1, 1)'s crop); "img110" (patch (1, 1, 0)
    saturated, a zero block across several crops)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 16, (N, S + 2, S + 2, S + 2))
    box = sum(k[:, a:a + S, b:b + S, c:c + S] for a in range(3) for b in range(3) for c in range(3))
    mr = (box - 202.0) / 81.0
    noise = rng.integers(0, 64, (N, S, S, S)) / 64.0
    us = 0.6 * (mr * mr) + 0.4 * mr + 0.3 * (noise - 0.5)
    for i, kind in enumerate(kinds):
        if kind == "flat":
            mr[i, : S // 2, :, : S // 2] = 0.0
            us[i, : S // 2, :, : S // 2] = 0.0
        elif kind == "sat":
            us[i] = 6.0 + noise[i]
        elif kind == "img102":
            us[i, :51, :51, :51] = 0.05 * us[i, :51, :51, :51]
            mr[i, 40:80, 51:, 51:] = 0.0
            us[i, 40:80, 51:, 51:] = 0.0
        elif kind == "img110":
            us[i, 51:102, 51:102, :51] = 6.0 + noise[i, 51:102, 51:102, :51]
            mr[i, :, :60, 60:80] = 0.0
    return us.astype(np.float32)[:, None], mr.astype(np.float32)[:, None]


def case_inputs(name):
    c = CASES[name]
    return lc2_pair(c["seed"], c["N"], c["S"], c["kinds"])


def patch_of(name):
    c = CASES[name]
    return c["S"] if c["patch"] is None else c["patch"]


def difference_filter(dtype=torch.float64):
    f = torch.zeros(3, 1, 3, 3, 3, dtype=dtype)
    for k, (dz, dy, dx) in enumerate(((0, 0, 1), (0, 1, 0), (1, 0, 0))):
        f[k, 0, 1 - dz, 1 - dy, 1 - dx] = 1
        f[k, 0, 1 + dz, 1 + dy, 1 + dx] = -1
    return f


def lc2_fp64(us, mr, patch, radii, alpha=ALPHA, beta=BETA):
    """(N, 1, S, S, S) float64 tensors -> (B,) per-patch mean over `radii` of the reference's run(), restated in fp64 with
    torch ops (autograd-able): patches in (n, pz, py, px) order, the remainder dropped."""
    N, S = us.shape[0], us.shape[-1]
    nP = S // patch
    L = nP * patch

    def tiles(x):
        x = x[:, 0, :L, :L, :L].reshape(N, nP, patch, nP, patch, nP, patch)
        return x.permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, patch, patch, patch)

    u, m = tiles(us), tiles(mr)
    B = u.shape[0]
    g = torch.linalg.vector_norm(F.conv3d(m[:, None], difference_filter(m.dtype), padding=1), dim=1)
    out = 0
    for r in radii:
        w = 2 * r + 1
        pad = (patch - w) // 2
        sl = slice(pad, pad + w)
        n = w ** 3
        A = torch.stack([m[:, sl, sl, sl].reshape(B, n), g[:, sl, sl, sl].reshape(B, n),
                         torch.ones(B, n, dtype=m.dtype)], 1)
        b = u[:, sl, sl, sl].reshape(B, n)
        C = A @ A.transpose(1, 2) / n + alpha * torch.eye(3, dtype=m.dtype)
        Atb = (A @ b[..., None])[..., 0] / n
        c = torch.linalg.solve(C, Atb)
        var = (b * b).mean(1) - b.mean(1) ** 2
        dist = (b * b).mean(1) + torch.einsum("bi,bij,bj->b", c, C, c) - 2 * (c * Atb).sum(1)
        out = out + ((var - dist) / var.clamp_min(beta)).clamp(0, 1)
    return out / len(radii)


def fp64_case(name):
    """fp64 restatement of a case: forward (B,) per patch, and both input gradients of the module's output (LC2: the sum of
    the per-sample values; ImageLC2: the mean over the patches)."""
    us, mr = case_inputs(name)
    u = torch.tensor(us, dtype=torch.float64, requires_grad=True)
    m = torch.tensor(mr, dtype=torch.float64, requires_grad=True)
    per = lc2_fp64(u, m, patch_of(name), CASES[name]["radii"])
    (per.sum() if CASES[name]["patch"] is None else per.mean()).backward()
    return per.detach(), u.grad, m.grad


def halo_boxes(name):
    """Per patch, the slices (z, y, x) of the bounding box of the largest crop plus its 1-voxel halo."""
    c = CASES[name]
    P, S = patch_of(name), c["S"]
    w = 2 * max(c["radii"]) + 1
    lo = (P - w) // 2 - 1
    nP = S // P
    out = []
    for n in range(c["N"]):
        for pz in range(nP):
            for py in range(nP):
                for px in range(nP):
                    out.append((n, slice(pz * P + lo, pz * P + lo + w + 2), slice(py * P + lo, py * P + lo + w + 2),
                                slice(px * P + lo, px * P + lo + w + 2)))
    return out


def boxed(grad, name):
    """(N, 1, S, S, S) -> (B, L, L, L): the halo boxes of every patch."""
    g = np.asarray(grad)
    return np.stack([g[n, 0, z, y, x] for n, z, y, x in halo_boxes(name)])


def support_mask(name):
    """(N, 1, S, S, S) bool: the voxels a gradient may reach, every crop plus its face neighbours (its 1-voxel halo without
    edges and corners)."""
    c = CASES[name]
    P, S = patch_of(name), c["S"]
    nP = S // P
    m = np.zeros((c["N"], 1, S, S, S), bool)
    for r in c["radii"]:
        w = 2 * r + 1
        pad = (P - w) // 2
        for pz in range(nP):
            for py in range(nP):
                for px in range(nP):
                    z0, y0, x0 = pz * P + pad, py * P + pad, px * P + pad
                    for ax in range(3):
                        lo = [z0, y0, x0]
                        hi = [z0 + w, y0 + w, x0 + w]
                        lo[ax] -= 1
                        hi[ax] += 1
                        m[:, 0, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    return m


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---------------------------------------------------------------- conventions (torch autograd = the reference's)
def test_norm_gradient_is_zero_where_all_differences_vanish():
    d = torch.zeros(1, 3, 4, dtype=torch.float64, requires_grad=True)
    torch.norm(d, dim=1).sum().backward()
    assert torch.equal(d.grad, torch.zeros_like(d))


def test_clamp_min_passes_at_and_above_beta_only():
    v = torch.tensor([0.5 * BETA, BETA, 2 * BETA], dtype=torch.float64, requires_grad=True)
    v.clamp_min(BETA).sum().backward()
    assert v.grad.tolist() == [0.0, 1.0, 1.0]


def test_clamp_passes_inside_its_bounds_included():
    v = torch.tensor([-0.1, 0.0, 0.5, 1.0, 1.1], dtype=torch.float64, requires_grad=True)
    v.clamp(0, 1).sum().backward()
    assert v.grad.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]


# ---------------------------------------------------------------- the fixture against the fp64 restatement
@pytest.mark.parametrize("name", list(CASES))
def test_fixture_matches_fp64_restatement(name):
    g = golden("lc2.npz")
    per, du, dm = fp64_case(name)
    if CASES[name]["patch"] is None:
        np.testing.assert_allclose(g[f"{name}::fwd"], per.numpy(), atol=1e-5, rtol=0)
        ref_du, ref_dm, du, dm = g[f"{name}::dus"], g[f"{name}::dmr"], du.numpy(), dm.numpy()
    else:
        np.testing.assert_allclose(g[f"{name}::fwd_none"], per.numpy(), atol=1e-5, rtol=0)
        assert abs(float(g[f"{name}::fwd_mean"]) - float(per.mean())) <= 1e-5
        ref_du, ref_dm, du, dm = g[f"{name}::dus_box"], g[f"{name}::dmr_box"], boxed(du, name), boxed(dm, name)
    assert rel_l2(du, ref_du) < 1e-4 and rel_l2(dm, ref_dm) < 1e-4
    assert np.array_equal(ref_du == 0, du == 0) and np.array_equal(ref_dm == 0, dm == 0)


def test_cases_cover_the_edge_cases():
    """The fixture holds a saturated clamp (value 0, gradient exactly 0), a low-contrast patch (var < beta) that still has a
    gradient, and voxels where g = 0 next to a crop."""
    g = golden("lc2.npz")
    assert g["lc2_s17::fwd"][1] == 0 and not g["lc2_s17::dus"][1].any() and not g["lc2_s17::dmr"][1].any()
    sat = (1 * 2 + 1) * 2 + 0                                  # img110 patch (1, 1, 0)
    assert g["img110::fwd_none"][sat] == 0 and not g["img110::dus_box"][sat].any()
    us, _ = case_inputs("img102")
    crop = us[0, 0, 20:31, 20:31, 20:31].astype(np.float64)
    assert crop.var() < BETA and g["img102::fwd_none"][0] > 0 and g["img102::dus_box"][0].any()
    _, mr = case_inputs("lc2_s15")
    assert (mr[0, 0, 1:6, 1:6, 1:6] == 0).all()             # inside the zero block: g = 0


def test_support_is_the_crops_and_their_face_halos():
    g = golden("lc2.npz")
    for name in ("lc2_s15", "lc2_s17"):
        outside = ~support_mask(name)
        assert not g[f"{name}::dus"][outside].any() and not g[f"{name}::dmr"][outside].any()


def test_cpu_tensors_raise():
    from keymorph_amd._lib import KeymorphHipError
    from keymorph_amd.loss_ops import LC2, ImageLC2
    x = torch.zeros(1, 1, 17, 17, 17)
    with pytest.raises(KeymorphHipError):
        LC2()(x, x)
    with pytest.raises(KeymorphHipError):
        ImageLC2(patch_size=17, radiuses=(3,))(x, x)


def test_reference_attributes():
    from keymorph_amd.loss_ops import LC2, ImageLC2
    a, b = LC2(), ImageLC2()
    assert a.radiuses == (3, 5, 7) and b.patch_size == 51 and b.radii == (5,) and b.reduction == "mean"
    assert torch.equal(a.f, difference_filter(torch.float32)) and torch.equal(b.f, a.f)
    assert ImageLC2(reduction=None).reduction is None
    with pytest.raises(AssertionError):
        ImageLC2(reduction="sum")
