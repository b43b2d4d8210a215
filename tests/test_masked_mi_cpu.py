"""CPU: the masked restatement (tests/masked_mi_ref.py) against the unmasked one, the inputs of the masked drivers' GPU tests
validated on the restatement alone, and the masked entry points' argument checks (they return before any launch)."""
import ctypes

import pytest
import torch

from tests import masked_mi_ref as R
from tests import mi_ref
from tests import warp_mi_ref as W

F64 = torch.float64


def _pair(shape=(2, 1, 6, 7, 9), seed=4):
    a, b = mi_ref.smooth_pair(shape, seed)
    return a.to(F64), b.to(F64)


def test_a_mask_of_ones_is_the_unmasked_restatement():
    a, b = _pair()
    ones = torch.ones(a.shape, dtype=torch.uint8)
    assert torch.allclose(R.mutual_information(a, b, ones), mi_ref.mutual_information(a, b), rtol=0, atol=1e-14)
    mi, da, db = R.evaluate(a.float(), b.float(), ones)
    mi0, da0, db0 = mi_ref.evaluate(a.float(), b.float())
    assert torch.allclose(mi, mi0, rtol=0, atol=1e-14)
    assert torch.allclose(da, da0, rtol=0, atol=1e-15) and torch.allclose(db, db0, rtol=0, atol=1e-15)


def test_masked_equals_the_compacted_voxel_list():
    a, b = _pair()
    g = torch.Generator().manual_seed(0)
    mask = torch.rand(a.shape, generator=g) < 0.4
    rng = W.own_ranges(a, b)
    got = R.mutual_information(a, b, mask, 32, rng)
    for n in range(a.shape[0]):
        want = mi_ref.mi_sample(a[n][mask[n]], b[n][mask[n]], 32, rng[n][0], rng[n][1])
        assert abs(float(got[n]) - float(want)) <= 1e-14 and float(want) > 0
    # no counted voxel: exactly nothing
    mi, da, db = R.evaluate(a.float(), b.float(), torch.zeros(a.shape, dtype=torch.uint8))
    assert not mi.any() and not da.any() and not db.any()
    # a voxel that is not counted has no gradient
    _, da, db = R.evaluate(a.float(), b.float(), mask)
    assert not da[~mask].any() and not db[~mask].any() and da[mask].abs().max() > 0


def test_counted_set_of_the_chain():
    """The three factors on a grid whose answers are known: an integer shift along x."""
    dims = (4, 5, 8)
    mat = W.voxel_to_mat(torch.eye(3, dtype=F64)[None], torch.tensor([[0.0, 0.0, 3.0]], dtype=F64), dims)
    grid = W.grid_of(mat, dims)
    assert bool(R.counted(grid).all())
    inside = R.counted(grid, inside=True)[0, 0]
    assert bool(inside[..., :5].all()) and not bool(inside[..., 5:].any())          # x + 3 > 7 leaves the volume
    mm = torch.zeros((1, 1, *dims), dtype=torch.uint8)
    mm[..., 4] = 1                                                                  # moving voxel x = 4 <- fixed voxel x = 1
    c = R.counted(grid, moving_mask=mm)[0, 0]
    assert bool(c[..., 1].all()) and int(c.sum()) == 4 * 5
    mm[..., 7] = 1                                                                  # the border clamp replicates x = 7 ...
    assert int(R.counted(grid, moving_mask=mm).sum()) == 4 * 5 * 5
    assert int(R.counted(grid, moving_mask=mm, inside=True).sum()) == 4 * 5 * 2     # ... and `inside` drops the copies
    fm = torch.zeros((1, 1, *dims), dtype=torch.uint8)
    fm[:, :, 2] = 1
    assert int(R.counted(grid, fm, mm, True).sum()) == 5 * 2


def _mi_at(f64, m64, L, t, ranges, mask):
    mat = W.voxel_to_mat(L, t, f64.shape[2:])
    if mask is None:
        return float(W.warp_mi(m64, f64, mat, 32, ranges)[0])
    return float(R.warp_mi(m64, f64, mat, 32, ranges, mask, mask)[0])


def test_stationary_structure_pair():
    """What makes the masked driver test more than luck, on the restatement alone (test_warp_mi_cpu.py's _assert_peak): with the
    masks the true motion beats every +-1 voxel-equivalent perturbation of the six rigid parameters; without them it does not."""
    fixed, moving, L, t, mask = R.slab_pair(32)
    assert fixed.shape == moving.shape == mask.shape == (1, 1, 32, 32, 32)
    assert float(fixed[mask == 0].min()) >= 0 and 0 < int((mask == 0).sum()) < mask.numel() // 3
    assert not bool(mask[0, 0, R.SLAB_Z[0] - 1:R.SLAB_Z[1] + 1].any()) and bool(mask[0, 0, R.SLAB_Z[1] + 1:].all())
    f64, m64 = fixed.to(F64), moving.to(F64)
    ranges = W.own_ranges(moving, fixed)
    h = (fixed.shape[2] - 1) / 2
    for which, msk in (("masked", mask), ("unmasked", None)):
        top = _mi_at(f64, m64, L, t, ranges, msk)
        others = {"identity": _mi_at(f64, m64, torch.eye(3, dtype=F64)[None], torch.zeros(1, 3, dtype=F64), ranges, msk)}
        for k in range(3):
            for sgn in (1.0, -1.0):
                e = [0.0, 0.0, 0.0]
                e[k] = sgn
                others[f"shift {k} {sgn:+.0f}"] = _mi_at(f64, m64, L, t + torch.tensor([e], dtype=F64), ranges, msk)
                others[f"turn {k} {sgn:+.0f}"] = _mi_at(f64, m64, (W.rotation([v / h for v in e]) @ L[0])[None], t, ranges, msk)
        best = max(others, key=others.get)
        print(f"{which}: MI true {top:.5f}  best other: {best} {others[best]:.5f}")
        if msk is not None:
            assert top > others[best]
        else:
            assert others[best] > top


def test_masked_entry_points_refuse_bad_arguments():
    from keymorph_amd import _lib, build
    import os
    if not os.path.exists(build.LIBPATH):
        build.build()
    lib = _lib.load()
    x = ctypes.c_void_p(64)                # a non-null address: every call below returns before anything reads it
    for N, V, bins in ((0, 100, 32), (1, 0, 32), (1, 100, 7), (1, 100, 65), (70000, 100, 32)):
        assert lib.kmh_mi_hist_masked(x, x, x, x, N, V, bins, x, x, None) == -22
        assert lib.kmh_mi_bwd_masked(x, x, x, x, x, x, x, N, V, bins, x, x, None) == -22
    assert lib.kmh_mi_hist_masked(x, x, None, x, 1, 100, 32, x, None, None) == -22          # no count
    assert lib.kmh_mi_hist_masked(None, x, None, x, 1, 100, 32, x, x, None) == -22
    assert lib.kmh_mi_final_masked(x, x, None, 1, 32, x, x, None) == -22
    assert lib.kmh_mi_final_masked(x, x, x, 1, 66, x, x, None) == -22
    assert lib.kmh_mi_bwd_masked(x, x, None, x, x, x, None, 1, 100, 32, x, x, None) == -22
    for D, H, Wd, bins in ((16, 16, 1, 32), (16, 16, 16, 7), (16, 16, 16, 65), (1024, 1024, 1024, 32), (0, 16, 16, 32)):
        assert lib.kmh_warp_mi_hist_masked(x, x, None, None, x, x, 1, D, H, Wd, bins, 0, x, x, None) == -22
        assert lib.kmh_warp_mi_bwd_masked(x, x, None, None, x, x, x, x, x, 1, D, H, Wd, bins, 1, x, x, None) == -22
    assert lib.kmh_warp_mi_hist_masked(x, x, x, x, x, x, 1, 16, 16, 16, 32, 1, x, None, None) == -22
    assert lib.kmh_warp_mi_bwd_masked(x, x, x, x, x, x, x, x, None, 1, 16, 16, 16, 32, 1, x, x, None) == -22
    assert lib.kmh_warp_mi_bwd_masked(x, x, x, x, x, x, x, x, x, 1, 16, 16, 16, 32, 1, x, None, None) == -22
