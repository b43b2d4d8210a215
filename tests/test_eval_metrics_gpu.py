"""GPU: hausdorff_distance, fast_dice and dice (csrc/metrics.hip) against the reference's values in
tests/golden/eval_metrics.npz (bit for bit), a numpy brute force of the distance map, and the pairwise / groupwise wiring."""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

from tests.test_eval_metrics_cpu import REF_SAMPLING, brute_sq_map, hd_case, surface
from tests.util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = ["blobs", "odd_37x64x23", "flat_1x40x33", "thin", "faces", "rot96"]


def G():
    return golden("eval_metrics.npz")


def soft(m, seed):
    """float32 (bs, 2, D, H, W) with channel 0 nonzero exactly on m: soft values, 1e-30 and NaN inside, -0.0 outside."""
    rng = np.random.default_rng(seed)
    v = np.where(m, rng.uniform(0.01, 1.0, m.shape), 0.0).astype(np.float32)
    idx = np.argwhere(m)
    for j, val in zip(range(0, len(idx), max(1, len(idx) // 7)), (1e-30, np.nan, -2.5, 1e-30, np.nan, 3e38, 1e-30)):
        v[tuple(idx[j])] = val
    v[~m] = np.where(rng.random(int((~m).sum())) < 0.5, -0.0, 0.0)
    return np.stack([v, rng.random(m.shape).astype(np.float32)], 1)


def param_volume(shape, boxes, ellipsoids):
    """tests/test_eval_metrics_cpu.py::param_volume_np on the GPU (int64: exact)."""
    D, H, W = shape
    m = torch.zeros(shape, dtype=torch.bool, device=DEV)
    for z0, z1, y0, y1, x0, x1 in boxes.tolist():
        m[z0:z1, y0:y1, x0:x1] = True
    z = torch.arange(D, device=DEV).view(-1, 1, 1)
    y = torch.arange(H, device=DEV).view(1, -1, 1)
    x = torch.arange(W, device=DEV).view(1, 1, -1)
    for cz, cy, cx, rz, ry, rx in ellipsoids.tolist():
        q = (z - cz) ** 2 * (ry * rx) ** 2 + (y - cy) ** 2 * (rz * rx) ** 2 + (x - cx) ** 2 * (rz * ry) ** 2
        m |= q <= (rz * ry * rx) ** 2
    return m


@pytest.mark.parametrize("name", SMALL)
def test_hausdorff_equals_reference(name):
    from keymorph_amd.loss_ops import hausdorff_distance
    a, b, ref = hd_case(G(), name)
    fa, fb = soft(a, 1), soft(b, 2)
    assert hausdorff_distance(torch.tensor(fa, device=DEV), torch.tensor(fb, device=DEV)) == ref   # float32, soft, strided
    assert hausdorff_distance(fa, fb) == ref                                                      # numpy
    assert hausdorff_distance(torch.tensor(fa), torch.tensor(fb)) == ref                          # CPU tensors
    ta, tb = torch.tensor(a[:, None], device=DEV), torch.tensor(b[:, None], device=DEV)
    assert hausdorff_distance(ta, tb) == ref                                                      # bool
    assert hausdorff_distance(ta.to(torch.uint8), tb.to(torch.uint8)) == ref                      # uint8
    assert hausdorff_distance(ta.double() * 0.5, tb.to(torch.int32) * 3) == ref                   # mixed dtypes
    assert hausdorff_distance(ta.half(), tb.to(torch.bfloat16)) == ref


def test_hausdorff_reference_warped_soft_segmentations():
    from keymorph_amd.loss_ops import hausdorff_distance
    g, ge = G(), golden("groupwise_eval_tiny.npz")
    for key, ref in (("affine::seg_a_1", "seg_0"), ("tps_1::seg_a_1", "seg_2")):
        want = float(g[f"hdsoft::{key}::{ref}"])
        assert hausdorff_distance(torch.tensor(ge[key], device=DEV), torch.tensor(ge[ref], device=DEV).float()) == want
        assert hausdorff_distance(ge[key], ge[ref]) == want


@pytest.mark.parametrize("name", ["boxes256", "brain256"])
def test_hausdorff_256_equals_reference(name):
    from keymorph_amd.loss_ops import hausdorff_distance
    g = G()
    A = param_volume((256, 256, 256), g[f"big::{name}::boxes_a"], g[f"big::{name}::ell_a"])
    B = param_volume((256, 256, 256), g[f"big::{name}::boxes_b"], g[f"big::{name}::ell_b"])
    a, b = A[None, None].float(), B[None, None].float()
    hausdorff_distance(a, b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = hausdorff_distance(a, b)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"{name}: hausdorff_distance 256^3 {ms:.2f} ms (host clock, incl. the result copy)")
    assert got == float(g[f"big::{name}::value"])
    assert hausdorff_distance(a, b) == got                         # deterministic


@pytest.mark.parametrize("sampling,ulps", [(REF_SAMPLING, 0), ((1.0, 1.0, 1.0), 0), ((0.7, 1.3, 2.9), 2)])
def test_distance_map_vs_brute_force(sampling, ulps):
    from keymorph_amd.loss_ops import surface_distance_map_sq
    rng = np.random.default_rng(7)
    for shape in [(24, 24, 24), (13, 7, 21), (1, 9, 17), (5, 1, 3), (2, 3, 1), (19, 24, 11)]:
        m = rng.random(shape) < rng.choice([0.05, 0.3, 0.7])
        got = surface_distance_map_sq(torch.tensor(m, device=DEV), sampling).cpu().numpy()
        ref = brute_sq_map(m, sampling)
        assert np.array_equal(np.isinf(got), np.isinf(ref)), shape
        fin = np.isfinite(ref)
        if ulps == 0:
            assert np.array_equal(got[fin], ref[fin]), shape
        else:
            g, r = np.sqrt(got[fin]), np.sqrt(ref[fin])
            assert (np.abs(g - r) <= ulps * np.spacing(r)).all(), (shape, np.abs(g - r).max())


def test_hausdorff_non_dyadic_sampling_within_2ulp():
    from keymorph_amd.loss_ops import hausdorff_distance
    rng = np.random.default_rng(11)
    samp = (0.7, 1.3, 2.9)
    for shape in [(17, 20, 23), (1, 15, 30)]:
        a, b = rng.random(shape) < 0.4, rng.random(shape) < 0.2
        sa, sb = np.argwhere(surface(a)), np.argwhere(surface(b))
        from tests.test_eval_metrics_cpu import min_sq_dist
        ref = math.sqrt(max(min_sq_dist(sb, sa, samp).max(), min_sq_dist(sa, sb, samp).max()))
        got = hausdorff_distance(torch.tensor(a[None, None], device=DEV), torch.tensor(b[None, None], device=DEV), samp)
        assert abs(got - ref) <= 2 * np.spacing(ref)


def test_hausdorff_edge_cases():
    from keymorph_amd.loss_ops import hausdorff_distance
    z = torch.zeros(1, 1, 6, 7, 8, device=DEV)
    o = z.clone()
    o[0, 0, 2:4, 3:5, 1:6] = 1
    with pytest.raises(ValueError):
        hausdorff_distance(z, z)
    assert hausdorff_distance(z, o) == math.inf and hausdorff_distance(o, z) == math.inf
    assert hausdorff_distance(o, o) == 0.0
    with pytest.raises(ValueError):
        hausdorff_distance(o[0], o[0])
    # one sample of two empty: the batch raises, as the reference's max() does
    with pytest.raises(ValueError):
        hausdorff_distance(torch.cat([o, z]), torch.cat([o, z]))


def _fd_inputs(g, k):
    if k == "ties":
        return g["fd::ties::x"], g["fd::ties::y"]
    C = int(g[f"fd::{k}::C"])
    oh = lambda l: np.moveaxis(np.eye(C, dtype=np.float32)[l], -1, 1)       # noqa: E731
    return oh(g[f"fd::{k}::x"]), oh(g[f"fd::{k}::y"])


@pytest.mark.parametrize("k", ["onehot", "ties", "single"])
def test_fast_dice_equals_reference(k):
    from keymorph_amd.loss_ops import fast_dice
    g = G()
    x, y = _fd_inputs(g, k)
    ref = float(g[f"fd::{k}::value"])
    assert fast_dice(torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)) == ref
    assert fast_dice(x, y) == ref
    assert fast_dice(torch.tensor(x, device=DEV).double(), torch.tensor(y, device=DEV).double()) == ref


def test_dice_equals_reference():
    from keymorph_amd.loss_ops import dice
    g = G()
    x, y = g["dice::rand::x"], g["dice::rand::y"]
    ref = float(g["dice::rand::value"])
    assert dice(torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)) == ref
    assert dice(x.astype(bool), y.astype(bool)) == ref
    assert dice(torch.tensor(x, device=DEV).float(), torch.tensor(y).float()) == ref
    assert math.isnan(dice(np.zeros((3, 4)), np.zeros((3, 4))))


def test_pairwise_metrics_over_files(tmp_path):
    from keymorph_amd.loss_ops import DiceLoss, HausdorffPairwiseLoss, MultipleAvgSegPairwiseMetric, fast_dice, \
        hausdorff_distance
    rng = np.random.default_rng(3)
    lab = [rng.integers(0, 4, (1, 14, 12, 16)) for _ in range(3)]
    for l in lab:
        l[0, 3:11, 2:10, 4:12] = 0
    segs = [np.moveaxis(np.eye(4, dtype=np.float32)[l], -1, 1) for l in lab]
    paths = []
    for i, s in enumerate(segs):
        paths.append(str(tmp_path / f"seg_{i}.npy"))
        np.save(paths[-1], s)
    got = MultipleAvgSegPairwiseMetric()(paths, ["dice", "hausd", "harddice"])
    t = [torch.tensor(s, device=DEV) for s in segs]
    pairs = [(0, 1), (0, 2), (1, 2)]
    want_d = sum(fast_dice(t[i], t[j]) for i, j in pairs) / 3
    want_h = sum(hausdorff_distance(t[i], t[j]) for i, j in pairs) / 3
    want_hd = sum(DiceLoss(hard=True)(t[i], t[j]) for i, j in pairs) / 3
    assert got["dice"] == want_d and got["hausd"] == want_h
    assert float(got["harddice"]) == float(want_hd)
    assert HausdorffPairwiseLoss()(paths) == want_h
    assert HausdorffPairwiseLoss()(torch.cat(t)) == want_h


def test_evaluate_group_reports_hausd(tmp_path):
    from keymorph_amd.io import evaluate_group
    from keymorph_amd.loss_ops import MultipleAvgSegPairwiseMetric
    from tests.test_e2e_gpu import make_model
    from tests.util import seeded_state_dict, unet_shapes
    g, ge = golden("groupwise_tiny.npz"), golden("groupwise_eval_tiny.npz")
    km = make_model(16, seeded_state_dict(unet_shapes(16, 8, trunc=1), 200)).eval()
    os.makedirs(tmp_path / "img_m")
    os.makedirs(tmp_path / "seg_m")
    for i in range(3):
        np.savez(tmp_path / "img_m" / f"img_m_{i:03}.npz", img=g[f"img_{i}"])
        np.savez(tmp_path / "seg_m" / f"seg_m_{i:03}.npz", seg=ge[f"seg_{i}"].astype(np.float32))
    out = evaluate_group(km, tmp_path, ["affine"], DEV, metrics=("mse", "harddice", "hausd"), num_iters=2)
    got = json.load(open(tmp_path / "metrics-affine.json"))
    assert sorted(got) == ["harddice", "hausd", "mse"] and got == out["affine"]
    seg_a = sorted(str(tmp_path / "seg_a_affine" / f) for f in os.listdir(tmp_path / "seg_a_affine"))
    assert got["hausd"] == MultipleAvgSegPairwiseMetric()(seg_a, ["hausd"])["hausd"]
    assert math.isfinite(got["hausd"]) and got["hausd"] >= 0
