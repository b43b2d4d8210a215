"""CPU: evaluation metrics wiring (fast_dice / dice / hausdorff_distance), and the consistency of
tests/golden/eval_metrics.npz with a numpy brute force.  The helpers here are shared with test_eval_metrics_gpu.py."""
import math
import os

import numpy as np
import pytest

from tests.util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SAMPLING = (1.25, 1.25, 10.0)


def surface(m):
    """m & ~erode(m), 6-neighbour cross, zero border (scipy binary_erosion with generate_binary_structure(3, 1))."""
    p = np.pad(np.asarray(m, bool), 1)
    inner = p[1:-1, 1:-1, 1:-1].copy()
    for ax in range(3):
        for sh in (-1, 1):
            inner &= np.roll(p, sh, axis=ax)[1:-1, 1:-1, 1:-1]
    return np.asarray(m, bool) & ~inner


def min_sq_dist(points, targets, sampling, chunk=1024):
    """For each point (k, 3) the smallest ((dx sx)^2 + (dy sy)^2) + (dz sz)^2 over targets (n, 3), in that order."""
    sz, sy, sx = sampling
    out = np.full(len(points), np.inf)
    if len(targets) == 0:
        return out
    t = targets.astype(np.float64)
    for i in range(0, len(points), chunk):
        p = points[i:i + chunk].astype(np.float64)
        dz = (p[:, None, 0] - t[None, :, 0]) * sz
        dy = (p[:, None, 1] - t[None, :, 1]) * sy
        dx = (p[:, None, 2] - t[None, :, 2]) * sx
        out[i:i + chunk] = ((dx * dx + dy * dy) + dz * dz).min(1)
    return out


def brute_sq_map(m, sampling):
    """Squared distance from every voxel to the surface of m, (D, H, W) fp64."""
    pts = np.argwhere(np.ones(m.shape, bool))
    return min_sq_dist(pts, np.argwhere(surface(m)), sampling).reshape(m.shape)


def brute_hausdorff(a, b, sampling=REF_SAMPLING):
    """Batch mean of sqrt(max(max d_A^2 over S_B, max d_B^2 over S_A)) for (bs, D, H, W) masks."""
    hd = 0
    for i in range(len(a)):
        sa, sb = np.argwhere(surface(a[i])), np.argwhere(surface(b[i]))
        hd += math.sqrt(max(min_sq_dist(sb, sa, sampling).max(initial=-1), min_sq_dist(sa, sb, sampling).max(initial=-1)))
    return hd / len(a)


def hd_case(g, name):
    shape = tuple(int(v) for v in g[f"hd::{name}::shape"])
    n = int(np.prod(shape))
    a = np.unpackbits(g[f"hd::{name}::a"])[:n].reshape(shape).astype(bool)
    b = np.unpackbits(g[f"hd::{name}::b"])[:n].reshape(shape).astype(bool)
    return a, b, float(g[f"hd::{name}::value"])


def param_volume_np(shape, boxes, ellipsoids):
    """Union of boxes [z0, z1, y0, y1, x0, x1) and integer ellipsoids (cz, cy, cx, rz, ry, rx), int64 arithmetic."""
    D, H, W = shape
    m = np.zeros(shape, dtype=bool)
    for z0, z1, y0, y1, x0, x1 in boxes:
        m[z0:z1, y0:y1, x0:x1] = True
    z, y, x = np.ogrid[:D, :H, :W]
    for cz, cy, cx, rz, ry, rx in ellipsoids:
        q = ((z - cz) ** 2 * (ry * rx) ** 2 + (y - cy) ** 2 * (rz * rx) ** 2 + (x - cx) ** 2 * (rz * ry) ** 2)
        m |= q <= (rz * ry * rx) ** 2
    return m


def test_metric_names_registered():
    from keymorph_amd.loss_ops import MultipleAvgSegPairwiseMetric, fast_dice, hausdorff_distance
    fns = MultipleAvgSegPairwiseMetric().name2fn
    assert fns["hausd"] is hausdorff_distance and fns["dice"] is fast_dice


def test_hausdorff_of_a_non_array_raises_type_and_not_implemented():
    from keymorph_amd.loss_ops import hausdorff_distance
    with pytest.raises(TypeError) as e:
        hausdorff_distance(None, None)
    assert isinstance(e.value, NotImplementedError)


@pytest.mark.parametrize("name", ["blobs", "odd_37x64x23", "flat_1x40x33", "thin", "faces"])
def test_fixture_matches_brute_force(name):
    a, b, ref = hd_case(golden("eval_metrics.npz"), name)
    assert brute_hausdorff(a, b) == ref


def test_param_volume_recipe_sane():
    m = param_volume_np((9, 10, 11), [(1, 3, 2, 4, 0, 11)], [(5, 5, 5, 3, 2, 4)])
    assert m[1:3, 2:4, :].all() and m[5, 5, 5] and m[5, 5, 1] and not m[5, 5, 0] and not m[5, 8, 5]


def test_new_symbols_in_header_and_protos():
    from keymorph_amd import _lib
    txt = open(os.path.join(ROOT, "include", "keymorph_hip.h")).read()
    for name in ("kmh_hausdorff3d", "kmh_hausdorff3d_ws_bytes", "kmh_edt3d_sq", "kmh_edt3d_sq_ws_bytes", "kmh_label_counts"):
        assert name + "(" in txt and name in _lib.PROTOS, name
