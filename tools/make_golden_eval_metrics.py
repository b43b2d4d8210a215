#!/usr/bin/env python3
"""Golden values of the reference's evaluation metrics (keymorph/loss_ops.py:66-158: fast_dice, dice, hausdorff_distance),
written to tests/golden/eval_metrics.npz.  Build container only: it imports the REAL reference with the same three stub
packages tools/make_golden.py installs (the real scipy does the distance transforms).

    python tools/make_golden_eval_metrics.py

What is committed is data: channel-0 masks as np.packbits with their shapes, label maps, integer parameters of the 256^3
volumes (unions of boxes and integer ellipsoids, rebuilt exactly by tests/test_eval_metrics_gpu.py::param_volume) and
the reference's values.  Each 256^3 case costs the reference about 13 s.
"""
import os
import sys
import tempfile
import time

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

REF = os.environ.get("KEYMORPH_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "eval_metrics.npz")


def _install_stubs():
    d = tempfile.mkdtemp(prefix="km_stubs_")
    for name in ("nibabel", "skimage", "h5py"):
        os.makedirs(os.path.join(d, name))
        with open(os.path.join(d, name, "__init__.py"), "w") as f:
            f.write("morphology = None\n" if name == "skimage" else "")
    open(os.path.join(d, "skimage", "morphology.py"), "w").close()
    sys.path.insert(0, d)
    sys.path.insert(0, REF)


_install_stubs()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from keymorph import loss_ops  # noqa: E402
from keymorph.utils import align_img  # noqa: E402


def param_volume(shape, boxes, ellipsoids):
    """Union of boxes [z0, z1, y0, y1, x0, x1) and ellipsoids (cz, cy, cx, rz, ry, rx):
    (z-cz)^2 (ry rx)^2 + (y-cy)^2 (rz rx)^2 + (x-cx)^2 (rz ry)^2 <= (rz ry rx)^2, in int64 (same recipe as the test)."""
    D, H, W = shape
    m = np.zeros(shape, dtype=bool)
    for z0, z1, y0, y1, x0, x1 in boxes:
        m[z0:z1, y0:y1, x0:x1] = True
    z, y, x = np.ogrid[:D, :H, :W]
    for cz, cy, cx, rz, ry, rx in ellipsoids:
        q = ((z - cz) ** 2 * (ry * rx) ** 2 + (y - cy) ** 2 * (rz * rx) ** 2 + (x - cx) ** 2 * (rz * ry) ** 2)
        m |= q <= (rz * ry * rx) ** 2
    return m


def blobs(rng, shape, thr):
    """Random blobs: box-smoothed uniform noise above a threshold."""
    v = torch.tensor(rng.random(shape), dtype=torch.float32)[None, None]
    k = tuple(min(5, n if n % 2 else n - 1) for n in shape)
    v = F.avg_pool3d(v, k, stride=1, padding=tuple(c // 2 for c in k), count_include_pad=False)[0, 0].numpy()
    return v > thr


def main():
    rng = np.random.default_rng(20261016)
    d = {}
    names = []

    def hd_case(name, a, b):
        """a, b: (bs, D, H, W) bool channel-0 masks; reference value on float32 (bs, 1, D, H, W) arrays."""
        a, b = np.asarray(a, bool), np.asarray(b, bool)
        assert a.shape == b.shape and a.ndim == 4
        hd = loss_ops.hausdorff_distance(a[:, None].astype(np.float32), b[:, None].astype(np.float32))
        d[f"hd::{name}::shape"] = np.array(a.shape, dtype=np.int64)
        d[f"hd::{name}::a"] = np.packbits(a.ravel())
        d[f"hd::{name}::b"] = np.packbits(b.ravel())
        d[f"hd::{name}::value"] = np.float64(hd)
        names.append(name)
        print(f"hd {name} {a.shape}: {hd!r}")

    # random blobs, bs = 2
    hd_case("blobs", np.stack([blobs(rng, (20, 22, 18), 0.5) for _ in range(2)]),
            np.stack([blobs(rng, (20, 22, 18), 0.5) for _ in range(2)]))
    # odd and flat shapes
    hd_case("odd_37x64x23", blobs(rng, (37, 64, 23), 0.5)[None], blobs(rng, (37, 64, 23), 0.49)[None])
    hd_case("flat_1x40x33", blobs(rng, (1, 40, 33), 0.5)[None], blobs(rng, (1, 40, 33), 0.52)[None])
    # thin and one-voxel structures
    a = np.zeros((16, 17, 19), bool)
    a[8, 3:14, 2:17] = True               # one-voxel-thick plane
    a[2:14, 9, 9] = True                  # a line through it
    b = np.zeros_like(a)
    b[3, 4, 5] = True                     # a single voxel
    b[12, 2:15, 14] = True
    hd_case("thin", a[None], b[None])
    # a mask touching every face against an interior blob
    a = np.ones((18, 21, 15), bool)
    a[4:14, 5:16, 3:12] = False
    hd_case("faces", a[None], blobs(rng, (18, 21, 15), 0.5)[None])

    # soft segmentations the reference itself warped (groupwise_eval_tiny.npz)
    ge = np.load(os.path.join(os.path.dirname(OUT), "groupwise_eval_tiny.npz"))
    for key, ref in (("affine::seg_a_1", "seg_0"), ("tps_1::seg_a_1", "seg_2")):
        hd = loss_ops.hausdorff_distance(ge[key], ge[ref].astype(np.float32))
        d[f"hdsoft::{key}::{ref}"] = np.float64(hd)
        print(f"hd soft {key} vs {ref}: {hd!r}")

    # a one-hot map warped by the reference's align_img under a rotation, 96^3
    S = 96
    lab = np.zeros((S, S, S), np.int64)
    lab[param_volume((S, S, S), [], [(48, 48, 48, 36, 30, 40)])] = 1
    lab[param_volume((S, S, S), [(30, 50, 40, 60, 20, 44)], [(56, 40, 58, 12, 16, 10)])] = 2
    onehot = F.one_hot(torch.tensor(lab), 3).permute(3, 0, 1, 2)[None].float()
    ang = np.deg2rad(11.0)
    theta = torch.tensor([[[np.cos(ang), -np.sin(ang), 0, 0.03], [np.sin(ang), np.cos(ang), 0, -0.02], [0, 0, 1, 0.01]]],
                         dtype=torch.float32)
    grid = F.affine_grid(theta, onehot.shape, align_corners=False)
    warped = align_img(grid, onehot)
    hd_case("rot96", (warped[:, 0] != 0).numpy(), (onehot[:, 0] != 0).numpy())
    hd_direct = loss_ops.hausdorff_distance(warped, onehot)
    assert hd_direct == d["hd::rot96::value"], (hd_direct, d["hd::rot96::value"])

    # 256^3 volumes as integer parameters
    big = {
        "boxes256": ([(40, 200, 50, 210, 60, 190)], [(60, 170, 30, 230, 70, 200)], []),
        "brain256": ([(100, 140, 90, 170, 120, 136)], [(64, 190, 40, 220, 30, 226)],
                     [(128, 128, 128, 96, 110, 100), (150, 110, 130, 40, 35, 50)]),
    }
    for name, (boxes_a, boxes_b, ells) in big.items():
        ell_a, ell_b = ells[:1], ells[1:]
        ba = np.array(boxes_a, np.int64).reshape(-1, 6)
        bb = np.array(boxes_b, np.int64).reshape(-1, 6)
        ea = np.array(ell_a, np.int64).reshape(-1, 6)
        eb = np.array(ell_b, np.int64).reshape(-1, 6)
        A = param_volume((256, 256, 256), ba, ea)
        B = param_volume((256, 256, 256), bb, eb)
        t0 = time.time()
        hd = loss_ops.hausdorff_distance(A[None, None].astype(np.float32), B[None, None].astype(np.float32))
        print(f"hd {name} 256^3: {hd!r} ({time.time() - t0:.1f} s on the host)")
        for k, v in (("boxes_a", ba), ("boxes_b", bb), ("ell_a", ea), ("ell_b", eb)):
            d[f"big::{name}::{k}"] = v
        d[f"big::{name}::value"] = np.float64(hd)

    # fast_dice / dice
    lx = rng.integers(0, 5, (2, 12, 14, 10)).astype(np.uint8)
    ly = np.where(rng.random(lx.shape) < 0.7, lx, rng.integers(0, 5, lx.shape)).astype(np.uint8)
    ly[ly == 3] = 4                                           # label 3 only in x
    oh = lambda l, c: np.moveaxis(np.eye(c, dtype=np.float32)[l], -1, 1)   # noqa: E731
    d["fd::onehot::x"], d["fd::onehot::y"], d["fd::onehot::C"] = lx, ly, np.int64(5)
    d["fd::onehot::value"] = np.float64(loss_ops.fast_dice(oh(lx, 5), oh(ly, 5)))
    tx = (rng.integers(0, 3, (2, 4, 6, 5, 7)) * 0.5).astype(np.float32)    # many argmax ties
    ty = (rng.integers(0, 3, (2, 4, 6, 5, 7)) * 0.5).astype(np.float32)
    d["fd::ties::x"], d["fd::ties::y"] = tx, ty
    d["fd::ties::value"] = np.float64(loss_ops.fast_dice(tx, ty))
    z = np.zeros((1, 9, 8, 7), np.uint8)
    d["fd::single::x"], d["fd::single::y"], d["fd::single::C"] = z, z, np.int64(3)
    d["fd::single::value"] = np.float64(loss_ops.fast_dice(oh(z, 3), oh(z, 3)))
    bx = rng.random((3, 11, 13, 9)) < 0.4
    by = rng.random((3, 11, 13, 9)) < 0.3
    d["dice::rand::x"], d["dice::rand::y"] = bx.astype(np.uint8), by.astype(np.uint8)
    d["dice::rand::value"] = np.float64(loss_ops.dice(bx, by))
    for k in ("onehot", "ties", "single"):
        print(f"fast_dice {k}: {d[f'fd::{k}::value']!r}")
    print(f"dice rand: {d['dice::rand::value']!r}")

    d["hd_names"] = np.array(names)
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
