#!/usr/bin/env python3
"""Golden values of the reference's LC2 / ImageLC2 (keymorph/loss_ops.py:250-391), written to tests/golden/lc2.npz.  Build
container only: it imports the REAL reference on the CPU with the same stub packages tools/make_golden_eval_metrics.py
installs, and runs the reference's forward and its fp32 autograd.

    python tools/make_golden_lc2.py

Inputs are not stored: tests/test_lc2_cpu.py::lc2_pair rebuilds them from the case table (integer draws, exact arithmetic).
Stored: forward values, and d/d(us), d/d(mr) -- whole volumes for LC2, the halo box of every patch for ImageLC2 (the gradient
is zero elsewhere, which the tests check on the volumes they compute).
"""
import os
import sys
import tempfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

REF = os.environ.get("KEYMORPH_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "lc2.npz")


def _install_stubs():
    d = tempfile.mkdtemp(prefix="km_stubs_")
    for name in ("nibabel", "skimage", "h5py"):
        os.makedirs(os.path.join(d, name))
        with open(os.path.join(d, name, "__init__.py"), "w") as f:
            f.write("morphology = None\n" if name == "skimage" else "")
    open(os.path.join(d, "skimage", "morphology.py"), "w").close()
    sys.path.insert(0, d)
    sys.path.insert(0, REF)
    sys.path.insert(1, ROOT)


_install_stubs()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keymorph import loss_ops  # noqa: E402
from tests.test_lc2_cpu import CASES, boxed, case_inputs, halo_boxes  # noqa: E402


def main():
    d = {}
    for name, c in CASES.items():
        us, mr = case_inputs(name)
        u = torch.tensor(us, requires_grad=True)
        m = torch.tensor(mr, requires_grad=True)
        if c["patch"] is None:
            out = loss_ops.LC2(radiuses=c["radii"])(u, m)
            out.sum().backward()
            d[f"{name}::fwd"] = out.detach().numpy()
            d[f"{name}::dus"], d[f"{name}::dmr"] = u.grad.numpy(), m.grad.numpy()
            print(name, out.detach().numpy())
        else:
            mod = loss_ops.ImageLC2(patch_size=c["patch"], radiuses=c["radii"])
            out = mod(u, m)
            out.backward()
            none = loss_ops.ImageLC2(patch_size=c["patch"], radiuses=c["radii"], reduction=None)(u.detach(), m.detach())
            d[f"{name}::fwd_mean"] = np.float32(out.item())
            d[f"{name}::fwd_none"] = none.numpy()
            d[f"{name}::dus_box"], d[f"{name}::dmr_box"] = boxed(u.grad.numpy(), name), boxed(m.grad.numpy(), name)
            rest = np.stack([u.grad.numpy(), m.grad.numpy()])
            for n, z, y, x in halo_boxes(name):
                rest[:, n, 0, z, y, x] = 0
            assert not rest.any(), name                        # nothing outside the boxes
            print(name, out.item(), none.numpy())
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
