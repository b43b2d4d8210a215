#!/usr/bin/env python3
"""Golden values of the reference's brain extractor (keymorph/model.py:533-616, Simple_Unet), written to
tests/golden/brainmask*.npz.  Build container only: it imports the REAL reference on the CPU with the same stub packages
tools/make_golden_lc2.py installs and runs its forward and autograd, in fp32 and -- the same module, .double() -- in fp64.

    KEYMORPH_REFERENCE=<checkout of the reference> python tools/make_golden_brainmask.py

The notebook's channel lists with out_ch = 1, seeded weights (ONE state_dict: InstanceNorm holds no parameters, so both
cases share it), seeded input and a fixed cotangent.  Two cases:
    plain     use_in=False at (2, 1, 32, 16, 48): non-cubic, batch of 2, bottleneck 2 x 1 x 3
    instance  use_in=True  at (1, 1, 32, 32, 32): the smallest cube whose bottleneck has more than one voxel (the
              reference's InstanceNorm refuses a single voxel)
Arrays only.  No committed file may exceed 1 MiB, so the arrays are packed into numbered parts of at most 900 KB
(tests/brainmask_ref.py::load_fixture merges them), and the results of the fp64 run are stored rounded to fp32: they only feed
the RECORD of distances (1e-7 .. 1e-3 relative), which a 6e-8 rounding does not move at the two digits that are printed.
Keys: "keys" (ordered state_dict names), "sd::<name>", and per case c: "c::x", "c::cot", "c::y", "c::y64", "c::gx", "c::gx64",
"c::g::<name>", "c::g64::<name>".
"""
import os
import sys
import tempfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

REF = os.environ.get("KEYMORPH_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REF:
    sys.exit("set KEYMORPH_REFERENCE (or pass the path) to a checkout of the reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
PART_BYTES = 900 * 1024


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

from keymorph.model import Simple_Unet  # noqa: E402

ENC, DEC = [4, 8, 16, 32], [32, 16, 8, 4]
CASES = {"plain": (False, (2, 1, 32, 16, 48)), "instance": (True, (1, 1, 32, 32, 32))}


def seeded_state(net, seed):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in net.state_dict().items():
        r = torch.randn(v.shape, generator=g)
        out[k] = r / float(np.sqrt(np.prod(v.shape[1:]))) * 1.4 if v.dim() > 1 else 0.1 * r
    return out


def run(net, x, cot):
    x = x.clone().requires_grad_(True)
    y = net(x)
    y.backward(cot)
    return y.detach(), x.grad.detach(), {k: p.grad.detach() for k, p in net.named_parameters()}


def main():
    torch.manual_seed(0)
    d = {}
    sd = None
    for ci, (name, (use_in, shape)) in enumerate(CASES.items()):
        net = Simple_Unet(1, 1, use_in, ENC, DEC)
        if sd is None:
            sd = seeded_state(net, 20)
            d["keys"] = np.array(list(sd.keys()))
            for k, v in sd.items():
                d["sd::" + k] = v.numpy()
        net.load_state_dict(sd, strict=True)
        g = torch.Generator().manual_seed(100 + ci)
        x = torch.randn(shape, generator=g)
        cot = torch.randn(shape, generator=g)
        y, gx, gp = run(net, x, cot)
        net64 = Simple_Unet(1, 1, use_in, ENC, DEC).double()
        net64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        y64, gx64, gp64 = run(net64, x.double(), cot.double())
        d[f"{name}::x"], d[f"{name}::cot"] = x.numpy(), cot.numpy()
        d[f"{name}::y"], d[f"{name}::y64"] = y.numpy(), y64.float().numpy()
        d[f"{name}::gx"], d[f"{name}::gx64"] = gx.numpy(), gx64.float().numpy()
        for k in sd:
            d[f"{name}::g::{k}"], d[f"{name}::g64::{k}"] = gp[k].numpy(), gp64[k].float().numpy()
        rel = lambda a, b: float((a.double() - b).norm() / b.norm())      # noqa: E731
        print(name, "y rel L2 (fp32 vs fp64)", rel(y, y64), "gx", rel(gx, gx64))
    for f in os.listdir(GOLDEN):
        if f.startswith("brainmask") and f.endswith(".npz"):
            os.remove(os.path.join(GOLDEN, f))
    parts, cur, size = [], {}, 0
    for k, v in d.items():
        if cur and size + v.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    parts.append(cur)
    for i, part in enumerate(parts):
        out = os.path.join(GOLDEN, "brainmask.npz" if i == 0 else f"brainmask_part{i}.npz")
        np.savez_compressed(out, **part)
        print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
