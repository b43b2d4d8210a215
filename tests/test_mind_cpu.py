"""CPU: the restatement of the MIND-SSC distance (tests/mind_ref.py) is what it claims to be -- its closed-form gradient equals
autograd, it has the invariances the definition promises -- the C ABI declares and exports the kernel's entries, and on a pair
under an inverted non-linear contrast and a smooth bias field the restated deformable driver recovers the deformation with the
local descriptor where mutual information does not."""
import os
import re

import pytest
import torch

from tests import mind_ref as R

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNTIED = [name for name in R.CASES if name not in R.TIED]


@pytest.mark.parametrize("name", UNTIED)
def test_closed_form_equals_autograd(name):
    a, b, r, d = R.case_inputs(name)
    _, da, db = R.evaluate(a, b, r, d)
    ca, cb = R.closed_form(a, b, r, d)
    for got, ref in ((ca, da), (cb, db)):
        for n in range(a.shape[0]):
            err = float((got[n] - ref[n]).norm() / ref[n].norm())
            print(f"{name}[{n}]: closed form vs autograd, relative L2 {err:.3e}")
            assert err <= 1e-10, (name, n, err)


def test_closed_form_is_finite_under_exact_ties():
    """`masked`: the low-x half of a is 0, so all 12 distances tie at 0 there and the clamp sits at its lower bound, while the
    cotangent is not 0 (b's descriptor is not 1).  The closed form sends the minimum's share to channel 0; away from the zero
    half it is the untied gradient, so it equals autograd wherever D has no tie."""
    a, b, r, d = R.case_inputs("masked")
    ca, cb = R.closed_form(a, b, r, d)
    assert torch.isfinite(ca).all() and torch.isfinite(cb).all()
    _, da, db = R.evaluate(a, b, r, d)
    far = a.shape[4] // 2 + 2 * (r + d)                # beyond the reach of the tied voxels
    assert float((ca[..., far:] - da[..., far:]).norm() / da[..., far:].norm()) <= 1e-10
    assert float((cb - db).norm() / db.norm()) <= 1e-10                      # b has no ties
    M = R.descriptor(a.double(), r, d, R.bounds_of(a.double(), b.double(), r, d)[:, 0])
    assert float((M[..., :a.shape[4] // 2 - r - d] - 1).abs().max()) == 0.0


@pytest.mark.parametrize("name", ["tiny_ragged", "ragged_r1d1", "r3d3"])
def test_invariant_to_offset_and_scale(name):
    """a -> s a + t scales every D_c by s^2, and m / V with it when the bounds are recomputed: the descriptor does not change.
    s = 4 and t = 1 keep the float32 inputs exact in fp64 up to the rounding of the sums."""
    a, b, r, d = R.case_inputs(name)
    a, b = a.double(), b.double()
    base = R.mind(a, b, r, d)
    moved = R.mind(4.0 * a + 1.0, -0.5 * b - 3.0, r, d)
    err = float((base - moved).abs().max())
    print(f"{name}: value {float(base[0]):.6e}  change under affine intensity maps {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("name", list(R.CASES))
def test_zero_on_itself_and_symmetric(name):
    a, b, r, d = R.case_inputs(name)
    a, b = a.double(), b.double()
    assert float(R.mind(a, a, r, d).abs().max()) == 0.0
    out = R.mind(a, b, r, d)
    assert torch.equal(out, R.mind(b, a, r, d))
    assert float(out.min()) > 0.0


def test_flat_volume_has_descriptor_one_and_finite_gradients():
    _, b, r, d = R.case_inputs("ragged_r1d1")
    flat = torch.full_like(b, 3.0)
    bounds = R.bounds_of(flat.double(), b.double(), r, d)
    assert float(bounds[0, 0].abs().max()) == 0.0                            # lo = hi = 0: nothing is divided by it
    for dtype in (F64, torch.float32):
        M = R.descriptor(flat.to(dtype), r, d, bounds[:, 0].to(dtype))
        assert float((M - 1).abs().max()) == 0.0
        out, da, db = R.evaluate(flat, b, r, d, dtype=dtype)
        assert torch.isfinite(out).all() and torch.isfinite(da).all() and torch.isfinite(db).all()
        ca, cb = R.closed_form(flat, b, r, d, dtype=dtype)
        assert torch.isfinite(ca).all() and torch.isfinite(cb).all()
    assert float(R.mind(flat, flat, r, d).abs().max()) == 0.0


def test_header_declares_and_library_exports_the_entries():
    from keymorph_amd import _lib, build
    txt = open(os.path.join(ROOT, "include", "keymorph_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    if not os.path.exists(build.LIBPATH):
        build.build()
    lib = _lib.load()
    for name in ("kmh_mind_ws_bytes", "kmh_mind_bounds", "kmh_mind_fwd", "kmh_mind_bwd"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.PROTOS and hasattr(lib, name), name
    # two floats per 4 x 8 x 32 tile and sample, and the backward's 12 + 6 fields of the volume's size; 0 for what the entries refuse
    tiles, voxels = 10 * 5 * 3, 40 * 36 * 70
    assert lib.kmh_mind_ws_bytes(2, 40, 36, 70, 1, 2) >= 2 * 2 * tiles * 4 + 18 * 2 * voxels * 4
    assert lib.kmh_mind_ws_bytes(2, 40, 36, 70, 1, 2) <= 2 * 2 * tiles * 4 + 256 + 18 * 2 * voxels * 4
    assert lib.kmh_mind_ws_bytes(2, 40, 36, 70, 3, 3) == lib.kmh_mind_ws_bytes(2, 40, 36, 70, 1, 1)
    for args in ((0, 40, 36, 70, 1, 2), (2, 0, 36, 70, 1, 2), (2, 40, 36, -1, 1, 2), (2, 40, 36, 70, 0, 2), (2, 40, 36, 70, 4, 2),
                 (2, 40, 36, 70, 1, 0), (2, 40, 36, 70, 1, 4), (1, 2048, 1024, 1024, 1, 2)):
        assert lib.kmh_mind_ws_bytes(*args) == 0, args


def test_local_descriptor_recovers_under_inverted_contrast_and_bias_where_mutual_information_does_not():
    """The restated driver in fp64 on inverted_pair(), each metric run once and cached.  Measured: identity 1.786, "mind" 0.859,
    "mi" 1.671 voxels."""
    err, start = R.inverted_run("mind")
    err_mi, _ = R.inverted_run("mi")
    print(f"inverted pair: identity {start:.3f}  mind {err:.3f}  mi {err_mi:.3f} voxel")
    assert err <= 0.6 * start, (err, start)
    assert err_mi > err, (err_mi, err)
    # the figures the GPU test prints beside its own
    for key, got in (("identity", start), ("mind", err), ("mi", err_mi)):
        assert abs(got - R.RESTATED[key]) <= 0.05, (key, got)
