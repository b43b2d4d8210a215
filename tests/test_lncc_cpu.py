"""CPU: the restatement of local normalised cross-correlation (tests/lncc_ref.py) is what it claims to be -- its closed-form
gradient equals autograd, it has the invariances the definition promises -- the C ABI declares and exports the kernel's entries,
and on a pair under a smooth bias field the restated deformable driver recovers the deformation with the local metric where
mutual information does not."""
import os
import re

import pytest
import torch

from tests import lncc_ref as R

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(R.CASES))
def test_closed_form_equals_autograd(name):
    a, b, window = R.case_inputs(name)
    _, da, db = R.evaluate(a, b, window)
    ca, cb = R.closed_form(a, b, window)
    for got, ref in ((ca, da), (cb, db)):
        for n in range(a.shape[0]):
            err = float((got[n] - ref[n]).norm() / ref[n].norm())
            print(f"{name}[{n}]: closed form vs autograd, relative L2 {err:.3e}")
            assert err <= 1e-10, (name, n, err)


@pytest.mark.parametrize("name", ["tiny_ragged", "odd_box_w5", "w15"])
def test_invariant_to_offset_and_scale(name):
    """cc changes under b -> s b only through eps (eps -> s^2 eps undoes it) and not at all under a constant offset.

    To 1e-12 in the arithmetic the kernel uses, in fp64: each sample recentred by its first voxel (the float32 inputs, 1000 and 50
    are exact in fp64, so the offset leaves the recentred volume bit for bit and the scale is what is tested), and to 1e-12 without
    recentring for the scale alone.  Without recentring the OFFSET t costs fp64 itself t^2 / variance * 2^-53 per rounding of
    Saa - Sa^2 / n: the inputs' noise (sd 0.05) keeps the variance above 2.5e-3, so 1e6 / 2.5e-3 * 1.1e-16 = 4.4e-8 relative,
    and with the two roundings of the difference that evaluation gets 1e-7 (measured: 1e-10 .. 6e-9 on the mean) -- still four
    orders under what zero padding does to the value, which is what the truncated windows are for."""
    a, b, window = R.case_inputs(name)
    a, b = a.double(), b.double()
    eps, s = 1e-5, 50.0

    def mean(x, y, e, recentre, pad=False):
        if pad:                                    # the zero-padded variant: n = w^3 everywhere
            n = float(window ** 3)
            Sa, Sb, Saa, Sbb, Sab = (R.box(t, window) for t in (x, y, x * x, y * y, x * y))
            cross, va, vb = Sab - Sa * Sb / n, (Saa - Sa * Sa / n).clamp_min(0), (Sbb - Sb * Sb / n).clamp_min(0)
            return (cross * cross / (va * vb + e)).mean(dim=(1, 2, 3, 4))
        return R.lncc_map(x, y, window, e, recentre=recentre).mean(dim=(1, 2, 3, 4))
    base = mean(a, b, eps, True)
    assert float((base - mean(a + 1000.0, s * b + 300.0, eps * s * s, True)).abs().max()) <= 1e-12
    plain = mean(a, b, eps, False)
    assert float((plain - base).abs().max()) <= 1e-12
    assert float((plain - mean(a, s * b, eps * s * s, False)).abs().max()) <= 1e-12
    moved = float((plain - mean(a + 1000.0, s * b + 300.0, eps * s * s, False)).abs().max())
    padded = float((mean(a, b, eps, False, pad=True) - mean(a + 1000.0, s * b + 300.0, eps * s * s, False, pad=True)).abs().max())
    print(f"{name}: offset 1000 without recentring moves the fp64 value by {moved:.3e}; with zero padding by {padded:.3e}")
    assert moved <= 1e-7 and padded > 1e-3


def test_affine_related_volumes_score_one():
    a, _, window = R.case_inputs("odd_box_w5")
    out = R.lncc(a, -3.0 * a.double() + 2.0, window, 1e-12)
    assert float((out - 1).abs().max()) <= 1e-6, out


@pytest.mark.parametrize("name", list(R.CASES))
def test_symmetric_and_in_range(name):
    a, b, window = R.case_inputs(name)
    cc = R.lncc_map(a.double(), b.double(), window)
    assert torch.equal(cc, R.lncc_map(b.double(), a.double(), window))
    assert float(cc.min()) >= 0.0 and float(cc.max()) <= 1.0 + 1e-12


def test_constant_windows_score_exactly_zero():
    a, b, window = R.case_inputs("masked")
    r, half = window // 2, a.shape[4] // 2
    for dtype in (F64, torch.float32):
        cc = R.lncc_map(a.to(dtype), b.to(dtype), window)
        assert float(cc[..., :half - r].abs().max()) == 0.0 and float(cc[..., half:].max()) > 0.0
    _, da, db = R.evaluate(a, b, window)
    assert torch.isfinite(da).all() and torch.isfinite(db).all()


def test_header_declares_and_library_exports_the_entries():
    from keymorph_amd import _lib, build
    txt = open(os.path.join(ROOT, "include", "keymorph_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    if not os.path.exists(build.LIBPATH):
        build.build()
    lib = _lib.load()
    for name in ("kmh_lncc_ws_bytes", "kmh_lncc_fwd", "kmh_lncc_bwd"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.PROTOS and hasattr(lib, name), name
    # one float per 16 x 8 x 32 tile and sample, and five fields of the volume's size; 0 for what the entries refuse
    assert lib.kmh_lncc_ws_bytes(2, 40, 36, 70, 9) >= 2 * (3 * 5 * 3) * 4 + 5 * 2 * 40 * 36 * 70 * 4
    assert lib.kmh_lncc_ws_bytes(2, 40, 36, 70, 9) <= 2 * (3 * 5 * 3) * 4 + 256 + 5 * 2 * 40 * 36 * 70 * 4
    assert lib.kmh_lncc_ws_bytes(2, 40, 36, 70, 8) == 0 and lib.kmh_lncc_ws_bytes(0, 40, 36, 70, 9) == 0
    assert lib.kmh_lncc_ws_bytes(1, 40, 36, 70, 17) == 0 and lib.kmh_lncc_ws_bytes(1, 2048, 1024, 1024, 9) == 0


def test_local_metric_recovers_under_a_bias_field_where_mutual_information_does_not():
    """The restated driver in fp64 on biased_pair(), each metric run once and cached.  Measured: identity 1.786, "lncc" 0.621,
    "mi" 1.575 voxels."""
    err, start = R.biased_run("lncc")
    err_mi, _ = R.biased_run("mi")
    print(f"biased pair: identity {start:.3f}  lncc {err:.3f}  mi {err_mi:.3f} voxel")
    assert err <= start / 2, (err, start)
    assert err_mi > err, (err_mi, err)
    # the figures the GPU test prints beside its own
    for key, got in (("identity", start), ("lncc", err), ("mi", err_mi)):
        assert abs(got - R.RESTATED[key]) <= 0.05, (key, got)
