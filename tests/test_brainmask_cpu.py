"""CPU: the brain extractor's module surface (state_dict of the reference's Simple_Unet, checkpoint loading), the per-axis
definition of the trilinear resize against F.interpolate, and the host oracle of clean_mask on masks with known answers."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import brainmask_ref as R


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


# ---- module surface ---------------------------------------------------------------------------------------------------
def test_state_dict_matches_the_reference(fx):
    from keymorph_amd.model import Simple_Unet, simple_block
    net = Simple_Unet(1, 1, False, R.ENC_NF, R.DEC_NF)                 # constructs on the CPU
    sd = net.state_dict()
    keys = [str(k) for k in fx["keys"]]
    assert list(sd.keys()) == keys
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(fx["sd::" + k].shape) for k in keys}
    assert sorted(keys) == sorted([f"block{i}.conv1.{p}" for i in range(9) for p in ("weight", "bias")]
                                  + ["conv.weight", "conv.bias"])
    assert not list(net.buffers())                                      # InstanceNorm: no parameters, no buffers
    assert isinstance(net.block0, simple_block) and isinstance(net, torch.nn.Module)
    for (cin, cout), k in zip(R.LAYER_PAIRS, keys[::2]):
        assert tuple(sd[k].shape) == (cout, cin, 3, 3, 3), k
    net.load_state_dict(R.fixture_state_dict(fx), strict=True)
    assert Simple_Unet(1, 1, True, R.ENC_NF, R.DEC_NF).state_dict().keys() == sd.keys()


@pytest.mark.parametrize("prefix", ["", "module."])
def test_load_brain_extractor(fx, prefix, tmp_path):
    from keymorph_amd.io import load_brain_extractor
    sd = R.fixture_state_dict(fx)
    path = tmp_path / "brain_extraction_model.pth.tar"
    torch.save({"u1": {prefix + k: v for k, v in sd.items()}}, path)
    net = load_brain_extractor(str(path))
    assert not net.training
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    bad = dict(sd)
    bad.pop("conv.bias")
    torch.save({"u1": bad}, path)
    with pytest.raises(RuntimeError):                                   # strict=True
        load_brain_extractor(str(path))


def test_cpu_input_is_an_error(fx):
    from keymorph_amd._lib import KeymorphHipError
    from keymorph_amd.model import Simple_Unet
    net = Simple_Unet(1, 1, False, R.ENC_NF, R.DEC_NF)
    with pytest.raises(ValueError, match="multiples of 16"):
        net(torch.zeros(1, 1, 16, 24, 16))
    with pytest.raises(KeymorphHipError):
        net(torch.zeros(1, 1, 16, 16, 16))


# ---- the resize definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: "%s-%s-%s" % (("x".join(map(str, c[0]))), c[1], c[2]))
def test_resize_restatement_vs_interpolate(case):
    """The per-axis tables evaluated in fp64 against F.interpolate in fp64: no farther than twice torch's own CPU fp32
    result is (the restatement rounds the coordinate once where torch rounds scale and coordinate) + 1e-7 max|x|; exact for
    dyadic scales.  The backward range tables are contiguous (resize_axis_table raises otherwise) and cover every reference."""
    shape, size, factor = case
    x = torch.randn(shape, generator=torch.Generator().manual_seed(7))
    tabs, out = R.resize_tables(shape, size, factor)
    kw = dict(size=size) if size is not None else dict(scale_factor=factor)
    ref64 = F.interpolate(x.double(), mode="trilinear", align_corners=False, **kw)
    ref32 = F.interpolate(x, mode="trilinear", align_corners=False, **kw)
    assert tuple(ref64.shape[2:]) == out
    mine = R.resize_ref64(x.double(), tabs)
    d_mine = float((mine - ref64).abs().max())
    d_torch = float((ref32.double() - ref64).abs().max())
    print(f"resize {shape} -> {out}: restatement {d_mine:.3e}, torch fp32 {d_torch:.3e}")
    assert d_mine <= 2 * d_torch + 1e-7 * float(x.abs().max())
    dyadic = all(o == 2 * i or 2 * o == i or o == i for i, o in zip(shape[2:], out))
    if dyadic:
        assert d_mine == 0.0
    for (i0, i1, lam, lo, hi), n_in, n_out in zip(tabs, shape[2:], out):
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and (lam >= 0).all()
        for i in range(n_in):
            ref = np.nonzero((i0 == i) | (i1 == i))[0]
            if len(ref):
                assert (lo[i], hi[i]) == (ref[0], ref[-1]) and len(ref) == hi[i] - lo[i] + 1
            else:
                assert lo[i] > hi[i]
        assert lo.min() >= 0 and hi.max() <= n_out - 1


def test_resize_argument_errors():
    from keymorph_amd import utils
    x = torch.zeros(1, 1, 4, 4, 4)
    with pytest.raises(ValueError):
        utils.resize_trilinear(x)
    with pytest.raises(ValueError):
        utils.resize_trilinear(x, size=(8, 8, 8), scale_factor=2)


# ---- the clean_mask oracle on masks with known answers ------------------------------------------------------------------
def test_oracle_corner_touching_cubes():
    from scipy import ndimage
    m = R.corner_cubes()
    assert R.label_oracle(m)[1] == 1                                   # 26-connectivity: one component
    assert ndimage.label(m)[1] == 2                                    # 6-connectivity: two
    assert np.array_equal(R.clean_mask_oracle(m, 0.2), m)


def test_oracle_threshold_is_strict():
    m = np.zeros((5, 5, 16), dtype=np.uint8)
    m[1, 1, 0:10] = 1                                                  # 10 voxels
    m[3, 3, 0:2] = 1                                                   # 2 voxels: 2 / 10 is not > 0.2
    m[3, 3, 8:11] = 1                                                  # 3 voxels: survives
    out = R.clean_mask_oracle(m, 0.2)
    assert out.dtype == np.uint8
    assert out[1, 1, 0:10].all() and not out[3, 3, 0:2].any() and out[3, 3, 8:11].all()
    assert out.sum() == 13
    with pytest.raises(ValueError):
        R.clean_mask_oracle(np.zeros((3, 3, 3), dtype=np.uint8))


def test_oracle_test_masks():
    assert R.label_oracle(R.serpentine(32))[1] == 1
    lab, n = R.label_oracle(R.blob_and_islands())
    assert sorted(np.bincount(lab.reshape(-1))[1:]) == [1, 7, 500, 501, 2000, 2001, 10000]
    out = R.clean_mask_oracle(R.blob_and_islands(), 0.2)
    assert out.sum() == 10000 + 2001
    assert R.clean_mask_oracle(R.blob_and_islands(), 0.05).sum() == 10000 + 2000 + 2001 + 501


def test_clean_mask_rejects_non_3d():
    from keymorph_amd.model import clean_mask
    with pytest.raises(ValueError):
        clean_mask(np.zeros((4, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        clean_mask(np.full((2, 2, 2), 2.0))
