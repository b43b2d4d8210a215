"""GPU: the trilinear label vote (csrc/label_warp.hip; ops.warp_labels, grid_sample3d(..., "label") and everything that hands a
mode to align_img) and Dice on integer label maps (csrc/label_dice.hip; loss_ops.label_dice).

The definition is exact, so every comparison here is equality: both outputs of warp_labels against the chain it replaces, run on
the GPU -- argmax and max over the channels of align_img(grid, one_hot(lab).float()) -- and against the numpy restatement
(tests/labelwarp_ref.py, itself pinned on the CPU).  Ids the chain cannot encode are checked by relabelling: the vote sees labels
only through == and <, so it commutes with any strictly increasing map of the ids."""
import functools

import numpy as np
import pytest
import torch

from tests import labelwarp_ref as R
from tests import sampler_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32

VOLUMES = [(1, 1, 1, 1, 1), (1, 1, 1, 1, 2), (1, 1, 3, 1, 5), (1, 2, 2, 3, 4), (2, 3, 5, 6, 7), (1, 1, 3, 40, 67),
           (1, 1, 1, 2, 771)]
# output shapes: 105, 105, 42, 30, 75, 80 and 2109 voxels -- every residue of 4, and two chunks of 1024 with a ragged third
KINDS = {"interior": (3, 5, 7), "outside": (3, 5, 7), "lattice": (2, 3, 7), "border": (2, 3, 5), "halfway": (3, 5, 5),
         "nonfinite": (2, 5, 8), "ragged": R.OUT_SHAPE}
DTYPES = [torch.uint8, torch.bool, torch.int16, torch.int32, torch.int64]
WIDE = [(torch.int16, [0, 7, 300, 2035]), (torch.int32, [-5, 0, 70000, 2 ** 31 - 1]), (torch.int64, [-2 ** 40, 0, 3, 2 ** 40]),
        (torch.uint8, [0, 1, 200, 255])]


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def labels(shape):
    """4 i.i.d. labels, int64 numpy"""
    return R.random_labels(shape, 4, seed=sum(shape) * 7 + 1)


@functools.lru_cache(maxsize=None)
def grid(shape, kind):
    name = "outside" if kind == "ragged" else kind
    return R.coordinate_set(name, shape[0], shape[2:], KINDS[kind], seed=list(KINDS).index(kind))


@functools.lru_cache(maxsize=None)
def restated(shape, kind, binary=False):
    lab = labels(shape) % 2 if binary else labels(shape)
    return R.vote(lab, grid(shape, kind))


def chain(lab, g):
    """argmax and max over the channels of align_img(grid, one_hot(lab).float()), channel by channel of lab (N, C, ...) int64"""
    from keymorph_amd.utils import align_img, one_hot
    outs = [align_img(g, one_hot(lab[:, c:c + 1]).float()) for c in range(lab.shape[1])]
    return (torch.cat([torch.argmax(o, 1, keepdim=True) for o in outs], 1),
            torch.cat([o.max(1, keepdim=True).values for o in outs], 1))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", VOLUMES, ids=lambda s: "x".join(map(str, s)))
def test_definition(shape, kind):
    from keymorph_amd import ops
    g = torch.from_numpy(grid(shape, kind)).to(DEV)
    for binary in (False, True):
        lab64 = torch.from_numpy(labels(shape) % 2 if binary else labels(shape)).to(DEV)
        want, wwant = chain(lab64, g)
        rl, rw = restated(shape, kind, binary)
        for dt in ([torch.bool] if binary else [d for d in DTYPES if d != torch.bool]):
            got, w = ops.warp_labels(lab64.to(dt), g, return_weight=True)
            assert got.dtype == dt and w.dtype == torch.float32 and got.shape == want.shape == w.shape
            assert not got.requires_grad and not w.requires_grad
            nl, nw = int((got.long() != want).sum()), int((w != wwant).sum())
            ml, mw = int((_np(got.long()) != rl).sum()), int((_np(w) != rw).sum())
            assert nl == 0 and nw == 0, f"{dt}: {nl} labels and {nw} weights differ from the one-hot chain"
            assert ml == 0 and mw == 0, f"{dt}: {ml} labels and {mw} weights differ from the restatement"


@pytest.mark.parametrize("dt,ids", WIDE, ids=[str(d).split(".")[1] for d, _ in WIDE])
def test_wide_ids_by_relabelling(dt, ids):
    from keymorph_amd import ops
    r = torch.tensor(ids, dtype=dt, device=DEV)
    for shape in ((2, 3, 5, 6, 7), (1, 1, 3, 40, 67)):
        lab = torch.from_numpy(labels(shape)).to(DEV)
        for kind in ("outside", "halfway", "ragged"):
            g = torch.from_numpy(grid(shape, kind)).to(DEV)
            small, ws = ops.warp_labels(lab, g, return_weight=True)
            wide, ww = ops.warp_labels(r[lab], g, return_weight=True)
            assert wide.dtype == dt
            assert torch.equal(wide, r[small]) and torch.equal(ww, ws), (shape, kind)


def test_invariants():
    from keymorph_amd import ops
    shape = (2, 3, 5, 6, 7)
    lab = torch.from_numpy(labels(shape)).to(DEV).to(torch.int16)
    ident = S.identity(2, shape[2:])
    got, w = ops.warp_labels(lab, torch.from_numpy(ident).to(DEV), return_weight=True)
    assert torch.equal(got, lab) and bool((w > 0.999).all())      # (the fp32 centres of sizes 5, 6, 7 are an ulp off the lattice)
    got = ops.warp_labels(lab, torch.from_numpy(S.shift(ident, shape[2:], (2, -1, 1))).to(DEV))
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(7), indexing="ij")
    want = _np(lab)[:, :, np.clip(z + 1, 0, 4), np.clip(y - 1, 0, 5), np.clip(x + 2, 0, 6)]
    assert np.array_equal(_np(got), want)
    for kind in ("halfway", "ragged"):
        g = torch.from_numpy(grid(shape, kind)).to(DEV)
        out, w = ops.warp_labels(lab, g, return_weight=True)
        again, wagain = ops.warp_labels(lab, g, return_weight=True)
        assert torch.equal(out, again) and torch.equal(w, wagain)
        assert torch.equal(out, ops.warp_labels(lab, g))              # the all-equal shortcut leaks into neither variant
        for n in range(2):
            o, ww = ops.warp_labels(lab[n:n + 1].contiguous(), g[n:n + 1].contiguous(), return_weight=True)
            assert torch.equal(out[n:n + 1], o) and torch.equal(w[n:n + 1], ww)
        for c in range(3):
            o, ww = ops.warp_labels(lab[:, c:c + 1].contiguous(), g, return_weight=True)
            assert torch.equal(out[:, c:c + 1], o) and torch.equal(w[:, c:c + 1], ww)
    # a constant map takes the shortcut at every voxel: still the chain's weight
    const = torch.full((1, 1, 3, 40, 67), 5, dtype=torch.int64, device=DEV)
    g = torch.from_numpy(grid((1, 1, 3, 40, 67), "ragged")).to(DEV)
    out, w = ops.warp_labels(const, g, return_weight=True)
    _, wwant = chain(const, g)
    assert bool((out == 5).all()) and torch.equal(w, wwant)
    # under autograd the graph is left alone
    gr = g.clone().requires_grad_(True)
    assert not ops.warp_labels(const, gr).requires_grad
    assert not ops.grid_sample3d(const, gr, "label").requires_grad


def test_surface_is_warp_labels_of_the_same_grid(monkeypatch):
    from keymorph_amd import augmentation as A
    from keymorph_amd import ops
    from keymorph_amd import utils as U
    from keymorph_amd.io import apply_bspline, apply_mat, apply_svf, svf_grid, translate
    from keymorph_amd.transformations import AffineTransform
    from keymorph_amd.utils import align_img
    rng = np.random.default_rng(31)
    dims = (9, 10, 12)
    for dt in (torch.uint8, torch.int64):
        x = torch.from_numpy(rng.integers(0, 5, (2, 2) + dims)).to(DEV).to(dt)
        mat = torch.tensor(np.eye(3, 4)[None] + rng.normal(0, 0.05, (2, 3, 4)), dtype=torch.float32, device=DEV)
        ctrl = torch.tensor(rng.normal(0, 0.03, (2, 3) + ops.bspline_lattice_shape(dims, 4)), dtype=torch.float32, device=DEV)

        def same(got, g):
            assert got.dtype == dt and torch.equal(got, ops.warp_labels(x, g))

        g = ops.affine_grid(mat, dims)
        same(ops.grid_sample3d(x, g, "label"), g)
        same(align_img(g, x, "label"), g)
        same(apply_mat(x, mat, "label"), g)
        same(apply_bspline(x, ctrl, mat, "label"), ops.bspline_grid(ctrl, dims, mat))
        for inverse in (False, True):
            same(apply_svf(x, ctrl, mat, 4, inverse, "label"), svf_grid(ctrl, dims, mat, 4, inverse))
        t = torch.tensor([[1.0, -2.0, 0.5], [0.0, 3.0, -1.5]], device=DEV)
        seen = []                                                   # the grid translate builds, as it hands it to align_img
        with monkeypatch.context() as mp:
            mp.setattr(U, "align_img", lambda grid, vol, mode="bilinear": seen.append(grid) or align_img(grid, vol, mode))
            got = translate(x, t, "label")
        assert len(seen) == 1 and not torch.equal(seen[0], ops.affine_grid(mat, dims))
        same(got, seen[0])
        params = (torch.tensor([[1.1, 0.95, 1.05]]), torch.tensor([[0.05, -0.08, 0.03]]), torch.tensor([[0.2, -0.1, 0.15]]),
                  torch.tensor([[0.02, -0.03, 0.01, 0.02, -0.01, 0.03]]))
        aug = A.AffineDeformation3d(device=DEV)
        phi = AffineTransform(matrix=aug.build_affine_matrix(2, params)).get_flow_field(x.size())
        same(aug.deform_img(x, params, interp_mode="label"), phi)
        same(aug(x, params=params, interp_mode="label"), phi)
        assert not torch.equal(align_img(phi, x, "label"), align_img(phi, x.float(), "nearest").to(dt))
        # the 4-D path: a depth-1 volume sampled at z = 0
        x2 = x[:, :, 0].contiguous()
        g2 = torch.from_numpy(rng.random((2, 7, 9, 2), dtype=F32) * F32(2.4) - F32(1.2)).to(DEV)
        g3 = torch.cat([g2, torch.zeros_like(g2[..., :1])], -1).unsqueeze(1)
        got = align_img(g2, x2, "label")
        assert got.dtype == dt and got.shape == (2, 2, 7, 9)
        assert torch.equal(got, ops.warp_labels(x2.unsqueeze(2), g3).squeeze(2))
    with pytest.raises(ValueError):
        translate(x, torch.zeros(2, 3, device=DEV), "labels")


def test_refusals():
    from keymorph_amd import _lib, ops
    x = torch.zeros(1, 1, 3, 4, 5, dtype=torch.int32, device=DEV)
    g = torch.zeros(1, 2, 2, 2, 3, device=DEV)
    for f in (torch.float32, torch.float64, torch.float16):
        with pytest.raises(TypeError, match="integer"):
            ops.warp_labels(x.to(f), g)
    with pytest.raises(TypeError):
        ops.grid_sample3d(x.float(), g, "label")
    with pytest.raises(_lib.KeymorphHipError):
        ops.warp_labels(x.cpu(), g)
    with pytest.raises(_lib.KeymorphHipError):
        ops.warp_labels(x, g.cpu())
    for bad in (x[0], x[:, :, :, :, :0], x[:, :0]):
        with pytest.raises(ValueError):
            ops.warp_labels(bad, g)
    for bad in (g[0], g[..., :2], g[:, :0], torch.zeros(2, 2, 2, 2, 3, device=DEV)):
        with pytest.raises(ValueError):
            ops.warp_labels(x, bad)
    # a channel plane of 2^29 voxels: a view of one element, so nothing that large exists before or after the refusal
    assert ops.LABEL_MAX_PLANE == 1 << 29 and ops.LABEL_MAX_PLANES == 65535
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    for dt in (torch.uint8, torch.int64):
        huge = torch.zeros(1, dtype=dt, device=DEV).expand(1, 1, 1 << 9, 1 << 10, 1 << 10)
        for call in (lambda: ops.warp_labels(huge, g), lambda: ops.warp_labels(huge, g, return_weight=True),
                     lambda: ops.grid_sample3d(huge, g, "label")):
            with pytest.raises(ValueError):
                call()
    many = torch.zeros(1, dtype=torch.uint8, device=DEV).expand(256, 256, 1, 1, 1)      # N C one past the limit
    with pytest.raises(ValueError):
        ops.warp_labels(many, g.expand(256, 2, 2, 2, 3))
    assert torch.cuda.max_memory_allocated() < before + (1 << 28)      # (a copy of the byte map alone would be 512 MiB)
    ok = torch.zeros(1, dtype=torch.uint8, device=DEV).expand(255, 257, 1, 1, 1)        # 65535 planes: the limit itself
    assert ops.warp_labels(ok, g.expand(255, 2, 2, 2, 3)).shape == (255, 257, 2, 2, 2)


# ------------------------------------------------------------------------------------------------------------- label_dice
def test_label_dice_equals_fast_dice():
    from keymorph_amd.loss_ops import fast_dice, label_dice
    from keymorph_amd.utils import one_hot
    rng = np.random.default_rng(17)
    x = rng.integers(0, 6, (2, 1, 5, 6, 7))
    y = np.where(rng.random(x.shape) < 0.7, x, rng.integers(0, 6, x.shape))
    y[y == 4] = 0                                                    # label 4 in x only
    pairs = [(x, y), (np.full_like(x, 3), np.full_like(x, 3)), (x, x)]
    for a, b in pairs:
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        top = int(max(a.max(), b.max()))

        def channels(t):                                             # one_hot stops at t's own largest label: pad to the pair's
            oh = one_hot(t).float()
            return torch.cat([oh, oh.new_zeros((oh.shape[0], top + 1 - oh.shape[1]) + oh.shape[2:])], 1)

        want = fast_dice(channels(ta), channels(tb))
        for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):
            got = label_dice(ta.to(dt), tb.to(dt))
            assert isinstance(got, float) and got == want, (dt, got, want)
        assert label_dice(a, b) == want                              # numpy arrays
        assert label_dice(a.astype(np.uint16), tb) == want           # an unsigned array and a tensor of another dtype
        mean, ids, per = R.dice_formula(a, b)
        got, gids, gper = label_dice(ta, tb, return_per_label=True)
        assert got == want == mean and np.array_equal(gids, ids) and np.array_equal(gper, per)
        assert gids.dtype == np.int64 and gper.dtype == np.float64
    m = torch.from_numpy(rng.integers(0, 2, (3, 4, 5)).astype(bool)).to(DEV)
    assert label_dice(m, ~m) == 0.0 and label_dice(m, m) == pytest.approx(1.0, abs=1e-5)


def test_label_dice_wide_ids_and_refusals():
    from keymorph_amd.loss_ops import label_dice
    rng = np.random.default_rng(19)
    r = np.array([0, 7, 300, 2035], np.int16)
    x = r[rng.integers(0, 4, (1, 1, 9, 10, 11))]
    y = np.where(rng.random(x.shape) < 0.6, x, r[rng.integers(0, 4, x.shape)])
    mean, ids, per = R.dice_formula(x, y)
    got, gids, gper = label_dice(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), return_per_label=True)
    assert got == mean and gids.tolist() == [0, 7, 300, 2035] and np.array_equal(gper, per)
    assert label_dice(x.astype(np.int64), y.astype(np.int32)) == mean
    top = torch.tensor([0, 65535], dtype=torch.int32, device=DEV)
    assert label_dice(top, top) == 2 / (2 + 1e-5)
    for bad in (torch.tensor([0, 65536], dtype=torch.int32), torch.tensor([0, -1], dtype=torch.int16),
                torch.tensor([3, 2 ** 40], dtype=torch.int64)):
        with pytest.raises(ValueError, match="label ids"):
            label_dice(bad.to(DEV), torch.zeros_like(bad).to(DEV))
        with pytest.raises(ValueError, match="label ids"):
            label_dice(torch.zeros_like(bad).to(DEV), bad.to(DEV))
    many = torch.arange(4097, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="4096"):
        label_dice(many, many)
    assert label_dice(many[:4096], many[:4096]) == pytest.approx(1.0, abs=1e-4)      # 2 / (2 + 1e-5) per label
    with pytest.raises(ValueError):
        label_dice(many, many[:4096])
    with pytest.raises(TypeError):
        label_dice(many.float(), many.float())


# ------------------------------------------------------------------------------------------------- the README's figure
def test_rotation_round_trip_figure():
    """A 32^3 map (ball, shell, half shell) rotated by +17 degrees about z and back through io.apply_mat: the "label" round trip
    equals the restatement's map exactly; the Dice of both round trips against the original is printed (README: on an MI355X
    0.9818 and 152 voxels changed with "label", 0.9772 and 208 with "nearest")."""
    from keymorph_amd import ops
    from keymorph_amd.io import apply_mat
    from keymorph_amd.loss_ops import label_dice
    lab = R.ball_shells(32)
    x = torch.from_numpy(lab).to(DEV)
    mats = [torch.from_numpy(R.rotation_z(d)).to(DEV) for d in (17.0, -17.0)]
    want = lab
    for m in mats:
        want, _ = R.vote(want, _np(ops.affine_grid(m, (32, 32, 32))))
    figures = {}
    for mode in ("label", "nearest"):
        back = x if mode == "label" else x.float()
        for m in mats:
            back = apply_mat(back, m, mode)
        back = back.to(torch.uint8)
        _, ids, per = label_dice(back, x, return_per_label=True)
        figures[mode] = (float(per[ids > 0].mean()), int((back != x).sum()))
        print(f"round trip +-17 degrees, {mode}: mean Dice of labels 1-3 {figures[mode][0]:.4f}, "
              f"{figures[mode][1]} of {x.numel()} voxels changed")
        if mode == "label":
            assert np.array_equal(_np(back), want)
