"""CPU: the restatement of the trilinear label vote (tests/labelwarp_ref.py) is itself pinned -- against torch's CPU sampler run
on the one-hot volume (argmax over the channels, and their maximum), against the tie rule on ties made by construction, and by
the properties of the definition (relabelling commutes, the identity grid returns the input) -- and label_dice's host arithmetic
against the reference's formula on counts.

Equality with torch is required.  torch's kernel may add a voxel's eight terms in another association than the sampler's fma
chain, so a different label is tolerated only where the float64 margin between the winner and the best other label is under
1e-5 (ten times the float32 rounding of eight terms of size <= 1 is 8 * 6e-8 ~ 5e-7), only in the interior, outside, lattice
and border sets, and in at most 0.5 % of a set's voxels.  The halfway set is all ties and near ties: it is compared with torch
only where every weight is an exact eighth, so that any correct evaluation agrees, and checked against the tie rule by
construction elsewhere."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import labelwarp_ref as R
from tests import sampler_ref as S

VOLUMES = [((2, 1, 5, 6, 7), 4), ((2, 1, 4, 8, 8), 4), ((1, 1, 3, 40, 67), 3)]


def torch_chain(lab, grid, nlab):
    oh = F.one_hot(torch.from_numpy(lab[:, 0].astype(np.int64)), nlab).permute(0, 4, 1, 2, 3).float()
    out = F.grid_sample(oh, torch.from_numpy(grid), mode="bilinear", padding_mode="border", align_corners=False)
    w, l = out.max(1, keepdim=True)
    return torch.argmax(out, 1, keepdim=True).numpy(), w.numpy()


# the halfway set only on the power-of-two volume, where every weight is an exact eighth
TORCH_CASES = [(shape, nlab, name) for shape, nlab in VOLUMES for name in R.SETS
               if name != "halfway" or shape == (2, 1, 4, 8, 8)]


@pytest.mark.parametrize("shape,nlab,name", TORCH_CASES, ids=["x".join(map(str, s[2:])) + "-" + n for s, _, n in TORCH_CASES])
def test_restatement_against_torch_cpu(shape, nlab, name):
    lab = R.random_labels(shape, nlab, seed=7)
    grid = R.coordinate_set(name, shape[0], shape[2:])
    got, w = R.vote(lab, grid)
    ref, wref = torch_chain(lab, grid, nlab)
    _, _, margin = R.vote64(lab, grid)
    differ = got != ref
    print(f"{shape} {name}: {int(differ.sum())} of {differ.size} labels differ, "
          f"{int((w != wref).sum())} weights differ, max |dw| {np.abs(w - wref).max():.3e}")
    if name == "halfway":
        assert not differ.any()
        assert np.array_equal(w, wref)
        return
    assert (margin[differ] < 1e-5).all(), f"labels differ at margins up to {margin[differ].max():.3e}"
    assert differ.mean() <= 0.005
    assert np.array_equal(w[~differ], wref[~differ])


@pytest.mark.parametrize("parity", ["x", "xyz"])
def test_tie_rule_by_construction(parity):
    """(2, 5, 6, 7) volumes with two labels per cell, four corners each, sampled where all eight weights are exactly 1/8: both
    sums are exactly 1/2 and the smaller label has to win"""
    N, D, H, W = 2, 5, 6, 7
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    par = (x if parity == "x" else x + y + z) % 2
    pairs = [(3, 1), (0, 2)]
    lab = np.stack([np.where(par == 0, a, b) for a, b in pairs])[:, None].astype(np.int64)
    rng = np.random.default_rng(3)
    pts = [R.exact_halfway(s) for s in (W, H, D)]
    assert all(len(p) >= 2 for p in pts)
    grid = np.empty((N,) + R.OUT_SHAPE + (3,), np.float32)
    for k in range(3):
        grid[..., k] = rng.choice(pts[k], size=grid.shape[:-1])
    got, w = R.vote(lab, grid)
    for n, (a, b) in enumerate(pairs):
        assert (got[n] == min(a, b)).all()
    assert (w == np.float32(0.5)).all()


def test_halfway_set_is_ties_and_near_ties():
    """what the halfway set is for: a large share of its voxels have a float64 margin of (nearly) nothing, and where the float32
    and the float64 vote disagree at all, the margin is within float32 rounding"""
    for shape, nlab in VOLUMES:
        lab = R.random_labels(shape, nlab, seed=7)
        grid = R.coordinate_set("halfway", shape[0], shape[2:])
        a, _ = R.vote(lab, grid)
        b, _, margin = R.vote64(lab, grid)
        print(f"{shape}: {100 * (np.abs(margin) < 1e-5).mean():.1f} % near ties, {int((a != b).sum())} float32/float64 disagreements")
        assert (np.abs(margin) < 1e-5).mean() > 0.1
        assert (np.abs(margin[a != b]) < 1e-5).all()


@pytest.mark.parametrize("dtype,ids", [(np.int16, [0, 7, 300, 2035]), (np.int32, [-5, 0, 70000, 2 ** 31 - 1]),
                                       (np.int64, [-2 ** 40, 0, 3, 2 ** 40]), (np.uint8, [0, 1, 200, 255])])
def test_relabelling_commutes(dtype, ids):
    lab = R.random_labels((2, 3, 5, 6, 7), 4, seed=11)
    r = np.array(ids, dtype)
    for name in ("outside", "halfway"):
        grid = R.coordinate_set(name, 2, (5, 6, 7))
        a, wa = R.vote(r[lab], grid)
        b, wb = R.vote(lab, grid)
        assert a.dtype == dtype
        assert np.array_equal(a, r[b]) and np.array_equal(wa, wb)


def test_identity_and_shift():
    lab = R.random_labels((2, 2, 5, 6, 7), 5, seed=13, dtype=np.int32)
    g = S.identity(2, (5, 6, 7))
    got, w = R.vote(lab, g)
    assert np.array_equal(got, lab) and (w > 0.999).all()      # (the fp32 centres of sizes 5, 6, 7 are an ulp off the lattice)
    got, _ = R.vote(lab, S.shift(g, (5, 6, 7), (2, -1, 1)))
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(7), indexing="ij")
    want = lab[:, :, np.clip(z + 1, 0, 4), np.clip(y - 1, 0, 5), np.clip(x + 2, 0, 6)]
    assert np.array_equal(got, want)


def test_label_dice_host_arithmetic():
    from keymorph_amd.loss_ops import _dice_per_label
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, 6, 500), rng.integers(0, 6, 500)
    y[y == 4] = 0                                              # a label present in one map only
    mean, labels, per = R.dice_formula(x, y)
    cx, cy, cxy = (np.array([f(l) for l in labels], np.int64) for f in
                   (lambda l: (x == l).sum(), lambda l: (y == l).sum(), lambda l: ((x == l) & (y == l)).sum()))
    got = _dice_per_label(cx, cy, cxy)
    assert np.array_equal(got, per) and float(np.mean(got)) == mean
    assert per[list(labels).index(4)] == 0
    one = _dice_per_label(np.array([9]), np.array([9]), np.array([9]))      # one label: dice(), exactly 1
    assert one.tolist() == [1.0]
