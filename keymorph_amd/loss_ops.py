"""Losses with the reference's call surface (keymorph/loss_ops.py:9-63), HIP underneath."""
import math

import numpy as np
import torch

from . import ops


class MSELoss(torch.nn.Module):
    """keymorph/loss_ops.py:9-13"""

    def forward(self, pred, target):
        return ops.mse_loss(pred, target)


class DiceLoss(torch.nn.Module):
    """Soft / hard Dice loss (lower is better), keymorph/loss_ops.py:16-63.

    eps = 1 is added to numerator and denominator; the denominator uses squared sums.
    """

    def __init__(self, hard=False, return_regions=False):
        super().__init__()
        self.hard = hard
        self.return_regions = return_regions

    def forward(self, pred, target, ign_first_ch=False):
        assert pred.size() == target.size(), "Input and target are different dim"
        assert target.dim() in (4, 5)
        n, c = target.shape[:2]
        target = target.contiguous().view(n, c, -1)
        pred = pred.contiguous().view(n, c, -1)
        if self.hard:
            pred = ops.argmax_onehot(pred)
        if ign_first_ch:
            target = target[:, 1:, :]
            pred = pred[:, 1:, :]
            c -= 1
        v = target.shape[-1]
        rows = ops.dice_rows(pred.reshape(n * c, v), target.reshape(n * c, v)).view(n, c)
        if self.return_regions:
            return rows.mean(0)
        return rows.mean()


def warp_dice_loss(grid, seg_m, seg_f, ign_first_ch=False, return_regions=False):
    """`DiceLoss(return_regions=...)(align_img(grid, seg_m), seg_f, ign_first_ch)` -- the Dice branch of
    scripts/train.py:146-164 -- as ONE fused operator: the warped segmentation is never materialised (forward: one pass
    over grid + both segmentations; backward: one more pass that writes d(loss)/d(grid)).  Falls back to exactly that
    composition when the fused kernels do not apply (seg_m needing a gradient, 4-D inputs, > 128 channels)."""
    if not ops.warp_dice_ok(seg_m, grid) or seg_f.requires_grad:
        from .utils import align_img
        return DiceLoss(return_regions=return_regions)(align_img(grid, seg_m), seg_f, ign_first_ch=ign_first_ch)
    rows = ops.warp_dice_rows(seg_m, grid, seg_f)
    if ign_first_ch:
        rows = rows[:, 1:]
    return rows.mean(0) if return_regions else rows.mean()


# --------------------------------------------------------------------------
# eval-only metrics on the GPU (keymorph/loss_ops.py:161-247; callers pairwise_register_eval.py:332-345)
# --------------------------------------------------------------------------
def _jacdet(disp, want_map):
    from . import _lib
    from .ops import _p, _reduce_ws, _stream, check
    lib = _lib.load()
    assert disp.dim() == 5 and disp.shape[0] == 1 and disp.shape[1] == 3, "expected a (1, 3, D, H, W) map"
    if disp.dtype != torch.float32 or not disp.is_cuda:
        raise _lib.KeymorphHipError("jacobian determinant: expected a float32 tensor on the GPU")
    _, _, D, H, W = disp.shape
    st = disp.stride()
    if st[2:] == (H * W * st[4], W * st[4], st[4]) and st[4] in (1, 3) and (st[1] == 1 or st[1] == D * H * W):
        src, cs, vs = disp, st[1], st[4]          # NCDHW, or the permuted view of a (1, D, H, W, 3) grid: no copy
    else:
        src = disp.contiguous()
        cs, vs = D * H * W, 1
    jd = torch.empty((D - 4, H - 4, W - 4), dtype=torch.float32, device=disp.device) if want_map else None
    stats = torch.empty(4, dtype=torch.float64, device=disp.device)
    check(lib.kmh_jacobian_det(_p(src), cs, vs, D, H, W, _p(jd), _p(stats), _p(_reduce_ws(disp.device)), _stream()),
          "kmh_jacobian_det")
    return jd, stats


def _jacobian_determinant(disp):
    """(1, 3, D, H, W) -> (D-4, H-4, W-4) determinants of d(disp)/d(z,y,x) + I (loss_ops.py:161-228)."""
    return _jacdet(disp, True)[0]


def jdstd(disp):
    """Population standard deviation of the Jacobian determinant (loss_ops.py:231-234); Python float."""
    return float(_jacdet(disp, False)[1][1])


def jdlessthan0(disp, as_percentage=False):
    """Number (or fraction) of voxels with a non-positive Jacobian determinant (loss_ops.py:237-242)."""
    st = _jacdet(disp, False)[1]
    return float(st[2] / st[3]) if as_percentage else int(st[2])


# --------------------------------------------------------------------------
# segmentation eval metrics on the GPU (keymorph/loss_ops.py:66-158; callers pairwise_register_eval.py:329-331,
# groupwise_register_eval.py:492-511): csrc/metrics.hip computes the surfaces, distance transforms and label counts
# --------------------------------------------------------------------------
class MetricInputError(TypeError, NotImplementedError):
    """A metric input that is neither a torch tensor nor a numpy array.  A TypeError, as in the reference (`len(None)`),
    and a NotImplementedError, as the placeholder this function replaced raised."""


HAUSDORFF_SAMPLING = (1.25, 1.25, 10.0)     # keymorph/loss_ops.py:157, spacing along array axes (D, H, W)
_HD_DTYPES = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3, torch.bool: 4, torch.uint8: 4,
              torch.int8: 4, torch.int16: 5, torch.int32: 6, torch.int64: 7}


def _on_gpu(x, fn):
    """A tensor or ndarray as a tensor on the current GPU (the reference accepts both, utils._check_type); GPU tensors stay
    where they are."""
    if isinstance(x, np.ndarray):
        if x.dtype.kind == "u" and x.dtype.itemsize > 1:        # same-width signed view: "!= 0" is unchanged
            x = x.view(np.dtype(f"int{8 * x.dtype.itemsize}"))
        x = torch.from_numpy(np.ascontiguousarray(x))
    elif not isinstance(x, torch.Tensor):
        raise MetricInputError(f"{fn}: expected a torch.Tensor or a numpy.ndarray, got {type(x).__name__}")
    x = x.detach()
    dev = torch.cuda.current_device()
    if not x.is_cuda:
        return x.to(torch.device("cuda", dev))
    if x.device.index != dev:
        from ._lib import KeymorphHipError
        raise KeymorphHipError(f"{fn}: input is on {x.device} but the current device is cuda:{dev}")
    return x


def _channel0(x, fn):
    """Channel 0 of a (bs, C, D, H, W) input on the GPU, read in place where the layout allows it (no copy of C channels)."""
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        raise MetricInputError(f"{fn}: expected a torch.Tensor or a numpy.ndarray, got {type(x).__name__}")
    if x.ndim != 5:
        raise ValueError(f"{fn}: expected a (bs, C, D, H, W) segmentation, got shape {tuple(x.shape)}")
    t = _on_gpu(x[:, 0], fn)
    if t.dtype not in _HD_DTYPES:
        raise TypeError(f"{fn}: unsupported dtype {t.dtype}")
    if t.shape[0] > 0 and not t[0].is_contiguous():
        t = t.contiguous()
    return t


def hausdorff_distance(test_seg, gt_seg, sampling=HAUSDORFF_SAMPLING):
    """Hausdorff distance between the surfaces of channel 0 ("brain surface") of two (bs, C, D, H, W) segmentations,
    averaged over the batch (keymorph/loss_ops.py:121-158); a Python float.

    A voxel is set iff its value != 0 (NaN included), the surface is the set minus its 6-neighbour erosion with a zero
    border, and `sampling` weights the array axes (D, H, W).  The reference's sampling makes every squared distance an exact
    multiple of 1/16, so the value equals the reference's bit for bit.  Differences from the reference: if exactly one
    surface of a sample is empty the sample's distance is inf (the reference returns a number left over from scipy's
    feature transform); both empty raises ValueError (the reference's max() of an empty array)."""
    from . import _lib
    from .ops import _p, _stream, check
    a = _channel0(test_seg, "hausdorff_distance")
    b = _channel0(gt_seg, "hausdorff_distance")
    if a.shape != b.shape:
        raise ValueError(f"hausdorff_distance: shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    N, D, H, W = a.shape
    sq = []
    if N > 0:
        lib = _lib.load()
        ws = torch.empty(int(lib.kmh_hausdorff3d_ws_bytes(D, H, W)), dtype=torch.uint8, device=a.device)
        out = torch.empty(N, dtype=torch.float64, device=a.device)
        sz, sy, sx = (float(v) for v in sampling)
        check(lib.kmh_hausdorff3d(_p(a), _p(b), _HD_DTYPES[a.dtype], _HD_DTYPES[b.dtype], a.stride(0), b.stride(0), N, D, H,
                                  W, sz, sy, sx, _p(ws), _p(out), _stream()), "kmh_hausdorff3d")
        sq = out.cpu().tolist()
    hd = 0
    for i, v in enumerate(sq):
        if v != v:
            raise ValueError(f"hausdorff_distance: sample {i}: both surfaces are empty")
        hd += math.sqrt(v)
    return hd / N


def surface_distance_map_sq(seg, sampling=HAUSDORFF_SAMPLING):
    """Squared distance from every voxel to the surface of `seg != 0` ((D, H, W) tensor or array), the map
    hausdorff_distance reduces; fp64 on the GPU, +inf everywhere if the surface is empty."""
    from . import _lib
    from .ops import _p, _stream, check
    if not isinstance(seg, (torch.Tensor, np.ndarray)) or seg.ndim != 3:
        raise ValueError("surface_distance_map_sq: expected a (D, H, W) tensor or array")
    t = _channel0(seg[None, None], "surface_distance_map_sq")[0].contiguous()
    D, H, W = t.shape
    lib = _lib.load()
    ws = torch.empty(int(lib.kmh_edt3d_sq_ws_bytes(D, H, W)), dtype=torch.uint8, device=t.device)
    out = torch.empty((D, H, W), dtype=torch.float64, device=t.device)
    sz, sy, sx = (float(v) for v in sampling)
    check(lib.kmh_edt3d_sq(_p(t), _HD_DTYPES[t.dtype], D, H, W, sz, sy, sx, _p(ws), _p(out), _stream()), "kmh_edt3d_sq")
    return out


def _label_counts(x, y, fn, binary):
    """(|x = l|, |y = l|, |x = l and y = l|) per label as int64 numpy arrays, counted on the GPU."""
    from . import _lib
    from .ops import _p, _stream, check
    tx, ty = _on_gpu(x, fn), _on_gpu(y, fn)
    assert tx.shape == ty.shape, "both inputs should have same size, had {} and {}".format(tuple(tx.shape), tuple(ty.shape))
    if binary:
        for t in (tx, ty):
            if t.dtype != torch.bool and bool(((t != 0) & (t != 1)).any()):
                raise ValueError(f"{fn}: expected 0/1 inputs")
        tx, ty = ((t.view(torch.uint8) if t.dtype == torch.bool else (t != 0).to(torch.uint8)).contiguous() for t in (tx, ty))
        N, C, V, dt = 1, 0, tx.numel(), 0
    else:
        if tx.dim() < 2:
            raise ValueError(f"{fn}: expected (bs, C, ...) inputs")
        # exact conversions only: argmax ties and order are those of the original values
        wide = torch.float64 if tx.dtype in (torch.float64, torch.int32, torch.int64) else torch.float32
        tx, ty = tx.to(wide).contiguous(), ty.to(wide).contiguous()
        N, C = tx.shape[:2]
        V, dt = tx[0, 0].numel(), (1 if wide == torch.float64 else 0)
    nlab = C if C else 2
    counts = torch.zeros(3 * nlab, dtype=torch.int64, device=tx.device)
    if N * V > 0:
        lib = _lib.load()
        check(lib.kmh_label_counts(_p(tx), _p(ty), dt, N, C, V, _p(counts), _stream()), "kmh_label_counts")
    cx, cy, cxy = counts.cpu().numpy().reshape(3, nlab)
    return cx, cy, cxy


def _dice_from_counts(cx, cy, cxy):
    """keymorph/loss_ops.py:109-111 on counts: 2 * sum(x * y) / (sum(x) + sum(y)) (nan for two empty inputs, as numpy)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(2 * np.int64(cxy) / (np.int64(cx) + np.int64(cy)))


def fast_dice(x, y):
    """Mean Dice over the labels present in either channel-argmax map, pooled over the batch (keymorph/loss_ops.py:66-106);
    a Python float equal to the reference's.  Argmax and counts run on the GPU; the arithmetic on the handful of per-label
    counts is the reference's numpy expression.  With one label present this is dice(...) = 1.0, for tensors as for arrays
    (the reference crashes there on torch inputs)."""
    cx, cy, cxy = _label_counts(x, y, "fast_dice", binary=False)
    labels = np.nonzero(cx + cy)[0]
    if len(labels) > 1:
        hx, hy, diag = (c[labels].astype(np.float64) for c in (cx, cy, cxy))
        dice_score = 2 * diag / (hy + hx + 1e-5)
    else:
        l = labels[0]
        dice_score = _dice_from_counts(cx[l], cy[l], cxy[l])
    return float(np.mean(dice_score))


def _label_map(x, fn):
    """An integer label map (tensor or ndarray) on the GPU, contiguous, in one of kmh_warp_labels' element types; an unsigned
    numpy array wider than a byte goes to the next wider signed type first, so that its ids keep their values."""
    if isinstance(x, np.ndarray) and x.dtype.kind == "u" and x.dtype.itemsize in (2, 4):
        x = x.astype(np.dtype(f"int{16 * x.dtype.itemsize}"))
    t = _on_gpu(x, fn)
    if t.dtype == torch.int8:
        t = t.to(torch.int16)
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64):
        raise TypeError(f"{fn}: expected integer label maps (uint8, bool, int16, int32 or int64), got {t.dtype}")
    return t.contiguous()


def _dice_per_label(cx, cy, cxy):
    """fast_dice's arithmetic (keymorph/loss_ops.py:96-106) on the counts of the labels present in either map, in ascending
    label order: 2 |x = l and y = l| / (|y = l| + |x = l| + 1e-5) per label; a single label goes through _dice_from_counts."""
    if len(cx) > 1:
        hx, hy, diag = (np.asarray(c).astype(np.float64) for c in (cx, cy, cxy))
        return 2 * diag / (hy + hx + 1e-5)
    return np.array([_dice_from_counts(cx[0], cy[0], cxy[0])], dtype=np.float64)


def label_dice(x, y, return_per_label=False):
    """fast_dice on two integer label maps themselves: the mean over the labels present in either map of
    2 |x = l and y = l| / (|x = l| + |y = l| + 1e-5), pooled over the whole of both maps; a Python float equal to
    fast_dice(one_hot(x), one_hot(y)) where that can be built.  x, y: tensors or numpy arrays of one shape, uint8, bool, int16,
    int32 or int64, ids in [0, 65536) and at most 4096 distinct ids in the two maps together (ValueError otherwise).  Two passes
    over the maps on the GPU (which ids occur; their counts), no one-hot tensor: label_dice(ops.warp_labels(seg_m, grid), seg_f)
    scores a FreeSurfer-sized map.  return_per_label: (value, labels, dice), the ids (int64) and their Dice (float64) as numpy
    arrays."""
    from . import _lib
    from .ops import LABEL_DTYPES, _p, _stream, check
    from .utils import _MAX_LABEL
    fn = "label_dice"
    tx, ty = _label_map(x, fn), _label_map(y, fn)
    if tx.shape != ty.shape:
        raise ValueError(f"{fn}: shapes differ: {tuple(tx.shape)} vs {tuple(ty.shape)}")
    if tx.numel() == 0:
        raise ValueError(f"{fn}: the label maps are empty")
    if tx.dtype != ty.dtype:
        tx, ty = tx.to(torch.int64), ty.to(torch.int64)
    nbytes, signed = LABEL_DTYPES[tx.dtype]
    lib, n = _lib.load(), tx.numel()
    flags = torch.zeros(_MAX_LABEL + 1, dtype=torch.int32, device=tx.device)
    for t in (tx, ty):
        check(lib.kmh_label_presence_int(_p(t), nbytes, signed, n, _MAX_LABEL, _p(flags), _stream()), "kmh_label_presence_int")
    flags = flags.cpu().numpy()
    if flags[_MAX_LABEL]:
        raise ValueError(f"{fn}: label ids must lie in [0, {_MAX_LABEL})")
    labels = np.nonzero(flags[:_MAX_LABEL])[0].astype(np.int64)
    nlab = len(labels)
    if nlab > 4096:
        raise ValueError(f"{fn}: {nlab} distinct labels in the two maps, at most 4096 are counted")
    slot_of = np.full(_MAX_LABEL, 0xFFFF, dtype=np.uint16)
    slot_of[labels] = np.arange(nlab, dtype=np.uint16)
    slot_of = torch.from_numpy(slot_of.view(np.int16)).to(tx.device)
    counts = torch.zeros(3 * nlab, dtype=torch.int64, device=tx.device)
    check(lib.kmh_label_pair_counts(_p(tx), _p(ty), nbytes, signed, n, _p(slot_of), _MAX_LABEL, nlab, _p(counts), _stream()),
          "kmh_label_pair_counts")
    cx, cy, cxy = counts.cpu().numpy().reshape(3, nlab)
    per_label = _dice_per_label(cx, cy, cxy)
    value = float(np.mean(per_label))
    return (value, labels, per_label) if return_per_label else value


def dice(x, y):
    """2 * sum(x * y) / (sum(x) + sum(y)) of two 0/1 arrays or tensors (keymorph/loss_ops.py:109-111), counted on the GPU;
    a Python float (nan for two empty inputs)."""
    cx, cy, cxy = _label_counts(x, y, "dice", binary=True)
    return _dice_from_counts(cx[1], cy[1], cxy[1])


# --------------------------------------------------------------------------
# groupwise evaluation metrics over files or tensor stacks (keymorph/loss_ops.py:406-551; callers
# scripts/groupwise_register_eval.py:478-515): the pairwise / per-grid averages, HIP losses underneath
# --------------------------------------------------------------------------
def _load_file(path, device=None):
    """loss_ops.py:406-412 (.npy; NIfTI through keymorph_amd.io.read_nifti instead of nibabel); lands on the GPU."""
    import numpy as np
    path = str(path)
    if path.endswith(".nii") or path.endswith(".nii.gz"):
        from .io import read_nifti
        arr = read_nifti(path)[0]
    elif path.endswith(".npy"):
        arr = np.load(path)
    else:
        raise ValueError("File format not supported")
    return torch.tensor(arr).to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))


def _item(batch, i):
    return _load_file(batch[i]) if isinstance(batch[0], (str, bytes)) or hasattr(batch[0], "__fspath__") else batch[i:i + 1]


class _AvgPairwiseLoss(torch.nn.Module):
    """Mean of metric_fn over all unordered pairs (loss_ops.py:415-435)."""

    def __init__(self, metric_fn):
        super().__init__()
        self.metric_fn = metric_fn

    def forward(self, batch_of_imgs):
        loss, num = 0, 0
        for i in range(len(batch_of_imgs)):
            for j in range(i + 1, len(batch_of_imgs)):
                loss = loss + self.metric_fn(_item(batch_of_imgs, i), _item(batch_of_imgs, j))
                num += 1
        return loss / num


class MSEPairwiseLoss(_AvgPairwiseLoss):
    def __init__(self):
        super().__init__(MSELoss().forward)


class SoftDicePairwiseLoss(_AvgPairwiseLoss):
    def __init__(self):
        super().__init__(DiceLoss().forward)


class HardDicePairwiseLoss(_AvgPairwiseLoss):
    def __init__(self):
        super().__init__(DiceLoss(hard=True).forward)


class HausdorffPairwiseLoss(_AvgPairwiseLoss):
    def __init__(self):
        super().__init__(hausdorff_distance)


class MultipleAvgSegPairwiseMetric(torch.nn.Module):
    """Several pairwise segmentation metrics in one sweep over the files (loss_ops.py:499-527)."""

    def __init__(self):
        super().__init__()
        self.name2fn = {"dice": fast_dice,
                        "harddice": DiceLoss(hard=True).forward,
                        "harddiceroi": DiceLoss(hard=True, return_regions=True).forward,
                        "softdice": DiceLoss().forward,
                        "hausd": hausdorff_distance}

    def forward(self, batch_of_imgs, fn_names):
        for name in fn_names:
            if name not in self.name2fn:
                raise NotImplementedError(f"metric '{name}' is not part of the MI355X registration path")
        res, num = {name: 0 for name in fn_names}, 0
        for i in range(len(batch_of_imgs)):
            for j in range(i + 1, len(batch_of_imgs)):
                a, b = _item(batch_of_imgs, i), _item(batch_of_imgs, j)
                for name in fn_names:
                    res[name] = res[name] + self.name2fn[name](a, b)
                num += 1
        return {name: res[name] / num for name in fn_names}


class MultipleAvgGridMetric(torch.nn.Module):
    """Jacobian-determinant metrics averaged over the grids of a group (loss_ops.py:530-551)."""

    def __init__(self):
        super().__init__()
        self.name2fn = {"jdstd": jdstd, "jdlessthan0": jdlessthan0}

    def forward(self, batch_of_grids, fn_names):
        res = {name: 0 for name in fn_names}
        for i in range(len(batch_of_grids)):
            grid = _item(batch_of_grids, i).float()
            gp = grid.permute(0, 4, 1, 2, 3)
            for name in fn_names:
                res[name] += self.name2fn[name](gp)
        return {name: res[name] / len(batch_of_grids) for name in fn_names}


class AvgJDStd(MultipleAvgGridMetric):
    def forward(self, batch_of_grids):
        return super().forward(batch_of_grids, ["jdstd"])["jdstd"]


class AvgJDLessThan0(MultipleAvgGridMetric):
    def forward(self, batch_of_grids):
        return super().forward(batch_of_grids, ["jdlessthan0"])["jdlessthan0"]


# --------------------------------------------------------------------------
# LC2 / ImageLC2 on the GPU (keymorph/loss_ops.py:250-391): csrc/lc2.hip forms the gradient magnitude, the moments, the 3 x 3
# solve and the backward; ImageLC2's patch tiling is index arithmetic inside the kernels (no patch batch is copied)
# --------------------------------------------------------------------------
_LC2_ALPHA, _LC2_BETA = 1e-3, 1e-2          # run()'s defaults, the values forward() uses (loss_ops.py:268, 360)


def _difference_filter():
    """The reference's `f` (loss_ops.py:254-260): channel k holds +1 / -1 taps on either side of the centre along W, H, D, the
    conv3d weight of the central differences whose norm is g.  Kept as the attribute; the kernels apply it implicitly."""
    f = torch.zeros(3, 1, 3, 3, 3)
    for k, (dz, dy, dx) in enumerate(((0, 0, 1), (0, 1, 0), (1, 0, 0))):
        f[k, 0, 1 - dz, 1 - dy, 1 - dx] = 1
        f[k, 0, 1 + dz, 1 + dy, 1 + dx] = -1
    return f


class LC2(torch.nn.Module):
    """LC2 similarity of (bs, 1, S, S, S) pairs with S odd (keymorph/loss_ops.py:250-302), on the GPU: forward() returns the
    per-sample mean of run() over `radiuses`, shape (bs,), float32, differentiable in both inputs.  A radius with
    2r + 1 >= S raises ValueError (the reference's crop is empty there and its reshape fails)."""

    def __init__(self, radiuses=(3, 5, 7)):
        super().__init__()
        self.radiuses = radiuses
        self.f = _difference_filter()

    def forward(self, us, mr):
        return self._volumes(us, mr, tuple(self.radiuses), _LC2_ALPHA, _LC2_BETA)

    def run(self, us, mr, radius=9, alpha=_LC2_ALPHA, beta=_LC2_BETA):
        return self._volumes(us, mr, (radius,), alpha, beta)

    @staticmethod
    def _volumes(us, mr, radii, alpha, beta):
        us, mr = us.squeeze(1), mr.squeeze(1)
        assert us.shape == mr.shape
        assert us.shape[1] == us.shape[2] == us.shape[3]
        assert us.shape[1] % 2 == 1, "Input must be odd size"
        return ops.lc2(us, mr, us.shape[1], radii, alpha, beta)


class ImageLC2(torch.nn.Module):
    """LC2 over non-overlapping patch_size^3 patches of (N, 1, S, S, S) volumes (keymorph/loss_ops.py:305-391), on the GPU:
    S // patch_size patches per axis (the remainder dropped), in (N, nD, nH, nW) order; forward() returns their mean
    (reduction "mean") or the per-patch vector (None), float32, differentiable in both inputs.  The reference's assertions
    are kept, its odd-channel check included; like the reference it works for one channel only (ValueError otherwise)."""

    def __init__(self, patch_size=51, radiuses=(5,), reduction="mean"):
        super().__init__()
        self.patch_size = patch_size
        self.radii = radiuses
        assert reduction in ["mean", None]
        self.reduction = reduction
        self.f = _difference_filter()

    def forward(self, us, mr):
        assert us.shape == mr.shape, f"Input and target have different shapes, {us.shape} vs {mr.shape}"
        assert us.shape[-1] == us.shape[-2] == us.shape[-3], f"Dimensions must be equal, currently {us.shape}"
        assert us.shape[1] % 2 == 1, f"Input must be odd size, currently {us.shape}"
        if us.dim() != 5:
            raise ValueError(f"ImageLC2: expected (N, 1, S, S, S) volumes, got {tuple(us.shape)}")
        return ops.lc2(us, mr, self.patch_size, tuple(self.radii), _LC2_ALPHA, _LC2_BETA, self.reduction == "mean")

    def run(self, us, mr, radius=9, alpha=_LC2_ALPHA, beta=_LC2_BETA):
        """run() on a batch of (B, 1, P, P, P) patches -> (B,)."""
        us, mr = us.squeeze(1), mr.squeeze(1)
        return ops.lc2(us, mr, us.shape[-1], (radius,), alpha, beta)


# --------------------------------------------------------------------------
# mutual information on the GPU (csrc/mi.hip): the intensity similarity between MR modalities (T1 / T2 / PD)
# --------------------------------------------------------------------------
class MILoss(torch.nn.Module):
    """-mean over the batch of the mutual information of (N, 1, D, H, W) float32 pairs (ops.mutual_information: cubic B-spline
    Parzen windows, `bins` bins, per-sample ranges); lower is better, differentiable in both inputs:
    MILoss()(align_img(grid, img_m), img_f) scores or trains a multi-modal alignment.  mask: ops.mutual_information's, the voxels
    that are counted."""

    def __init__(self, bins=32):
        super().__init__()
        self.bins = bins

    def forward(self, pred, target, mask=None):
        return -ops.mutual_information(pred, target, self.bins, mask=mask).mean()


class WarpMILoss(torch.nn.Module):
    """-mean over the batch of ops.warp_mutual_information(moving, fixed, mat, bins, ranges): MILoss of the moving volume warped
    by the (N, 3, 4) matrix `mat` in one fused pass, differentiable in `mat` only.  fixed_mask, moving_mask, inside: the
    operator's, which voxels are counted."""

    def __init__(self, bins=32):
        super().__init__()
        self.bins = bins

    def forward(self, moving, fixed, mat, ranges=None, fixed_mask=None, moving_mask=None, inside=False):
        return -ops.warp_mutual_information(moving, fixed, mat, self.bins, ranges, fixed_mask, moving_mask, inside).mean()


class LNCCLoss(torch.nn.Module):
    """-mean over the batch of ops.local_ncc(pred, target, window, eps): the squared local normalised cross-correlation over
    truncated window^3 cubes of (N, 1, D, H, W) float32 pairs; lower is better, differentiable in both inputs.  The mono-modal
    similarity that survives a smooth bias field: LNCCLoss()(align_img(grid, img_m), img_f)."""

    def __init__(self, window=9, eps=1e-5):
        super().__init__()
        self.window, self.eps = window, eps

    def forward(self, pred, target):
        return -ops.local_ncc(pred, target, self.window, self.eps).mean()


class MINDLoss(torch.nn.Module):
    """Mean over the batch of ops.mind_ssc_loss(pred, target, radius, dilation): the squared distance of the MIND-SSC
    self-similarity context descriptors of (N, 1, D, H, W) float32 pairs; lower is better, differentiable in both inputs.  The
    local similarity for two modalities: MINDLoss()(align_img(grid, img_m), img_f).  The clamp of the descriptor's variance comes
    from the pair it is called on (ops.mind_bounds); a driver that wants it fixed while it warps calls ops.mind_ssc_loss with
    bounds of its own."""

    def __init__(self, radius=1, dilation=2):
        super().__init__()
        self.radius, self.dilation = radius, dilation

    def forward(self, pred, target):
        return ops.mind_ssc_loss(pred, target, self.radius, self.dilation).mean()


class BendingLoss(torch.nn.Module):
    """Mean over the batch of ops.bspline_bending(q): the squared second differences of a (N, 3, Cz, Cy, Cx) control lattice along
    its three axes, the smoothness penalty of a free-form deformation (ops.bspline_grid)."""

    def forward(self, q):
        return ops.bspline_bending(q).mean()
