"""CPU: pins tests/pointwise_ref.py, the fp64 restatement that tests/test_pointwise_edges_gpu.py holds csrc/pointwise.hip against
-- its forward and three gradients against fp64 F.conv3d autograd, the exact generator against its claim (integer results that
float32 holds), the bars against float32 evaluations in other summation orders, the slab count's chain length against every
slab geometry, the power of both arms against a result with one product left out, and the case table against the rows the
kernels' tiling asks for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_ref as R

SMALL = [r for r in R.CASES if r[0] * r[1] < 5000]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _rel(got, truth):
    return float(np.abs(got - truth).max() / max(np.abs(truth).max(), 1e-300))


@pytest.mark.parametrize("row", R.CASES, ids=R.ids())
@pytest.mark.parametrize("bias", [True, False])
def test_restatement_vs_fp64_conv3d_autograd(row, bias):
    """fwd, dgrad, wgrad (dw and db) of the restatement against fp64 F.conv3d and its autograd to 1e-12, with and without bias"""
    N, V, Cin, Cout = row
    c = R.real_case(*row)
    xt = _t(c["x"]).permute(0, 2, 1).reshape(N, Cin, 1, 1, V).requires_grad_(True)
    wt = _t(c["w"]).reshape(Cout, Cin, 1, 1, 1).requires_grad_(True)
    bt = _t(c["b"]).requires_grad_(True) if bias else None
    yt = F.conv3d(xt, wt, bt)
    yt.backward(_t(c["dy"]).reshape(N, Cout, 1, 1, V))
    b = c["b"] if bias else None
    assert _rel(R.fwd(c["x"], c["w"], b), yt.detach().numpy().reshape(N, Cout, V)) <= 1e-12
    assert _rel(R.dgrad(c["dy"], c["w"]), xt.grad.numpy().reshape(N, Cin, V).transpose(0, 2, 1)) <= 1e-12
    dw, db = R.wgrad(c["dy"], c["x"])
    assert _rel(dw, wt.grad.numpy().reshape(Cout, Cin)) <= 1e-12
    if bias:
        assert _rel(db, bt.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("row", R.CASES, ids=R.ids())
def test_exact_generator_is_exact(row):
    """integer inputs in [-8, 8], every sum of |products| below 2^24 (bias and pre-filled gradients included): the fp64 results
    are integers that float32 holds, and a float32 evaluation in numpy's own order returns them bit for bit"""
    c = R.exact_case(*row)
    for k, v in c.items():
        assert v.dtype == np.float32 and np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 8, k
    assert R.worst_sums(c) < 2.0 ** 24
    dw, db = R.wgrad(c["dy"], c["x"])
    outs = {"y": R.fwd(c["x"], c["w"], c["b"]), "y nobias": R.fwd(c["x"], c["w"], None), "dx": R.dgrad(c["dy"], c["w"]),
            "dw": dw, "db": db, "dw acc": dw + c["dw0"], "db acc": db + c["db0"]}
    for k, v in outs.items():
        assert np.array_equal(v, np.rint(v)) and np.array_equal(v.astype(np.float32).astype(np.float64), v), k
        assert not np.signbit(v[v == 0]).any(), k                                  # sums from +0: no -0.0
    y32 = np.matmul(c["w"][None], c["x"].transpose(0, 2, 1)) + c["b"][None, :, None]
    assert y32.dtype == np.float32 and np.array_equal(y32, outs["y"].astype(np.float32))


@pytest.mark.parametrize("row", R.CASES, ids=R.ids())
def test_bars_are_positive_and_hold_for_float32_in_other_orders(row):
    """every bar is positive everywhere, and float32 evaluations of the real arm in numpy's own (blocked, fused) order and in
    plain sequential order stay under it -- the bars are upper bounds of fp32 arithmetic, whatever the order"""
    N, V, Cin, Cout = row
    c = R.real_case(*row)
    x, w, b, dy = c["x"], c["w"], c["b"], c["dy"]
    bars = {"y": R.fwd_bar(x, w, b), "y nobias": R.fwd_bar(x, w, None), "dx": R.dgrad_bar(dy, w)}
    bars["dw"], bars["db"] = R.wgrad_bar(dy, x)
    for k, v in bars.items():
        assert np.isfinite(v).all() and (v > 0).all(), k
    bw_acc, bb_acc = R.wgrad_bar(dy, x, acc0=(c["dw0"], c["db0"]))
    assert (bw_acc >= bars["dw"]).all() and (bb_acc >= bars["db"]).all() and (bw_acc > bars["dw"]).any()
    if N * V > 5000:
        return
    y32 = np.matmul(w[None], x.transpose(0, 2, 1)) + b[None, :, None]
    assert (np.abs(y32 - R.fwd(x, w, b)) <= bars["y"]).all()
    seq = np.zeros((N, Cout, V), np.float32)
    for ci in range(Cin):
        seq = seq + w[None, :, ci, None] * x[:, None, :, ci]
    assert (np.abs(seq + b[None, :, None] - R.fwd(x, w, b)) <= bars["y"]).all()
    dx32 = np.matmul(dy.transpose(0, 2, 1), w[None])
    assert (np.abs(dx32 - R.dgrad(dy, w)) <= bars["dx"]).all()
    d32 = dy.transpose(1, 0, 2).reshape(Cout, N * V)
    dw, db = R.wgrad(dy, x)
    assert (np.abs(d32 @ x.reshape(N * V, Cin) - dw) <= bars["dw"]).all()
    assert (np.abs(np.cumsum(d32, 1, dtype=np.float32)[:, -1] - db) <= bars["db"]).all()


def test_slab_chain_length_covers_every_slab_geometry():
    """wgrad_terms(N, V, nslab) is at least the number of voxels in the longest slab for EVERY way of cutting N V voxels into
    nslab equal slabs with a shorter, non-empty last one -- whatever rule the library picks its slab length by"""
    for tot in list(range(1, 300)) + [600, 771, 4097, 20001]:
        for L in sorted({1, 2, 3, 63, 64, 65, 128, 192, 256, tot // 3 + 1, tot // 2 + 1, tot - 1, tot, tot + 5} - {0, -1}):
            nslab = -(-tot // L)
            assert R.wgrad_terms(1, tot, nslab) >= min(tot, L), (tot, L, nslab)
            assert R.wgrad_terms(1, tot, nslab) <= tot
    assert R.wgrad_terms(3, 6667, None) == 20001 and R.wgrad_terms(3, 6667, 1) == 20001


def _droppable(c):
    """the last (n, v, ci, co) in scan order whose three products are all non-zero"""
    x, w, dy = c["x"], c["w"], c["dy"]
    N, V, Cin = x.shape
    Cout = w.shape[0]
    for n in range(N - 1, -1, -1):
        for v in range(V - 1, -1, -1):
            for co in range(Cout - 1, -1, -1):
                for ci in range(Cin - 1, -1, -1):
                    if x[n, v, ci] != 0 and w[co, ci] != 0 and dy[n, co, v] != 0:
                        return n, v, ci, co
    return None


@pytest.mark.parametrize("row", R.CASES, ids=R.ids())
def test_one_missing_term_is_seen_by_both_arms(row):
    """a result with the product of ONE (n, v, ci, co) left out -- the last one of the ragged corner, and one in the middle --
    differs from the truth in the exact arm (whose comparison is bit equality), and in the real arm leaves the forward and
    data-gradient bars by a factor of at least 4 on every row (the smallest factor over the table is printed)"""
    N, V, Cin, Cout = row
    e = R.exact_case(*row)
    t = _droppable(e)
    if t is None:
        assert N * V * Cin * Cout == 1                   # the one-term row may draw a zero factor: then nothing can be dropped
    else:
        y, dx, dw = R.drop_term(e, *t)
        assert not np.array_equal(y.astype(np.float32), R.fwd(e["x"], e["w"], e["b"]).astype(np.float32))
        assert not np.array_equal(dx.astype(np.float32), R.dgrad(e["dy"], e["w"]).astype(np.float32))
        assert not np.array_equal(dw.astype(np.float32), R.wgrad(e["dy"], e["x"])[0].astype(np.float32))
    c = R.real_case(*row)
    worst = np.inf
    for n, v, ci, co in ((N - 1, V - 1, Cin - 1, Cout - 1), (N // 2, V // 2, Cin // 2, Cout // 2), (0, 0, 0, 0)):
        y, dx, _ = R.drop_term(c, n, v, ci, co)
        fy = np.abs(y - R.fwd(c["x"], c["w"], c["b"])) / R.fwd_bar(c["x"], c["w"], c["b"])
        fx = np.abs(dx - R.dgrad(c["dy"], c["w"])) / R.dgrad_bar(c["dy"], c["w"])
        assert np.count_nonzero(fy) == 1 and np.count_nonzero(fx) == 1
        worst = min(worst, float(fy.max()), float(fx.max()))
    print(f"{row}: a missing term leaves the bar by a factor of at least {worst:.1f}")
    assert worst >= 4.0


def test_real_generator_spreads_channel_scales():
    """the channels of x span about 2^12 in scale, and pairing a term with the NEIGHBOURING channel's weight is far outside
    the bar: the compensating scales cancel in the correct pairing only"""
    row = (1, 33, 200, 257)
    c = R.real_case(*row)
    rms = np.sqrt((c["x"].astype(np.float64) ** 2).mean((0, 1)))
    assert 2.0 ** 11 <= rms.max() / rms.min() <= 2.0 ** 13
    wrong = R.fwd(c["x"], np.roll(c["w"], 1, axis=1), c["b"])
    assert (np.abs(wrong - R.fwd(c["x"], c["w"], c["b"])) > 4 * R.fwd_bar(c["x"], c["w"], c["b"])).all()


def test_case_table_holds_every_required_row():
    assert 18 <= len(R.CASES) <= 22 and len(set(R.CASES)) == len(R.CASES)
    for k, col in (("N", 0), ("V", 1), ("Cin", 2), ("Cout", 3)):
        have = {r[col] for r in R.CASES}
        assert set(R.REQUIRED[k]) <= have, (k, sorted(set(R.REQUIRED[k]) - have))
    for name, pred in R.REQUIRED_ROWS.items():
        assert any(pred(*r) for r in R.CASES), name
    for rows in (R.AUTOGRAD_ROWS, (R.CONTAINMENT_ROW,)):
        assert set(rows) <= set(R.CASES)
    biggest = max(4 * max(N * V * Cin, N * V * Cout, Cin * Cout) for N, V, Cin, Cout in R.CASES)
    assert biggest <= 5.5e6, biggest
    assert len(SMALL) == len(R.CASES) - 1
