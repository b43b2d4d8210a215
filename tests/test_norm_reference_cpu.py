"""CPU: pins tests/norm_ref.py, the fp64 restatement that tests/test_norm_edges_gpu.py holds csrc/norm.hip against -- its forward
and gradients against fp64 torch autograd, its pooling against F.max_pool3d bit for bit, nearest_src against F.interpolate,
the statistics bars against a float32 emulation of the kernel's summation order, the cancellation floor of the coefficient
formulas against long double, and every data generator against the class it claims."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as R

POOL_SHAPES = [(2, 2, 2), (4, 6, 10), (7, 5, 9), (3, 2, 2)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _rel(got, truth):
    return float(np.abs(got - truth).max() / max(np.abs(truth).max(), 1e-300))


def _ncdhw(x):          # (D, H, W, C) -> (1, C, D, H, W)
    return _t(x).permute(3, 0, 1, 2)[None]


# ------------------------------------------------------------------------------------------- restatement vs autograd
@pytest.mark.parametrize("C,G", [(8, 8), (12, 4), (16, 1), (96, 8)])
@pytest.mark.parametrize("affine", [True, False])
def test_group_norm_restatement_vs_autograd(C, G, affine):
    """statistics -> coefficients -> apply and back, each formula of the restatement, against fp64 F.group_norm autograd"""
    N, V = 3, 45
    c = R.coeff_case(C, G, N, V, affine)
    x, dy, gamma, beta = c["x"], c["dxn"], c["gamma"], c["beta"]
    xt = _t(x).permute(0, 2, 1).requires_grad_(True)                                       # (N, C, V)
    gt = None if gamma is None else _t(gamma).requires_grad_(True)
    bt = None if beta is None else _t(beta).requires_grad_(True)
    yt = F.group_norm(xt, G, gt, bt, R.EPS)
    yt.backward(_t(dy).permute(0, 2, 1))
    mr = np.stack([R.gn_fwd_coeffs(c["stats"][n], gamma, beta, G, V)[2] for n in range(N)])
    c123, dgamma, dbeta = R.gn_bwd_coeffs(c["ab"], gamma, mr, G, V)
    for n in range(N):
        scale, shift, _ = R.gn_fwd_coeffs(c["stats"][n], gamma, beta, G, V)
        y, _ = R.norm_apply(x[n], scale, shift, False)
        dx, _ = R.gn_bwd_apply(dy[n], x[n], c123[n], False)
        assert _rel(y, yt[n].detach().numpy().T) <= 1e-12
        assert _rel(dx, xt.grad[n].numpy().T) <= 1e-12
        ch = R.chain_bars(x[n], dy[n], gamma, beta, G)                                     # the propagation's own values
        assert _rel(ch["y"].v, y) <= 1e-12 and _rel(ch["dx"].v, dx) <= 1e-12 and (ch["dx"].e > 0).all()
    if affine:
        assert _rel(dgamma, gt.grad.numpy()) <= 1e-12 and _rel(dbeta, bt.grad.numpy()) <= 1e-12
        ds, bh = R.fold_inputs(c["ab"], gamma, beta, mr, G)
        f123, fdg, fdb = R.gn_bwd_coeffs_fold(ds, bh, gamma, beta, mr, G, V)
        assert _rel(f123, c123) <= 1e-12 and _rel(fdg, dgamma) <= 1e-12 and _rel(fdb, dbeta) <= 1e-12


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape,C", [((6, 4, 10), 4), ((2, 2, 2), 12), ((6, 4, 10), 3)])
@pytest.mark.parametrize("quantised", [False, True])
def test_in_bwd_restatement_vs_autograd(pool, shape, C, quantised):
    """in_bwd against fp64 autograd of ReLU(IN(z)) and MaxPool(ReLU(IN(z))); the quantised volume makes torch's winner rule
    part of the answer"""
    z = R.kink_free(shape, C, 5, quantised)
    ush = tuple(s // 2 for s in shape) if pool else shape
    du = np.random.default_rng(3).standard_normal(ush + (C,)).astype(np.float32)
    zt = _ncdhw(z).requires_grad_(True)
    u = F.relu(F.instance_norm(zt, eps=R.EPS))
    if pool:
        u = F.max_pool3d(u, 2)
    u.backward(_ncdhw(du))
    truth = zt.grad[0].permute(1, 2, 3, 0).numpy()
    assert _rel(R.in_bwd(z, du, pool), truth) <= 1e-12


# ----------------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("cls", R.POOL_CLASSES)
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool2_and_scatter_are_torch_bit_for_bit(cls, shape):
    for C in (1, 3):
        x = R.pool_data(cls, shape, C).astype(np.float64)
        D, H, W = shape
        xt = _ncdhw(x).requires_grad_(True)
        yt, it = F.max_pool3d(xt, 2, return_indices=True)
        y, arg = R.maxpool2(x)
        assert np.array_equal(_bits(y), _bits(yt[0].detach().permute(1, 2, 3, 0).numpy()))
        k = arg.astype(np.int64)
        zo, yo, xo = np.meshgrid(*(np.arange(s // 2) for s in shape), indexing="ij")
        flat = ((2 * zo[..., None] + (k >> 2)) * H + 2 * yo[..., None] + ((k >> 1) & 1)) * W + 2 * xo[..., None] + (k & 1)
        assert np.array_equal(flat, it[0].permute(1, 2, 3, 0).numpy())
        dy = np.random.default_rng(1).standard_normal(y.shape)
        yt.backward(_ncdhw(dy))
        dx = R.maxpool2_scatter(dy, arg, shape)
        assert np.array_equal(_bits(dx), _bits(xt.grad[0].permute(1, 2, 3, 0).numpy()))
        assert (dx[2 * (D // 2):] == 0).all() and (dx[:, 2 * (H // 2):] == 0).all() and (dx[:, :, 2 * (W // 2):] == 0).all()


def test_pool_generators_sit_in_their_class():
    for shape in POOL_SHAPES:
        for C in (1, 4):
            w = lambda cls: R._windows(R.pool_data(cls, shape, C))                     # noqa: E731
            a = w("all_equal")
            assert (a == a[:, :, :, :1]).all()
            r = w("relu")
            assert (r >= 0).all() and ((r == 0).sum(3) >= 2).all() and (r.max(3) == 0).any()
            i = w("neg_inf")
            assert np.isneginf(i).any() and np.isneginf(i).all(3).any()
            assert (w("all_negative") < 0).all()
            assert np.isnan(w("nan_first")[:, :, :, 0]).all() and not np.isnan(w("nan_first")[:, :, :, 1:]).any()
            assert np.isnan(w("nan_middle")[:, :, :, 3]).all() and np.isnan(w("nan_last")[:, :, :, 7]).all()
            fl = w("nan_first_last")
            assert np.isnan(fl[:, :, :, 0]).all() and np.isnan(fl[:, :, :, 7]).all()
            assert (R.maxpool2(R.pool_data("nan_first_last", shape, C))[1] == 7).all()       # the LAST NaN wins: position, not value
            assert (R.maxpool2(R.pool_data("all_equal", shape, C))[1] == 0).all()            # the FIRST of equals wins


# ------------------------------------------------------------------------------------------------------------ nearest
def test_nearest_src_is_atens_legacy_nearest():
    pairs = R.nearest_pairs()
    assert len(pairs) == sum(i + 2 for i in range(1, 18))
    for n_in, n_out in pairs:
        src = F.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None], size=n_out, mode="nearest")[0, 0].numpy()
        assert np.array_equal(R.nearest_src(np.arange(n_out), n_in, n_out), src.astype(np.int64)), (n_in, n_out)


def test_upcat_restatement_vs_autograd():
    r = np.random.default_rng(0)
    skip, low = r.standard_normal((5, 7, 3, 2)), r.standard_normal((2, 3, 3, 4))
    st, lt = _ncdhw(skip).requires_grad_(True), _ncdhw(low).requires_grad_(True)
    out = torch.cat([st, F.interpolate(lt, size=(5, 7, 3), mode="nearest")], 1)
    assert np.array_equal(R.upcat(skip, low), out[0].detach().permute(1, 2, 3, 0).numpy())
    g = r.standard_normal((5, 7, 3, 6))
    out.backward(_ncdhw(g))
    dskip, dlow, mag = R.upcat_bwd(g, 2, (2, 3, 3))
    assert np.array_equal(dskip, st.grad[0].permute(1, 2, 3, 0).numpy())
    assert _rel(dlow, lt.grad[0].permute(1, 2, 3, 0).numpy()) <= 1e-14 and (mag >= np.abs(dlow) - 1e-12).all()


# --------------------------------------------------------------------------------------------------- statistics bars
def test_stats_geometry_is_the_launch():
    assert R.stats_geometry(333, 3) == (1, 3, 85, 1, 333) and R.stats_geometry(333, 260)[1:3] == (65, 3)
    assert R.stats_geometry(333, 512)[2] == 2 and R.stats_geometry(333, 516)[2] == 1 and R.stats_geometry(333, 1024)[2] == 1
    assert R.stats_geometry(2049, 8)[3:] == (2, 1025) and R.stats_geometry(*R.STAT_V_CAP)[3:] == (512, 2049)
    for C in R.STAT_REFUSED_C:
        assert R.stats_geometry(333, C) is None
    assert all(R.stats_geometry(V, C) is not None for V, C in R.STAT_SHAPES)


@pytest.mark.parametrize("V,C", R.STAT_SHAPES, ids=[f"V{v}-C{c}" for v, c in R.STAT_SHAPES])
def test_emulated_kernel_order_stays_inside_the_statistics_bars(V, C):
    """a correct float32 implementation of the kernel's summation order against the bars 64 u sum|a|, 65 u sum a^2, 65 u sum|ab|
    for every data class, both modes; prints the worst ratio (norm_ref's docstring carries the table's maximum)"""
    worst = [0.0, 0.0, 0.0]
    for cls in R.STAT_CLASSES:
        a = R.stat_data(cls, 1, V, C)[0]
        b = R.stat_data("zero_mean", 1, V, C, seed=1)[0] + np.float32(0.5)
        for j, bb in enumerate((None, b)):
            got, truth, bars = R.emulate_stats_fp32(a, bb, V, C), R.channel_sums(a, bb), R.stats_bars(a, bb)
            for i in range(2):
                err = np.abs(got[i] - truth[i])
                assert (err <= bars[i]).all(), (cls, j, i, float((err / np.maximum(bars[i], 1e-300)).max()))
                ratio = float((err[bars[i] > 0] / bars[i][bars[i] > 0]).max()) if (bars[i] > 0).any() else 0.0
                k = 0 if i == 0 else 1 + j
                worst[k] = max(worst[k], ratio)
    print(f"V {V} C {C}: worst error / bar  sum a {worst[0]:.3f}  sum a^2 {worst[1]:.3f}  sum ab {worst[2]:.3f}")


def test_stat_generators_sit_in_their_class():
    for V, C in ((333, 3), (65, 8), (1, 3)):
        a = R.stat_data("const", 2, V, C).astype(np.float64)
        assert (a[..., 0].var(1) == 0).all() and (a[..., 0] == R.CONST_VALUE).all()
        s, ss = R.channel_sums(a[0])
        assert ss[0] / V - (s[0] / V) ** 2 == 0.0                                # exactly, by the kernels' formula too
        r = R.stat_data("relu", 2, V, C)
        assert (r >= 0).all() and (V < 60 or 0.3 < (r == 0).mean() < 0.7)
        o = R.stat_data("outlier", 2, V, C)[..., C - 1]
        assert ((o != 0).sum(1) == 1).all() and o.max() == 1e6
        if V > 60:
            off = R.stat_data("offset100", 2, V, C).astype(np.float64)
            assert abs(off.mean() - 100) < 0.5 and 0.8 < off.std() < 1.2
            big = R.stat_data("big_channel", 2, V, C).astype(np.float64).std((0, 1))
            assert C == 1 or big[C // 2] > 3e3 * np.delete(big, C // 2).max()
            z = R.stat_data("zero_mean", 2, V, C).astype(np.float64)
            assert abs(z.mean()) < 0.2


# ------------------------------------------------------------------------------------------------- coefficient floor
@pytest.mark.parametrize("C,G", R.COEFF_CG)
def test_coefficient_floor_against_long_double(C, G):
    """the fp64 restatement against the same formulas in long double: the floor of the coefficient bars, printed per case
    group; it must leave the bar to the one fp32 rounding (8 floor <= 1e-3 of 2 u max|truth|)"""
    assert np.finfo(R.LD).nmant >= 63, "long double is no wider than double here: the floor would read 0"
    for count in R.COEFF_COUNTS:
        for affine in (True, False):
            N = 3
            c = R.coeff_case(C, G, N, count, affine)
            mrs, worst = [], {}
            for n in range(N):
                fl, out = R.coeff_floor(R.gn_fwd_coeffs, c["stats"][n], c["gamma"], c["beta"], G, count, R.EPS)
                mrs.append(out[2].astype(np.float32))
                for nm, f, o in zip(("scale", "shift", "mean_rstd"), fl, out):
                    worst[nm] = max(worst.get(nm, 0.0), f / np.abs(o).max())
                if count == 1 and G == C:
                    assert (out[2][:, 1] == 1 / np.sqrt(R.EPS)).all()                  # variance exactly 0
                assert np.isfinite(out[2]).all()
            mr = np.stack(mrs)
            fl, out = R.coeff_floor(R.gn_bwd_coeffs, c["ab"], c["gamma"], mr, G, count)
            for nm, f, o in zip(("c1", "c2", "c3"), [float(np.abs(out[0][..., i].astype(R.LD) - R.gn_bwd_coeffs(
                    c["ab"], c["gamma"], mr, G, count, dtype=R.LD)[0][..., i]).max()) for i in range(3)],
                    [out[0][..., i] for i in range(3)]):
                worst[nm] = f / max(np.abs(o).max(), 1e-300)
            worst["dgamma"], worst["dbeta"] = fl[1] / max(np.abs(out[1]).max(), 1e-300), fl[2] / np.abs(out[2]).max()
            if affine:
                ds, bh = R.fold_inputs(c["ab"], c["gamma"], c["beta"], mr, G)
                ff, fo = R.coeff_floor(R.gn_bwd_coeffs_fold, ds, bh, c["gamma"], c["beta"], mr, G, count)
                worst["fold c123"], worst["fold dgamma"] = ff[0] / np.abs(fo[0]).max(), ff[1] / max(np.abs(fo[1]).max(), 1e-300)
            print(f"C {C} G {G} count {count} affine {affine}: floor / max|truth| " +
                  "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
            assert all(8 * v <= 1e-3 * 2 * R.U for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------------- generators
@pytest.mark.parametrize("shape,C", [((6, 4, 10), 4), ((6, 4, 10), 12), ((2, 2, 2), 4), ((2, 2, 2), 12), ((6, 4, 10), 3),
                                     ((2, 2, 2), 3)])
def test_kink_free_volumes_are_away_from_the_kink(shape, C):
    for seed in (0, 1):
        for q in (False, True):
            z = R.kink_free(shape, C, seed, q)
            mean, rstd = R.instance_stats(z)
            assert (np.abs((z.astype(np.float64) - mean) * rstd) >= 1e-3).all(), (shape, C, seed, q)
            if q:
                w = R._windows(z)
                assert (z * 4 == np.round(z * 4)).all() and ((w == w.max(3, keepdims=True)).sum(3) >= 2).all()


def test_range_scale_property():
    assert R.range_scale_property(1.0, 2.0 ** 14) and not R.range_scale_property(1.0, 2.0 ** 15)
    assert R.range_scale_property(np.nextafter(np.float32(2), np.float32(0)), 2.0 ** 14)
    assert R.range_scale_property(0.0, 1.0) and R.range_scale_property(np.inf, 1.0) and R.range_scale_property(np.nan, 1.0)
    assert not R.range_scale_property(3.0, 3.0 * 2 ** 12)
