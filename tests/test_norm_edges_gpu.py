"""GPU: csrc/norm.hip (statistics, GroupNorm / InstanceNorm coefficients, the apply passes, MaxPool3d(2) in its variants, the lazy
InstanceNorm backward, upsample + concat, layout conversion, ReLU mask, range scale) against the fp64 restatement of
tests/norm_ref.py at the shapes where each kernel changes its path.  tests/test_norm_reference_cpu.py pins the restatement.

Every assertion is a bit equality or a bar derived in norm_ref's docstring (u = eps32 / 2): statistics 64 u sum|a| and 65 u
sum|ab|; coefficient kernels 2 u |truth| + 8 floor; apply passes 3 u (|c1 g| + |c2 x| + |c3|); chains the statistics bounds
propagated through the formulas (norm_ref.chain_bars).  Each test prints error and bar; the docstrings carry the worst ratio
error / bar observed on gfx950 (MI355X)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
POOL_SHAPES = [(2, 2, 2), (4, 6, 10), (7, 5, 9), (3, 2, 2)]


def _B():
    from keymorph_amd import backbone_ops as B
    return B


def _L():
    from keymorph_amd import _lib
    from keymorph_amd.ops import _p, _stream
    return _lib.load(), _lib.check, _p, _stream, _lib.KeymorphHipError


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {np.argwhere(bad)[0]}"


def _check(tag, got, truth, bar, quiet=False):
    """|got - truth| <= bar element by element (bar 0: exact); -> worst error / bar"""
    got, truth, bar = np.asarray(got, np.float64), np.asarray(truth, np.float64), np.broadcast_to(bar, np.shape(truth))
    err = np.abs(got - truth)
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))
    if not quiet:
        print(f"{tag}: error {float(err.max(initial=0.0)):.3e}, bar {float(bar.max(initial=0.0)):.3e}, worst error / bar {ratio:.3f}")
    assert np.isfinite(got).all() and ratio <= 1.0, f"{tag}: worst error / bar {ratio:.3f}"
    return ratio


def _expected_scale(m):
    """{S, 1/S} of range_scale for a bound m: m S in [2^14, 2^15), S = 1 for zero or a non-finite bound"""
    m = float(m)
    if not (0 < m < 3.0e38):
        return 1.0
    return 2.0 ** (15 - int(np.frexp(np.float32(m))[1]))


# ================================================================================================ statistics
def _stats_truth(a, b):
    return np.stack([np.stack(R.channel_sums(a[n], None if b is None else b[n]), -1) for n in range(a.shape[0])])


def _stats_bar(a, b):
    return np.stack([np.stack(R.stats_bars(a[n], None if b is None else b[n]), -1) for n in range(a.shape[0])])


@pytest.mark.parametrize("V,C", R.STAT_SHAPES, ids=[f"V{v}-C{c}" for v, c in R.STAT_SHAPES])
def test_channel_stats_vs_fp64(V, C):
    """kmh_channel_stats, both modes, every data class, N = 3 and N = 1 (whose bits must be the batch's): 64 u sum|a|, 65 u
    sum a^2, 65 u sum|ab|.  Observed worst error / bar over the table 0.056 (V = 333, C = 1024; at most 0.015 where a lane
    holds few terms) -- the float32 emulation of the kernel's order gives 0.064 (norm_ref's docstring)."""
    B = _B()
    worst = 0.0
    for cls in R.STAT_CLASSES:
        a = R.stat_data(cls, 3, V, C)
        b = R.stat_data("zero_mean", 3, V, C, seed=1) + np.float32(0.5)
        ad, bd = _dev(a), _dev(b)
        for bb, bbd in ((None, None), (b, bd)):
            got = B.channel_stats(ad, bbd, 3, V, C)
            one = B.channel_stats(ad[:1].contiguous(), None if bbd is None else bbd[:1].contiguous(), 1, V, C)
            assert torch.equal(one[0], got[0]), f"{cls}: N = 1 differs from sample 0 of N = 3"
            worst = max(worst, _check(f"{cls} mode {int(bb is not None)}", _np(got), _stats_truth(a, bb), _stats_bar(a, bb), True))
    print(f"V {V} C {C}: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("V,C", R.STAT_SHAPES, ids=[f"V{v}-C{c}" for v, c in R.STAT_SHAPES])
def test_in_bwd_stats_vs_fp64(V, C):
    """kmh_in_bwd_stats on the statistics table: (sum g, sum g z), g = du [fma(z, scale, shift) > 0] with scale / shift the
    reference's InstanceNorm coefficients rounded to fp32 (the sign of the fused multiply-add is the sign of the exact value,
    which fp64 holds).  Observed worst error / bar 0.016."""
    lib, check, _p, _stream, _ = _L()
    worst = 0.0
    for cls in R.STAT_CLASSES:
        z = R.stat_data(cls, 2, V, C)
        du = R.stat_data("zero_mean", 2, V, C, seed=1)
        co = [R.gn_fwd_coeffs(np.stack(R.channel_sums(z[n]), -1), None, None, C, V) for n in range(2)]
        scale, shift = (np.stack([c[i] for c in co]).astype(np.float32) for i in (0, 1))
        keep = (z.astype(np.float64) * scale[:, None, :] + shift[:, None, :].astype(np.float64)) > 0
        g = np.where(keep, du, np.float32(0))
        out = torch.empty((2, C, 2), dtype=torch.float64, device=DEV)
        ws = torch.empty(int(lib.kmh_channel_stats_ws_bytes(2, C)), dtype=torch.uint8, device=DEV)
        zd, dd, sc, sh = _dev(z), _dev(du), _dev(scale), _dev(shift)
        check(lib.kmh_in_bwd_stats(_p(dd), _p(zd), _p(sc), _p(sh), 2, V, C, _p(out), _p(ws), _stream()), "kmh_in_bwd_stats")
        worst = max(worst, _check(cls, _np(out), _stats_truth(g, z), _stats_bar(g, z), True))
    print(f"V {V} C {C}: worst error / bar {worst:.3f}")


def test_channel_stats_only_if_gate():
    """only_if holding 1 gives the bits of only_if = None; holding 0 both launches return at once and the output keeps its
    sentinel"""
    B = _B()
    lib, check, _p, _stream, _ = _L()
    for V, C in ((333, 12), (2049, 3)):
        a, b = _dev(R.stat_data("offset100", 2, V, C)), _dev(R.stat_data("zero_mean", 2, V, C, seed=1))
        one, zero = torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        for bb in (None, b):
            assert torch.equal(B.channel_stats(a, bb, 2, V, C, only_if=one), B.channel_stats(a, bb, 2, V, C))
            out = torch.full((2, C, 2), -7.25, dtype=torch.float64, device=DEV)
            ws = torch.empty(int(lib.kmh_channel_stats_ws_bytes(2, C)), dtype=torch.uint8, device=DEV)
            check(lib.kmh_channel_stats(_p(a), _p(bb), int(bb is not None), 2, V, C, _p(out), _p(ws), _p(zero), _stream()), "stats")
            assert bool((out == -7.25).all())


@pytest.mark.parametrize("C", R.STAT_REFUSED_C)
def test_stats_refuse_unserved_channel_counts(C):
    """C = 257 (scalar route, more channel groups than threads) and C = 1028 (past 4 x 256) answer -22, for both kernels"""
    B = _B()
    lib, _, _p, _stream, Err = _L()
    a = torch.zeros((1, 5, C), device=DEV)
    with pytest.raises(Err, match="-22"):
        B.channel_stats(a, None, 1, 5, C)
    with pytest.raises(Err, match="-22"):
        B.channel_stats(a, a, 1, 5, C)
    out, ws, s = torch.zeros((1, C, 2), dtype=torch.float64, device=DEV), torch.empty(1 << 24, dtype=torch.uint8, device=DEV), a[0, 0]
    assert lib.kmh_in_bwd_stats(_p(a), _p(a), _p(s), _p(s), 1, 5, C, _p(out), _p(ws), _stream()) == -22


# ============================================================================================== coefficients
def _coeff_variants():
    return [(N, count, affine) for N in (1, 3) for count in R.COEFF_COUNTS for affine in (True, False)]


def _mr32(c, G, count, N):
    return np.stack([R.gn_fwd_coeffs(c["stats"][n], c["gamma"], c["beta"], G, count)[2] for n in range(N)]).astype(np.float32)


@pytest.mark.parametrize("C,G", R.COEFF_CG)
def test_fwd_coeffs_vs_fp64(C, G):
    """kmh_gn_fwd_coeffs fed the reference's fp64 statistics: scale, shift, mean_rstd within 2 u |truth| + 8 floor; count 1 with
    G = C is a group of variance exactly 0 (rstd = 1 / sqrt(eps)).  Observed worst error / bar 0.50: one rounding."""
    B = _B()
    worst = 0.0
    for N, count, affine in _coeff_variants():
        c = R.coeff_case(C, G, N, count, affine)
        got = B.norm_coeffs(_dev(c["stats"]), _dev(c["gamma"]), _dev(c["beta"]), N, C, G, count)
        for n in range(N):
            floors, truth = R.coeff_floor(R.gn_fwd_coeffs, c["stats"][n], c["gamma"], c["beta"], G, count, R.EPS)
            for nm, g, t, f in zip(("scale", "shift", "mean_rstd"), got, truth, floors):
                worst = max(worst, _check(f"N {N} count {count} affine {affine} {nm}[{n}]", _np(g)[n], t, R.coeff_bar(t, f), True))
    print(f"C {C} G {G}: worst error / bar {worst:.3f}")


def test_fwd_coeffs_group_of_variance_zero():
    """a constant group among ordinary ones: its rstd is 1 / sqrt(eps) within the bar 2 u |truth| + 8 floor, never inf or NaN.
    Observed worst error / bar 0.45."""
    B = _B()
    C, G, V = 12, 4, 333
    x = R.stat_data("zero_mean", 2, V, C)
    x[..., 3:6] = R.CONST_VALUE
    stats = _stats_truth(x, None)
    scale, shift, mr = B.norm_coeffs(_dev(stats), None, None, 2, C, G, V)
    for n in range(2):
        floors, truth = R.coeff_floor(R.gn_fwd_coeffs, stats[n], None, None, G, V, R.EPS)
        assert truth[2][1, 1] == 1 / np.sqrt(R.EPS) and truth[2][1, 0] == R.CONST_VALUE
        for nm, g, t, f in zip(("scale", "shift", "mean_rstd"), (scale, shift, mr), truth, floors):
            _check(f"{nm}[{n}]", _np(g)[n], t, R.coeff_bar(t, f))


@pytest.mark.parametrize("C,G", R.COEFF_CG)
def test_fwd_coeffs_range_scale_output(C, G):
    """the ascale output: S a power of two with (max|gamma| sqrt(count cpg) + max|beta|) S in [2^14, 2^15) (the bound is formed
    in fp32: 4 u of slack at the interval's ends) and S (1 / S) == 1"""
    lib, check, _p, _stream, _ = _L()
    for N, count, affine in _coeff_variants():
        c = R.coeff_case(C, G, N, count, affine)
        st, ga, be = _dev(c["stats"]), _dev(c["gamma"]), _dev(c["beta"])
        o = [torch.empty(s, device=DEV) for s in ((N, C), (N, C), (N, G, 2))]
        asc = torch.full((2,), -1.0, device=DEV)
        check(lib.kmh_gn_fwd_coeffs(_p(st), _p(ga), _p(be), N, C, G, float(count), R.EPS, _p(o[0]), _p(o[1]), _p(o[2]), _p(asc),
                                    _stream()), "kmh_gn_fwd_coeffs")
        S, inv = (float(v) for v in asc.cpu())
        bound = R.ascale_bound(c["gamma"], c["beta"], count, C // G)
        assert R.range_scale_property(bound, S, 4 * U) and S * inv == 1.0, (N, count, affine, bound, S, inv)


@pytest.mark.parametrize("C,G", R.COEFF_CG)
def test_bwd_coeffs_vs_fp64(C, G):
    """kmh_gn_bwd_coeffs (c123, dgamma, dbeta) fed the reference's fp64 sums and its fp32 mean / rstd, and the fold route
    (kmh_gn_bwd_coeffs_fold) on the same data: 2 u |truth| + 8 floor.  G > 64, N G > 256 and C > 256 take the loops' second
    trips.  Observed worst error / bar 0.50 (direct and fold): one rounding."""
    B = _B()
    worst = 0.0
    for N, count, affine in _coeff_variants():
        c = R.coeff_case(C, G, N, count, affine)
        mr = _mr32(c, G, count, N)
        floors, truth = R.coeff_floor(R.gn_bwd_coeffs, c["ab"], c["gamma"], mr, G, count)
        got = B._gn_bwd_coeffs(_dev(c["ab"]), _dev(c["gamma"]), _dev(mr), N, C, G, count)
        tag = f"N {N} count {count} affine {affine}"
        for nm, g, t, f in zip(("c123", "dgamma", "dbeta"), got, truth, floors):
            if g is None:
                assert not affine and nm != "c123"
                continue
            worst = max(worst, _check(f"{tag} {nm}", _np(g), t, R.coeff_bar(t, f), True))
        ds, bh = R.fold_inputs(c["ab"], c["gamma"], c["beta"], mr, G)
        ffl, ftruth = R.coeff_floor(R.gn_bwd_coeffs_fold, ds, bh, c["gamma"], c["beta"], mr, G, count)
        poison = torch.full((N, C, 2), float("nan"), dtype=torch.float64, device=DEV)     # the gated direct route must not run
        fgot = B._gn_bwd_coeffs(poison, _dev(c["gamma"]), _dev(mr), N, C, G, count, fold=(_dev(ds), _dev(bh), _dev(c["beta"])))
        for nm, g, t, f in zip(("c123", "dgamma", "dbeta"), fgot, ftruth, ffl):
            if g is not None:
                worst = max(worst, _check(f"{tag} fold {nm}", _np(g), t, R.coeff_bar(t, f), True))
    print(f"C {C} G {G}: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("C,G,N", [(12, 4, 1), (320, 320, 3)])
def test_fold_with_a_zero_gamma_flags_and_writes_nothing(C, G, N):
    """one gamma exactly 0: the flag reads 1 and c123, dgamma, dbeta stay as pre-filled; through the wrapper the un-gated
    direct route then gives the direct answer within 2 u |truth| + 8 floor.  Observed worst error / bar 0.49."""
    B = _B()
    lib, check, _p, _stream, _ = _L()
    count = 333
    c = R.coeff_case(C, G, N, count, True)
    c["gamma"][C - 2] = 0.0
    mr = _mr32(c, G, count, N)
    ds, bh = R.fold_inputs(c["ab"], c["gamma"], c["beta"], mr, G)
    dsd, bhd, ga, be, mrd = _dev(ds), _dev(bh), _dev(c["gamma"]), _dev(c["beta"]), _dev(mr)
    c123, dg, db = (torch.full(s, 3.5, device=DEV) for s in ((N, C, 3), (C,), (C,)))
    flag = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    check(lib.kmh_gn_bwd_coeffs_fold(_p(dsd), _p(bhd), _p(ga), _p(be), _p(mrd), N, C, G, float(count), _p(c123), _p(dg), _p(db),
                                     _p(flag), _stream()), "fold")
    assert int(flag) == 1 and all(bool((t == 3.5).all()) for t in (c123, dg, db))
    floors, truth = R.coeff_floor(R.gn_bwd_coeffs, c["ab"], c["gamma"], mr, G, count)
    got = B._gn_bwd_coeffs(_dev(c["ab"]), ga, mrd, N, C, G, count, fold=(dsd, bhd, be))
    for nm, g, t, f in zip(("c123", "dgamma", "dbeta"), got, truth, floors):
        _check(f"fallback {nm}", _np(g), t, R.coeff_bar(t, f))


# ==================================================================================================== apply
def _apply_inputs(N, V, C, seed=0):
    r = np.random.default_rng([N, V, C, seed, 5])
    x = r.standard_normal((N, V, C)).astype(np.float32)
    x.reshape(-1)[::7] = 0.0                                       # the mask is x > 0: exact zeros of both signs are masked
    x.reshape(-1)[3::11] = -0.0
    return r.standard_normal((N, V, C)).astype(np.float32), x, r.standard_normal((N, C, 3)).astype(np.float32)


@pytest.mark.parametrize("C", [3, 4, 8, 20])
@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("in_place", [True, False])
def test_gn_bwd_apply_vs_fp64(C, mask, in_place):
    """dx = [x > 0] (c1 dxn + c2 x + c3) with reference coefficients: 3 u (|c1 g| + |c2 x| + |c3|), masked elements (x = 0 and
    -0.0 among them) exactly 0, and the published range scale that of max|dx| as written.  Observed worst error / bar 0.59."""
    B = _B()
    N, V = 2, 77
    dxn, x, c123 = _apply_inputs(N, V, C)
    d, xd, cd = _dev(dxn), _dev(x), _dev(c123)
    sc2 = torch.zeros(2, device=DEV)
    out = None if in_place else torch.full((N, V, C), 9.0, device=DEV)
    got = B._gn_bwd_apply(d, xd, cd, N, V, C, sc2, from_relu=mask, out=out)
    assert got.data_ptr() == (d if in_place else out).data_ptr()
    g = _np(got)
    for n in range(N):
        truth, bar = R.gn_bwd_apply(dxn[n], x[n], c123[n], mask)
        _check(f"dx[{n}]", g[n], truth, bar)
        if mask:
            assert (_bits(g[n][~(x[n] > 0)]) == 0).all()
    S, inv = (float(v) for v in sc2.cpu())
    assert S == _expected_scale(np.abs(g).max()) and S * inv == 1.0 and R.range_scale_property(np.abs(g).max(), S)


@pytest.mark.parametrize("C", [8, 24])
def test_gn_bwd_apply_blocked_is_the_dense_result_relaid(C):
    B = _B()
    N, V = 2, 77
    dxn, x, c123 = _apply_inputs(N, V, C, 1)
    d, xd, cd = _dev(dxn), _dev(x), _dev(c123)
    s1, s2 = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV)
    dense = B._gn_bwd_apply(d, xd, cd, N, V, C, s1, out=torch.empty((N, V, C), device=DEV))
    blocked = B._gn_bwd_apply(d, xd, cd, N, V, C, s2, out=torch.full((N, V, C), 9.0, device=DEV), blocked=True)
    want = _np(dense).reshape(N, V, C // 8, 8).transpose(0, 2, 1, 3)
    _same_bits("blocked", _np(blocked).reshape(N, C // 8, V, 8), np.ascontiguousarray(want))
    assert torch.equal(s1, s2)


def test_gn_bwd_apply_refuses_blocked_in_place_and_ragged_chunks():
    B = _B()
    _, _, _, _, Err = _L()
    for C, in_place in ((12, False), (8, True)):
        dxn, x, c123 = (_dev(t) for t in _apply_inputs(1, 5, C))
        with pytest.raises(Err, match="-22"):
            B._gn_bwd_apply(dxn, x, c123, 1, 5, C, None, out=None if in_place else torch.empty_like(dxn), blocked=True)


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("relu", [0, 1])
def test_norm_apply_vs_fp64(C, relu):
    """y = act(x scale + shift): 3 u (|x scale| + |shift|).  Observed worst error / bar 0.33."""
    lib, check, _p, _stream, _ = _L()
    N, V = 2, 77
    r = np.random.default_rng([C, relu])
    x, sc, sh = (r.standard_normal(s).astype(np.float32) for s in ((N, V, C), (N, C), (N, C)))
    xd, scd, shd, y = _dev(x), _dev(sc), _dev(sh), torch.full((N, V, C), 9.0, device=DEV)
    check(lib.kmh_norm_apply(_p(xd), _p(scd), _p(shd), N, V, C, relu, _p(y), _stream()), "kmh_norm_apply")
    for n in range(N):
        truth, bar = R.norm_apply(x[n], sc[n], sh[n], relu)
        _check(f"y[{n}]", _np(y)[n], truth, bar)
    assert not relu or bool((y >= 0).all())


def test_relu_mask_at_zero_denormal_and_nan():
    """dz = dy where y > 0: y = 0, -0.0 and NaN give +0, a positive denormal passes the gradient; bit for bit"""
    lib, check, _p, _stream, _ = _L()
    special = np.array([0.0, -0.0, 1e-40, -1e-40, np.nan, 1.0, -1.0, np.float32(1.4e-45)], np.float32)
    y = np.tile(special, 131)[:1031]
    dy = np.random.default_rng(0).standard_normal(y.shape).astype(np.float32)
    dyd, yd, dz = _dev(dy), _dev(y), torch.full((y.size,), 9.0, device=DEV)
    check(lib.kmh_relu_mask(_p(dyd), _p(yd), y.size, _p(dz), _stream()), "kmh_relu_mask")
    _same_bits("dz", _np(dz), R.relu_mask(dy, y))


# ==================================================================================================== chains
def _gn_chain(x, dy, gamma, beta, G):
    """statistics -> coefficients -> apply and back on the GPU, no convolution in between"""
    B = _B()
    lib, check, _p, _stream, _ = _L()
    N, V, C = x.shape
    xd, dd, ga, be = _dev(x), _dev(dy), _dev(gamma), _dev(beta)
    scale, shift, mr = B.norm_coeffs(B.channel_stats(xd, None, N, V, C), ga, be, N, C, G, V)
    y = torch.empty_like(xd)
    check(lib.kmh_norm_apply(_p(xd), _p(scale), _p(shift), N, V, C, 0, _p(y), _stream()), "kmh_norm_apply")
    c123, dgamma, dbeta = B._gn_bwd_coeffs(B.channel_stats(dd, xd, N, V, C), ga, mr, N, C, G, V)
    dx = B._gn_bwd_apply(dd, xd, c123, N, V, C, None, from_relu=False, out=torch.empty_like(xd))
    return {"rstd": _np(mr)[..., 1], "y": _np(y), "dx": _np(dx), "dgamma": _np(dgamma), "dbeta": _np(dbeta)}


def _gn_truth(x, dy, gamma, beta, G, dtype=torch.float64):
    xt = torch.from_numpy(x).to(dtype).permute(0, 2, 1).requires_grad_(True)
    gt, bt = (torch.from_numpy(t).to(dtype).requires_grad_(True) for t in (gamma, beta))
    y = F.group_norm(xt, G, gt, bt, R.EPS)
    y.backward(torch.from_numpy(dy).to(dtype).permute(0, 2, 1))
    N, C, V = xt.shape
    rstd = torch.native_group_norm(xt.detach().contiguous(), gt.detach(), bt.detach(), N, C, V, G, R.EPS)[2].double().reshape(N, G)
    return {"rstd": rstd.numpy(), "y": y.detach().permute(0, 2, 1).double().numpy(), "dx": xt.grad.permute(0, 2, 1).double().numpy(),
            "dgamma": gt.grad.double().numpy(), "dbeta": bt.grad.double().numpy()}


def _chain_case(ratio, V):
    C, G, N = 8, 2, 2
    r = np.random.default_rng([int(ratio), V, 9])
    x = (ratio + r.standard_normal((N, V, C))).astype(np.float32)
    dy = r.standard_normal((N, V, C)).astype(np.float32)
    gamma, beta = (1 + 0.5 * r.standard_normal(C)).astype(np.float32), (0.3 * r.standard_normal(C)).astype(np.float32)
    return x, dy, gamma, beta, G


def _chain_check(got, truth, x, dy, gamma, beta, G):
    N = x.shape[0]
    ch = [R.chain_bars(x[n], dy[n], gamma, beta, G) for n in range(N)]
    worst = {}
    for k in ("rstd", "y", "dx"):
        for n in range(N):
            bar = ch[n][k].e + np.abs(ch[n][k].v - truth[k][n])          # + the fp64 cancellation of the kernels' own formula
            worst[k] = max(worst.get(k, 0.0), _check(f"{k}[{n}]", got[k][n], truth[k][n], bar, True))
    for k in ("dgamma", "dbeta"):
        v = sum(c[k].v for c in ch)
        bar = sum(c[k].e for c in ch) + U * np.abs(v) + np.abs(v - truth[k])
        worst[k] = _check(k, got[k], truth[k], bar, True)
    return worst, ch


@pytest.mark.parametrize("ratio", [0, 3, 30])
@pytest.mark.parametrize("V", [64, 3000])
def test_group_norm_chain_vs_fp64_autograd(ratio, V):
    """statistics -> coefficients -> apply forward, statistics (mode 1) -> backward coefficients -> apply, against fp64
    F.group_norm autograd at mean / std 0, 3, 30 with the propagated bar (norm_ref.chain_bars).  Observed worst error / bar:
    rstd 0.016, y 0.030, dx 0.050, dgamma 0.002, dbeta 0.002, all at mean / std 0; below 0.002 at 3 and 30 -- the bound is a
    worst case over 64-term sums and treats |x| d_scale and d_shift as independent, so it is loose by ~ mean / std there (the
    tight checks of each kernel are the tests above)."""
    x, dy, gamma, beta, G = _chain_case(ratio, V)
    got, truth = _gn_chain(x, dy, gamma, beta, G), _gn_truth(x, dy, gamma, beta, G)
    worst, ch = _chain_check(got, truth, x, dy, gamma, beta, G)
    assert max(float((c["rstd"].e / c["rstd"].v).max()) for c in ch) <= 1e-2        # inside the design's operating range
    print(f"mean/std {ratio} V {V}: worst error / bar " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("ratio", [100, 1000])
def test_group_norm_chain_past_its_operating_range(ratio):
    """mean / std 100 and 1000, V = 3000: the propagated bar on rstd is past 1e-2 (var = ss / m - mean^2 cancels (mean / std)^2
    of the fp32 sums' 64 u), so only finiteness and the derived bar are asserted; the observed relative errors are printed
    next to those of fp32 F.group_norm on the CPU (two-pass variance) -- recorded, not asserted.
    Observed on gfx950, max relative to max|truth|:
        mean / std 100    rstd 1.6e-5   y 1.5e-5   dx 1.4e-5     fp32 torch (CPU): rstd 1.4e-7   y 1.8e-6   dx 4.8e-7
        mean / std 1000   rstd 4.6e-3   y 3.9e-3   dx 4.0e-3     fp32 torch (CPU): rstd 8.6e-7   y 3.3e-5   dx 6.7e-6"""
    x, dy, gamma, beta, G = _chain_case(ratio, 3000)
    got, truth = _gn_chain(x, dy, gamma, beta, G), _gn_truth(x, dy, gamma, beta, G)
    worst, ch = _chain_check(got, truth, x, dy, gamma, beta, G)
    assert min(float((c["rstd"].e / c["rstd"].v).max()) for c in ch) > 1e-2
    t32 = _gn_truth(x, dy, gamma, beta, G, torch.float32)
    rel = lambda a, k: float(np.abs(a[k] - truth[k]).max() / np.abs(truth[k]).max())                          # noqa: E731
    print(f"mean/std {ratio}: kernels " + "  ".join(f"{k} {rel(got, k):.1e}" for k in ("rstd", "y", "dx")) + "   fp32 torch (CPU) " +
          "  ".join(f"{k} {rel(t32, k):.1e}" for k in ("rstd", "y", "dx")) + "   error / bar " +
          "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ================================================================================= lazy InstanceNorm backward
def _in_bwd_gpu(z, du, pool, in_place):
    B = _B()
    lib, check, _p, _stream, _ = _L()
    N, D, H, W, C = z.shape
    V = D * H * W
    zd, g = _dev(z), _dev(du)
    scale, shift, mr = B.norm_coeffs(B.channel_stats(zd, None, N, V, C), None, None, N, C, C, V)
    if not pool:
        return B._in_bwd(g, zd, zd, scale, shift, mr, in_place=in_place), g
    u = torch.empty((N, D // 2, H // 2, W // 2, C), device=DEV)
    arg = torch.empty(u.shape, dtype=torch.uint8, device=DEV)
    check(lib.kmh_maxpool3d_fwd(_p(zd), _p(u), _p(arg), N, D, H, W, C, _stream()), "kmh_maxpool3d_fwd")
    return B._in_bwd(g, u, zd, scale, shift, mr, arg=arg, in_place=in_place), g


def _in_truth(z, du, pool):
    zt = torch.from_numpy(z).double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    u = F.relu(F.instance_norm(zt, eps=R.EPS))
    u = F.max_pool3d(u, 2) if pool else u
    u.backward(torch.from_numpy(du).double().permute(0, 4, 1, 2, 3))
    return zt.grad.permute(0, 2, 3, 4, 1).numpy()


IN_SHAPES = ((6, 4, 10), (2, 2, 2))
IN_CASES = [(True, s, C) for s in IN_SHAPES for C in (4, 12)] + [(False, s, C) for s in IN_SHAPES for C in (3, 4)]


@pytest.mark.parametrize("pool,shape,C", IN_CASES)
@pytest.mark.parametrize("quantised", [False, True])
def test_in_bwd_vs_fp64_autograd(pool, shape, C, quantised):
    """_in_bwd against fp64 autograd of ReLU(IN(z)) and MaxPool(ReLU(IN(z))), N = 2, on volumes with |zhat| >= 1e-3 everywhere
    (every element compared) and on quantised ones with the window maximum tied (the winner rule is part of the answer); the
    bar is the chain's (norm_ref.chain_bars with G = C, g = scatter(du) [zhat > 0]).  Unpooled: in place and not, same bits.
    Observed worst error / bar 0.021."""
    N = 2
    z = np.stack([R.kink_free(shape, C, n, quantised) for n in range(N)])
    ush = tuple(s // 2 for s in shape) if pool else shape
    du = np.random.default_rng([C, 3] + list(shape)).standard_normal((N,) + ush + (C,)).astype(np.float32)
    truth = _in_truth(z, du, pool)
    got, g_in = _in_bwd_gpu(z, du, pool, False)
    assert got.data_ptr() != g_in.data_ptr()
    if not pool:
        again, g_in = _in_bwd_gpu(z, du, pool, True)
        assert again.data_ptr() == g_in.data_ptr() and torch.equal(again, got)
    worst = 0.0
    for n in range(N):
        mean, rstd = R.instance_stats(z[n])
        keep = ((z[n].astype(np.float64) - mean) * rstd > 0).reshape(-1, C)
        g = R.maxpool2_scatter(du[n], R.maxpool2(z[n])[1], shape) if pool else du[n]
        ch = R.chain_bars(z[n].reshape(-1, C), g.reshape(-1, C), None, None, C, mask=keep)["dx"]
        t = truth[n].reshape(-1, C)
        worst = max(worst, _check(f"dz[{n}]", _np(got)[n].reshape(-1, C), t, ch.e + np.abs(ch.v - t)))
    print(f"worst error / bar {worst:.3f}")


def test_in_bwd_pooled_route_refuses_what_it_cannot_serve():
    """C = 6 and an odd dimension answer -22; in place through the pooling (dz is 8 times the size of du) is refused by the
    wrapper before anything is launched"""
    _, _, _, _, Err = _L()
    for shape, C in (((4, 4, 4), 6), ((3, 2, 2), 4)):
        z = np.stack([R.kink_free(shape, C, n) for n in range(2)])
        du = np.ones((2,) + tuple(s // 2 for s in shape) + (C,), np.float32)
        with pytest.raises(Err, match="-22"):
            _in_bwd_gpu(z, du, True, False)
    z = np.stack([R.kink_free((2, 2, 2), 4, n) for n in range(2)])
    with pytest.raises(ValueError, match="in place"):
        _in_bwd_gpu(z, np.ones((2, 1, 1, 1, 4), np.float32), True, True)


# ================================================================================================== pooling
class _Ctx:
    def __init__(self, arg, xshape):
        self.saved_tensors, self.xshape = (arg,), xshape


def _pool_fwd(x):
    lib, check, _p, _stream, _ = _L()
    N, D, H, W, C = x.shape
    xd = _dev(x)
    y = torch.full((N, D // 2, H // 2, W // 2, C), 9.0, device=DEV)
    arg = torch.full(y.shape, 99, dtype=torch.uint8, device=DEV)
    check(lib.kmh_maxpool3d_fwd(_p(xd), _p(y), _p(arg), N, D, H, W, C, _stream()), "kmh_maxpool3d_fwd")
    return xd, y, arg


@pytest.mark.parametrize("cls", R.POOL_CLASSES)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_forward_winners_backward_bit_for_bit(cls, shape):
    """MaxPool3d(2): value, winner and scatter equal the restatement (pinned to fp64 F.max_pool3d on the CPU) in every bit, at
    ties, zeros, -inf and NaN by position, C in {1, 3, 4, 8, 16} (scalar and 16-byte kernels), through the wrapper as well;
    odd shapes: the trailing planes of the gradient are exactly 0"""
    B = _B()
    N = 2
    for C in (1, 3, 4, 8, 16):
        x = np.stack([R.pool_data(cls, shape, C, n) for n in range(N)])
        ref = [R.maxpool2(x[n]) for n in range(N)]
        xd, y, arg = _pool_fwd(x)
        _same_bits(f"C {C} y", _np(y), np.stack([r[0] for r in ref]))
        _same_bits(f"C {C} winners", _np(arg), np.stack([r[1] for r in ref]))
        xr = xd.clone().requires_grad_(True)
        yw = B.maxpool2(xr)
        _same_bits(f"C {C} wrapper y", _np(yw), np.stack([r[0] for r in ref]))
        dy = np.random.default_rng([C, 1]).standard_normal(yw.shape).astype(np.float32)
        yw.backward(_dev(dy))
        want = np.stack([R.maxpool2_scatter(dy[n], ref[n][1], shape) for n in range(N)])
        _same_bits(f"C {C} dx", _np(xr.grad), want)
        lib, check, _p, _stream, _ = _L()                  # the rescan route (no winners recorded) finds the same ones
        dx2, dyd = torch.zeros_like(xd), _dev(dy)
        check(lib.kmh_maxpool3d_bwd(_p(xd), None, _p(dyd), None, 0, _p(dx2), N, *shape, C, 0, _stream()), "kmh_maxpool3d_bwd")
        _same_bits(f"C {C} dx by rescan", _np(dx2), want)


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C,pad", [(3, 2), (4, 4), (4, 3), (8, 8), (16, 4)])
def test_maxpool_backward_with_a_second_gradient(shape, C, pad):
    """dx = scatter(dy) + add with `add` a channel-strided view of a wider tensor (stride a multiple of 4 floats or not) and a
    dense one: one fp32 addition per element, bit for bit; at odd shapes the trailing planes equal `add`"""
    B = _B()
    N = 2
    D, H, W = shape
    x = np.stack([R.pool_data("relu", shape, C, n) for n in range(N)])
    _, y, arg = _pool_fwd(x)
    r = np.random.default_rng([C, pad, 2])
    dy = r.standard_normal(tuple(y.shape)).astype(np.float32)
    wide = r.standard_normal((N, D, H, W, C + pad)).astype(np.float32)
    want = np.stack([R.maxpool2_scatter(dy[n], _np(arg)[n], shape, wide[n][..., :C]) for n in range(N)])
    for add in (_dev(wide)[..., :C], _dev(wide)[..., :C].contiguous()):
        dx = B._maxpool_bwd(_Ctx(arg, (N, D, H, W, C)), _dev(dy), add)
        _same_bits(f"dx (add stride {add.stride(3)})", _np(dx), want)


@pytest.mark.parametrize("shape", [(2, 2, 2), (4, 6, 10)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", [8, 16])
def test_maxpool_backward_blocked_split_and_lazy(shape, C):
    """the channel-blocked scatter (with and without a second gradient) is the dense one re-laid; kmh_maxpool3d_bwd_split's
    records are the fp16 hi / lo split of the dense result times S (hi = fp16(v S), lo = fp16(v S - hi)) with the last
    record of every plane zero; kmh_maxpool3d_bwd_lazy is scatter + the GroupNorm-backward apply (bar: the apply's 3 u (...)
    plus one rounding of the sum) with the range scale of what it wrote.  Observed worst error / bar (lazy) 0.58."""
    B = _B()
    lib, check, _p, _stream, _ = _L()
    N = 2
    D, H, W = shape
    V = D * H * W
    x = np.stack([R.pool_data("relu", shape, C, n) for n in range(N)])
    _, y, arg = _pool_fwd(x)
    r = np.random.default_rng([C, 7] + list(shape))
    dy = r.standard_normal(tuple(y.shape)).astype(np.float32)
    dyd = _dev(dy)
    dense = np.stack([R.maxpool2_scatter(dy[n], _np(arg)[n], shape) for n in range(N)])
    ctx = _Ctx(arg, (N, D, H, W, C))
    blk = B._maxpool_bwd(ctx, dyd, None, out_blocked=True)
    _same_bits("blocked", _np(blk).reshape(N, C // 8, D, H, W, 8), np.stack([R.to_blocked(d) for d in dense]))
    add = r.standard_normal((N, D, H, W, C)).astype(np.float32)
    blk = B._maxpool_bwd(ctx, dyd, _dev(add), out_blocked=True)
    _same_bits("blocked + add", _np(blk).reshape(N, C // 8, D, H, W, 8), np.stack([R.to_blocked(d + a) for d, a in zip(dense, add)]))
    # pre-split records
    sc = B.absmax_scale(dyd)
    S = float(sc[0])
    assert lib.kmh_maxpool3d_bwd_split_bytes(N, D, H, W, C) == N * (C // 8) * (V + 1) * 32
    rec = torch.full((N, C // 8, V + 1, 16), -1, dtype=torch.int16, device=DEV)
    check(lib.kmh_maxpool3d_bwd_split(_p(arg), _p(dyd), _p(sc), _p(rec), N, D, H, W, C, _stream()), "kmh_maxpool3d_bwd_split")
    v = (dense * np.float32(S)).reshape(N, V, C // 8, 8).transpose(0, 2, 1, 3)                       # a power of two: exact
    hi = v.astype(np.float16)
    lo = (v.astype(np.float64) - hi.astype(np.float64)).astype(np.float32).astype(np.float16)
    got = _np(rec).view(np.float16)
    assert np.array_equal(got[:, :, :V, :8], hi) and np.array_equal(got[:, :, :V, 8:], lo)
    assert (_bits(got[:, :, V]) == 0).all()
    # scatter + pending GroupNorm backward of the skip gradient
    dxn, xs, c123 = _apply_inputs(N, V, C, 3)
    dx, sc2 = torch.full((N, D, H, W, C), 9.0, device=DEV), torch.full((2,), -1.0, device=DEV)
    dxnd, xsd, c123d = _dev(dxn), _dev(xs), _dev(c123)
    check(lib.kmh_maxpool3d_bwd_lazy(_p(arg), _p(dyd), _p(dxnd), _p(xsd), _p(c123d), _p(dx), N, D, H, W, C, _p(sc2),
                                     _stream()), "kmh_maxpool3d_bwd_lazy")
    g = _np(dx).reshape(N, V, C)
    for n in range(N):
        t, bar = R.gn_bwd_apply(dxn[n], xs[n], c123[n], True)
        sct = dense[n].reshape(V, C).astype(np.float64)
        _check(f"lazy dx[{n}]", g[n], sct + t, bar + U * (np.abs(sct) + np.abs(t) + bar))
    assert float(sc2[0]) == _expected_scale(np.abs(g).max()) and float(sc2[0]) * float(sc2[1]) == 1.0


# ==================================================================================================== upcat
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("Cs,Cl", [(5, 7), (8, 12)])
def test_upcat_sweeps_every_ragged_size(axis, Cs, Cl):
    """upcat forward and both gradients with one axis swept over every (n_in, n_out), 1 <= n_in <= 17, n_in <= n_out <= 2 n_in
    + 1, the other two of size 1 and 2: forward and dskip bit for bit, dlow (up to 3 fp32 terms here, 27 in general) within
    27 u sum|terms|.  Observed worst error / bar 0.068."""
    B = _B()
    N, worst = 2, 0.0
    r = np.random.default_rng([axis, Cs, Cl])
    for n_in, n_out in R.nearest_pairs():
        lsh, osh = [1, 2], [1, 2]
        lsh.insert(axis, n_in)
        osh.insert(axis, n_out)
        skip = r.standard_normal([N] + osh + [Cs]).astype(np.float32)
        low = r.standard_normal([N] + lsh + [Cl]).astype(np.float32)
        g = r.standard_normal([N] + osh + [Cs + Cl]).astype(np.float32)
        sd, ld = _dev(skip).requires_grad_(True), _dev(low).requires_grad_(True)
        out = B.upcat(sd, ld)
        out.backward(_dev(g))
        for n in range(N):
            _same_bits(f"{n_in}->{n_out} out", _np(out)[n], R.upcat(skip[n], low[n]))
            dskip, dlow, mag = R.upcat_bwd(g[n], Cs, tuple(lsh))
            _same_bits(f"{n_in}->{n_out} dskip", _np(sd.grad)[n], dskip)
            worst = max(worst, _check(f"{n_in}->{n_out} dlow", _np(ld.grad)[n], dlow, 27 * U * mag, True))
    print(f"axis {axis}: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("Cs,Cl", [(5, 7), (8, 12)])
def test_upcat_exact_doubling(Cs, Cl):
    """every axis doubled (the 16-byte gradient kernel at Cs, Cl % 4 == 0): 8 terms per coarse voxel.  Observed worst error /
    bar 0.047."""
    B = _B()
    r = np.random.default_rng([Cs, Cl, 8])
    skip, low, g = (r.standard_normal(s).astype(np.float32) for s in ((2, 4, 6, 2, Cs), (2, 2, 3, 1, Cl), (2, 4, 6, 2, Cs + Cl)))
    sd, ld = _dev(skip).requires_grad_(True), _dev(low).requires_grad_(True)
    out = B.upcat(sd, ld)
    out.backward(_dev(g))
    for n in range(2):
        _same_bits("out", _np(out)[n], R.upcat(skip[n], low[n]))
        dskip, dlow, mag = R.upcat_bwd(g[n], Cs, (2, 3, 1))
        _same_bits("dskip", _np(sd.grad)[n], dskip)
        _check("dlow", _np(ld.grad)[n], dlow, 27 * U * mag)


# =================================================================================================== layout
@pytest.mark.parametrize("C", [2, 31, 32, 33, 65])
def test_layout_conversion_both_ways(C):
    """NCDHW <-> NDHWC at sizes round the 32 x 32 tile, both directions and the round trip, bit for bit"""
    B = _B()
    for V, dims in ((1, (1, 1, 1)), (31, (1, 1, 31)), (32, (2, 4, 4)), (33, (1, 3, 11)), (1000, (10, 10, 10))):
        x = np.random.default_rng([C, V]).standard_normal((2, C) + dims).astype(np.float32)
        xd = _dev(x)
        a = B.to_ndhwc(xd)
        _same_bits(f"V {V} to_ndhwc", _np(a), np.ascontiguousarray(x.transpose(0, 2, 3, 4, 1)))
        assert a.is_contiguous()
        b = B.to_ncdhw(a)
        _same_bits(f"V {V} round trip", _np(b), x)
        assert b.is_contiguous()


# ============================================================================================== range scale
def test_absmax_scale_at_powers_of_two_and_non_finite_values():
    """kmh_absmax_scale returns S with max|x| S in [2^14, 2^15): an exact power of two lands ON 2^14.  A NaN among finite values
    is ignored (fmaxf), an inf or an all-NaN tensor gives S = 1 -- pinned as the code has it."""
    B = _B()
    base = np.random.default_rng(4).uniform(-0.9, 0.9, 1003).astype(np.float32)
    for bound in (1.0, 2.0 ** 14, 2.0 ** -20):
        x = base * np.float32(bound)
        x[501] = -bound
        s = _np(B.absmax_scale(_dev(x)))
        assert float(s[0]) * bound == 2.0 ** 14 and float(s[0]) * float(s[1]) == 1.0, (bound, s)
        assert R.range_scale_property(bound, s[0])
        s = _np(B.absmax_scale(_dev(x * np.float32(0.25)), min_abs=bound))            # the floor takes over
        assert float(s[0]) * bound == 2.0 ** 14
    below = np.nextafter(np.float32(2.0), np.float32(0))
    assert float(B.absmax_scale(_dev(np.array([below, 0.5], np.float32)))[0]) * float(below) < 2.0 ** 15
    x = base.copy()
    x[7], x[500] = np.nan, 3.0
    assert float(B.absmax_scale(_dev(x))[0]) == _expected_scale(3.0) == 2.0 ** 13
    x[9] = np.inf
    assert _np(B.absmax_scale(_dev(x))).tolist() == [1.0, 1.0]
    assert _np(B.absmax_scale(_dev(np.full(77, np.nan, np.float32)))).tolist() == [1.0, 1.0]
