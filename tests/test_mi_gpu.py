"""GPU: ops.mutual_information / loss_ops.MILoss (csrc/mi.hip) against the fp64 restatement of tests/mi_ref.py -- value and both
gradients, the range ends, constant inputs, batching, bit-identical repeats, a gradient through align_img by finite differences --
and the centering step built on it (keymorph_amd.io.translate / estimate_translation / center_to).

The bars.  d32 = the distance of the restatement evaluated in fp32 on the CPU from its fp64 evaluation, on the same case: what
fp32 arithmetic costs in ANY summation order, times 4 for a different order.  The floor is what the kernel's accumulation format
costs by construction.  The histogram adds every window product w_a[i] w_b[j] rounded to a multiple of 2^-23, so a product is
off by at most q = 2^-24 and |dh_ij| <= n_ij q, n_ij = the number of voxels whose windows cover bin (i, j) (sum n = 16 V).
  value:     MI = sum p ln(p / (pa pb)) has dMI/dp_ij = G_ij - 1, so |dMI| <= (q / V) sum_ij n_ij (|G_ij| + 1).
  gradient:  dMI/da_v = (s_a / V) sum_ij G_ij b3'(u_a - i) b3(u_b - j) inherits |dG_ij| <= e_ij + ea_i + eb_j with the relative
             errors r = n q / h of the entry and of its two marginals, e = -ln(1 - r) where r < 1/2; an entry with r >= 1/2 may be
             rounded away altogether (G = 0 instead of G_ij) or keep one quantum: e = |G_ij| + |ln(h_ij 2^23)| + ln 2 there.
             |d grad_v| <= (s_a / V) sum_ij (e_ij + ea_i + eb_j) |b3'(u_a - i)| b3(u_b - j), and the floor of the relative L2
             error is the L2 norm of that bound over the L2 norm of the fp64 gradient.
All of it is computed from the fp64 restatement; nothing comes from the kernel's output."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mi_ref
from tests import sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
Q = 2.0 ** -24


def _pair(shape, seed):
    a, b = mi_ref.smooth_pair(shape, seed)
    if shape[0] > 1:                                   # another range per sample
        for n in range(1, shape[0]):
            a[n] = a[n] * (3.0 * n) - 7.0
            b[n] = b[n] * 0.125 + 100.0 * n
    return a, b


# name -> (shape, seed, bins, range_a, range_b)
CASES = {
    "tiny_ragged": ((1, 1, 5, 6, 7), 1, 32, None, None),                 # fewer voxels than one workgroup
    "batch_ranges": ((2, 1, 16, 16, 16), 2, 32, None, None),
    "odd_box": ((1, 1, 24, 20, 36), 3, 32, None, None),
    "two_flushes": ((1, 1, 40, 40, 40), 4, 32, None, None),              # 8 workgroups, two flushes of the LDS tables each
    "bins8": ((1, 1, 24, 20, 36), 3, 8, None, None),
    "bins64": ((1, 1, 24, 20, 36), 3, 64, None, None),
    "given_ranges": ((1, 1, 16, 16, 16), 5, 32, (-0.5, 1.5), (0.25, 0.75)),   # one range wider, one narrower than the data
}


def _derivative_matrix(x, lo, hi, bins):
    s = (bins - 3) / (hi - lo) if hi > lo else torch.zeros((), dtype=x.dtype)
    u = ((x - lo) * s + 1).clamp(1, bins - 2)
    k0 = (torch.floor(u).long() - 1).clamp(0, bins - 4)
    t = u - (k0 + 1)
    d = torch.stack([-0.5 * (1 - t) ** 2, 1.5 * t * t - 2 * t, -1.5 * t * t + t + 0.5, 0.5 * t * t], dim=1)
    k = k0[:, None] + torch.arange(4)[None, :]
    return torch.zeros(x.numel(), bins, dtype=x.dtype).scatter(1, k, d), torch.zeros(x.numel(), bins, dtype=x.dtype).scatter(
        1, k, torch.ones_like(d)), s


def _floors(a, b, bins, range_a, range_b, da, db):
    """The format's floors for one sample (fp64 tensors): (value, relative L2 of da, of db)."""
    a, b = a.reshape(-1), b.reshape(-1)
    V = a.numel()
    ra = range_a or (float(a.min()), float(a.max()))
    rb = range_b or (float(b.min()), float(b.max()))
    lo_a, hi_a, lo_b, hi_b = (torch.tensor(v, dtype=F64) for v in (*ra, *rb))
    wa, wb = mi_ref.window_matrix(a, lo_a, hi_a, bins), mi_ref.window_matrix(b, lo_b, hi_b, bins)
    dwa, ca, sa = _derivative_matrix(a, lo_a, hi_a, bins)
    dwb, cb, sb = _derivative_matrix(b, lo_b, hi_b, bins)
    h, n = wa.t() @ wb, ca.t() @ cb
    G = mi_ref.log_ratio(h / V)
    value = Q / V * float((n * (G.abs() + 1)).sum())
    r = torch.where(h > 0, n * Q / h.clamp_min(1e-300), torch.zeros_like(h))
    rough = G.abs() + torch.log(h.clamp_min(2.0 ** -23) * 2.0 ** 23).abs() + math.log(2)
    e = torch.where(r < 0.5, -torch.log1p(-r.clamp_max(0.5)), rough)
    e = torch.where((h == 0) & (n > 0), torch.zeros_like(e), e)         # exactly empty in both: G = 0 in both
    ha, hb = h.sum(1), h.sum(0)
    ea = -torch.log1p(-(n.sum(1) * Q / ha.clamp_min(1e-300)).clamp_max(0.5))
    eb = -torch.log1p(-(n.sum(0) * Q / hb.clamp_min(1e-300)).clamp_max(0.5))
    E = e + ea[:, None] + eb[None, :]
    bound_a = float(sa) / V * ((dwa.abs() @ E) * wb).sum(1)
    bound_b = float(sb) / V * ((dwb.abs() @ E.t()) * wa).sum(1)
    na, nb = float(da.norm()), float(db.norm())
    return value, (float(bound_a.norm()) / na if na > 0 else 0.0), (float(bound_b.norm()) / nb if nb > 0 else 0.0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, the fp64 and fp32 evaluations of the restatement and the bars of one case, computed once."""
    shape, seed, bins, ra, rb = CASES[name]
    a, b = _pair(shape, seed)
    mi64, da64, db64 = mi_ref.evaluate(a, b, bins, ra, rb, F64)
    mi32, da32, db32 = mi_ref.evaluate(a, b, bins, ra, rb, torch.float32)
    bars = []
    for n in range(shape[0]):
        fv, fa, fb = _floors(a[n].to(F64), b[n].to(F64), bins, ra, rb, da64[n], db64[n])
        d_v = abs(float(mi32[n]) - float(mi64[n]))
        d_a = float((da32[n].to(F64) - da64[n]).norm() / da64[n].norm())
        d_b = float((db32[n].to(F64) - db64[n]).norm() / db64[n].norm())
        bars.append({"value": max(4 * d_v, fv), "da": max(4 * d_a, fa), "db": max(4 * d_b, fb),
                     "d32": (d_v, d_a, d_b), "floor": (fv, fa, fb)})
    return a, b, mi64, da64, db64, bars


def run(a, b, bins=32, ra=None, rb=None, need=(True, True)):
    from keymorph_amd import ops
    a = a.to(DEV).requires_grad_(need[0])
    b = b.to(DEV).requires_grad_(need[1])
    mi = ops.mutual_information(a, b, bins, ra, rb)
    mi.sum().backward()
    return mi.detach(), a.grad, b.grad


@pytest.mark.parametrize("name", list(CASES))
def test_value_and_gradients_match_fp64(name):
    _, _, bins, ra, rb = CASES[name]
    a, b, mi64, da64, db64, bars = reference(name)
    mi, da, db = run(a, b, bins, ra, rb)
    assert mi.dtype == torch.float32 and mi.shape == (a.shape[0],) and da.shape == a.shape and db.shape == b.shape
    for n in range(a.shape[0]):
        ev = abs(float(mi[n]) - float(mi64[n]))
        ea = float((da[n].cpu().to(F64) - da64[n]).norm() / da64[n].norm())
        eb = float((db[n].cpu().to(F64) - db64[n]).norm() / db64[n].norm())
        print(f"{name}[{n}]: MI {float(mi64[n]):.6f}  |dMI| {ev:.3e}  relL2 da {ea:.3e} db {eb:.3e}  fp32-CPU distance "
              f"{bars[n]['d32']}  format floor {bars[n]['floor']}")
        assert ev <= bars[n]["value"], (name, n, ev, bars[n])
        assert ea <= bars[n]["da"] and eb <= bars[n]["db"], (name, n, ea, eb, bars[n])


def test_range_ends_sit_on_the_last_knots():
    """The minimum voxel has u = 1 (taps 1/6, 4/6, 1/6 on bins 0..2), the maximum u = B - 2 (the same on bins B-3..B-1, nothing
    at index B): two-valued images put their whole mass on those 3 x 3 corners, and MI is the closed form."""
    from keymorph_amd import ops
    B = 16
    g = torch.Generator().manual_seed(0)
    a = (torch.rand(1, 1, 9, 10, 11, generator=g) < 0.3).float() * 5.0 - 2.0
    b = torch.where(torch.rand(a.shape, generator=g) < 0.8, a, 1.0 - a)        # mostly follows a, else the other value
    mi, G = ops._mi_table(a.to(DEV), b.to(DEV), B)
    G = G[0].cpu()
    mask = torch.zeros(B, B, dtype=torch.bool)
    for i in (0, 1, 2, B - 3, B - 2, B - 1):
        for j in (0, 1, 2, B - 3, B - 2, B - 1):
            mask[i, j] = True
    assert (G[~mask] == 0).all() and (G[mask] != 0).any()
    ref = mi_ref.evaluate(a, b, B, grads=False)[0]
    # the format's floor in its crudest form: (q / V) sum n (|G| + 1) <= 16 q (max|G| + 1), max|G| < 9 here
    assert float(G.abs().max()) < 9 and abs(float(mi[0]) - float(ref[0])) <= 16 * Q * 10
    assert float(mi[0]) > 0.1


def test_constant_input_gives_exact_zeros():
    a, b = _pair((1, 1, 10, 12, 14), 6)
    c = torch.full_like(a, 0.37)
    for x, y in ((a, c), (c, b), (c, c)):
        mi, dx, dy = run(x, y)
        assert float(mi[0]) == 0.0
        assert (dx == 0).all() and (dy == 0).all()
    mi, dx, dy = run(a, b, 32, (0.5, 0.5), None)                              # a degenerate caller range: the same
    assert float(mi[0]) == 0.0 and (dx == 0).all() and (dy == 0).all()


def test_gradient_only_where_requested():
    a, b = _pair((1, 1, 10, 12, 14), 6)
    _, da, db = run(a, b)
    _, da1, none_b = run(a, b, need=(True, False))
    assert none_b is None and torch.equal(da1, da)
    _, none_a, db1 = run(a, b, need=(False, True))
    assert none_a is None and torch.equal(db1, db)


def test_batch_equals_single_samples():
    from keymorph_amd import ops
    a, b = _pair((3, 1, 14, 12, 18), 7)
    mi, da, db = run(a, b)
    _, G = ops._mi_table(a.to(DEV), b.to(DEV))
    for n in range(3):
        mi1, da1, db1 = run(a[n:n + 1], b[n:n + 1])
        assert torch.equal(mi1[0], mi[n]) and torch.equal(da1[0], da[n]) and torch.equal(db1[0], db[n])
        assert torch.equal(ops._mi_table(a[n:n + 1].to(DEV), b[n:n + 1].to(DEV))[1][0], G[n])


def test_repeat_runs_are_bit_identical():
    from keymorph_amd import ops
    a, b, *_ = reference("two_flushes")
    first = run(a, b) + (ops._mi_table(a.to(DEV), b.to(DEV))[1],)
    for _ in range(3):
        again = run(a, b) + (ops._mi_table(a.to(DEV), b.to(DEV))[1],)
        for x, y in zip(first, again):
            assert torch.equal(x, y)


def test_miloss_is_minus_the_mean():
    from keymorph_amd.loss_ops import MILoss
    from keymorph_amd import ops
    a, b, mi64, _, _, bars = reference("batch_ranges")
    loss = MILoss()(a.to(DEV), b.to(DEV))
    assert loss.shape == () and abs(float(loss) + float(mi64.mean())) <= max(bar["value"] for bar in bars) + 2.0 ** -23
    assert torch.equal(loss, -ops.mutual_information(a.to(DEV), b.to(DEV), 32).mean())
    assert torch.equal(MILoss(bins=8)(a.to(DEV), b.to(DEV)), -ops.mutual_information(a.to(DEV), b.to(DEV), 8).mean())


def test_gradient_through_align_img_matches_finite_differences():
    """d(-MI)/d(grid) of MILoss()(align_img(grid, moving), fixed) at 16^3 with an affine grid from the HIP grid generator, against
    central differences of the fp64 restatement (F.grid_sample in fp64) on a handful of grid entries."""
    from keymorph_amd import ops, synthetic
    from keymorph_amd.loss_ops import MILoss
    from keymorph_amd.utils import align_img
    S = 16
    f, m = _pair((1, 1, S, S, S), 8)
    mat = synthetic.random_affine_matrix(5, DEV)[:1, :3, :].contiguous().requires_grad_()
    grid = ops.affine_grid(mat, (S, S, S))
    grid.retain_grad()
    loss = MILoss()(align_img(grid, m.to(DEV)), f.to(DEV))
    loss.backward()
    assert mat.grad is not None and torch.isfinite(mat.grad).all() and mat.grad.abs().sum() > 0
    g64, m64, f64 = grid.detach().cpu().double(), m.double(), f.double()

    # no gradient flows through the ranges (the definition), so the differences hold them at the unperturbed image's minimum
    # and maximum -- the same numbers the automatic range gives at the base point
    base = F.grid_sample(m64, g64, mode="bilinear", padding_mode="border", align_corners=False)
    fixed_range = (float(base.min()), float(base.max()))

    def host(gr):
        return -float(mi_ref.mutual_information(F.grid_sample(m64, gr, mode="bilinear", padding_mode="border",
                                                              align_corners=False), f64, range_a=fixed_range)[0])
    assert abs(host(g64) - float(loss.detach())) < 1e-5
    # the entries: the twelve largest of the fp64 restatement's OWN autograd gradient (nothing of the kernel's output chooses
    # them), so that the LC2 test's bar, 2e-3 relative + 1e-6, is about entries that carry gradient
    gr = g64.clone().requires_grad_()
    (-mi_ref.mutual_information(F.grid_sample(m64, gr, mode="bilinear", padding_mode="border", align_corners=False),
                                f64)[0]).backward()
    # ... except the minimum and the maximum voxel themselves: a step past the range's end meets the clamp from one side
    ref_grad = gr.grad.abs().clone()
    for flat in (int(base.argmin()), int(base.argmax())):
        ref_grad.reshape(-1, 3)[flat] = 0
    picks = torch.topk(ref_grad.reshape(-1), 12).indices.tolist()
    h = 1e-5
    for flat in picks:
        c, x, y, z = flat % 3, (flat // 3) % S, (flat // (3 * S)) % S, flat // (3 * S * S)
        vals = []
        for sgn in (1.0, -1.0):
            gp = g64.clone()
            gp[0, z, y, x, c] += sgn * h
            vals.append(host(gp))
        fd = (vals[0] - vals[1]) / (2 * h)
        got = float(grid.grad[0, z, y, x, c])
        print(f"grid[{z},{y},{x},{c}]: kernel {got:.6e}  finite difference {fd:.6e}  fp64 autograd {float(gr.grad[0, z, y, x, c]):.6e}")
        assert math.isfinite(got) and abs(got - fd) <= 2e-3 * abs(fd) + 1e-6, (z, y, x, c, got, fd)


# ---- centering ---------------------------------------------------------------------------------------------------------------
def test_translate_matches_fp64_grid_sample():
    """translate() against the grid formula in fp64: its grid (the HIP grid generator on the same matrix) within fp32 rounding of
    (n - 1) / n * linspace(-1, 1, n) + 2 t / n, and its output within the sampler tests' bar of the fp64 sampler on that grid."""
    from keymorph_amd import ops
    from keymorph_amd.io import translate
    x = torch.rand(2, 2, 9, 12, 10, generator=torch.Generator().manual_seed(0))
    t = torch.tensor([[1.25, -2.5, 0.75], [-0.4, 3.0, -1.1]])
    out = translate(x.to(DEV), t.to(DEV))
    size = torch.tensor([9.0, 12.0, 10.0])
    mat = torch.cat([torch.diag((size - 1) / size).expand(2, 3, 3), (2 * t / size).unsqueeze(-1)], dim=2)
    grid = ops.affine_grid(mat.to(DEV), (9, 12, 10)).cpu()
    axes = [((n - 1) / n * torch.linspace(-1, 1, n, dtype=F64)[None, :] + 2 * t[:, k:k + 1].double() / n)
            for k, n in enumerate((9, 12, 10))]
    g64 = torch.stack([axes[2][:, None, None, :].expand(2, 9, 12, 10), axes[1][:, None, :, None].expand(2, 9, 12, 10),
                       axes[0][:, :, None, None].expand(2, 9, 12, 10)], dim=-1)
    assert float((grid.double() - g64).abs().max()) <= 4 * 2.0 ** -23
    R.assert_fwd(out.cpu().numpy(), R.grid_sample(x.numpy(), grid.numpy()), x.numpy(), "translate")
    ref = mi_ref.translate(x.double(), t.double())
    assert float((out.cpu().double() - ref).abs().max()) <= 1e-5          # fp32 grid against fp64 grid: slope 1 per voxel


def test_translate_integer_nearest_is_an_exact_shift():
    from keymorph_amd.io import translate
    x = torch.rand(1, 2, 8, 9, 10, generator=torch.Generator().manual_seed(1))
    out = translate(x.to(DEV), torch.tensor([[2.0, -1.0, 3.0]], device=DEV), "nearest").cpu()
    assert torch.equal(out[:, :, :6, 1:, :7], x[:, :, 2:, :8, 3:])
    assert torch.equal(out[:, :, 6:, 1:, :7], x[:, :, 7:8, :8, 3:].expand(1, 2, 2, 8, 7))          # border values outside


def test_translate_is_differentiable_in_t():
    from keymorph_amd.io import translate
    x = torch.rand(1, 1, 8, 9, 10, generator=torch.Generator().manual_seed(2))
    w = torch.rand(1, 1, 8, 9, 10, generator=torch.Generator().manual_seed(3))
    t = torch.tensor([[0.3, -0.6, 1.2]], device=DEV, requires_grad=True)
    (translate(x.to(DEV), t) * w.to(DEV)).sum().backward()
    t64 = t.detach().cpu().double().requires_grad_()
    (mi_ref.translate(x.double(), t64) * w.double()).sum().backward()
    assert torch.allclose(t.grad.cpu().double(), t64.grad, rtol=1e-4, atol=1e-4)


@pytest.fixture(scope="module")
def recovery():
    """The inputs validated in tests/test_mi_cpu.py at 32^3, and estimate_translation's answer with its defaults."""
    from keymorph_amd.io import estimate_translation
    fixed, moving = mi_ref.recovery_pair(32)
    return fixed, moving, estimate_translation(fixed.to(DEV), moving.to(DEV)).cpu()


def test_estimate_translation_recovers_the_shift(recovery):
    _, _, t = recovery
    err = (t[0].double() - torch.tensor(mi_ref.RECOVERY_SHIFT, dtype=F64)).abs()
    print("recovered", t[0].tolist(), "error", err.tolist())
    assert t.shape == (1, 3) and float(err.max()) <= 0.5


def test_estimate_translation_batch_equals_single_runs(recovery):
    from keymorph_amd.io import estimate_translation
    fixed, moving, t0 = recovery
    shift2 = (-1.4, 2.2, 1.7)
    fixed2, moving2 = mi_ref.recovery_pair(32, shift2, seed=9)
    t = estimate_translation(torch.cat([fixed, fixed2]).to(DEV), torch.cat([moving, moving2]).to(DEV)).cpu()
    t1 = estimate_translation(fixed2.to(DEV), moving2.to(DEV)).cpu()
    assert torch.equal(t[0], t0[0]) and torch.equal(t[1], t1[0])
    assert float((t[1].double() - torch.tensor(shift2, dtype=F64)).abs().max()) <= 0.5


def test_estimate_translation_does_not_wait_for_the_gpu(recovery):
    """One full-resolution level (no resize tables to upload) under torch's synchronisation check: any call that makes the host
    wait for the stream -- a host-to-device copy of a Python list among them -- raises."""
    from keymorph_amd.io import estimate_translation
    fixed, moving, _ = recovery
    f, m = fixed.to(DEV), moving.to(DEV)
    first = estimate_translation(f, m, shrink=(1,), iters=3)            # allocations and lazy initialisation happen here
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = estimate_translation(f, m, shrink=(1,), iters=3)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(first, again)


def test_center_to_applies_the_translation(recovery):
    from keymorph_amd.io import center_to, translate
    fixed, moving, t0 = recovery
    g = torch.Generator().manual_seed(4)
    fmask = torch.ones(fixed.shape, dtype=torch.uint8)
    mmask = torch.ones(moving.shape, dtype=torch.uint8)
    mmask[..., :3, :, :] = 0
    mmask[..., :, 29:, :] = 0
    skull = moving + 0.3 * torch.rand(moving.shape, generator=g) * (1 - mmask.float())          # outside the mask only
    aligned, mask, t = center_to(fixed.to(DEV), fmask.to(DEV), skull.to(DEV), mmask.to(DEV))
    assert mask.dtype == torch.uint8 and mask.shape == mmask.shape and aligned.dtype == torch.float32
    assert float((t[0].cpu().double() - torch.tensor(mi_ref.RECOVERY_SHIFT, dtype=F64)).abs().max()) <= 0.5
    assert torch.equal(mask, translate(mmask.float().to(DEV), t, "nearest").to(torch.uint8))
    assert torch.equal(aligned, translate(skull.to(DEV), t, "bilinear"))
    assert set(mask.unique().tolist()) <= {0, 1}
    # the mask is the input mask moved by round(t): compare with the exact integer shift of the nearest sampler
    ref = R.grid_sample_nearest(mmask.float().numpy(), _grid_of(t, moving.shape[2:]))
    assert np.array_equal(mask.cpu().numpy(), ref.astype(np.uint8))
    b = center_to(fixed.to(DEV), fmask.bool().to(DEV), skull.to(DEV), mmask.bool().to(DEV))[1]
    assert b.dtype == torch.bool and torch.equal(b, mask.bool())


def _grid_of(t, dims):
    from keymorph_amd import ops
    size = torch.tensor([float(n) for n in dims], device=t.device)
    N = t.shape[0]
    mat = torch.cat([torch.diag((size - 1) / size).expand(N, 3, 3), (2 * t / size).unsqueeze(-1)], dim=2)
    return ops.affine_grid(mat, dims).cpu().numpy()


# ---- input checks --------------------------------------------------------------------------------------------------------------
def test_input_checks():
    from keymorph_amd import ops
    from keymorph_amd._lib import KeymorphHipError
    from keymorph_amd.io import translate
    a = torch.rand(1, 1, 6, 6, 6, device=DEV)
    with pytest.raises(ValueError):
        ops.mutual_information(a, torch.rand(1, 1, 6, 6, 7, device=DEV))
    with pytest.raises(ValueError):
        ops.mutual_information(torch.rand(1, 2, 6, 6, 6, device=DEV), torch.rand(1, 2, 6, 6, 6, device=DEV))
    with pytest.raises(ValueError):
        ops.mutual_information(a[0], a[0])
    with pytest.raises(ValueError):
        ops.mutual_information(a.double(), a.double())
    with pytest.raises(ValueError):
        ops.mutual_information(a, a.half())
    with pytest.raises(KeymorphHipError):
        ops.mutual_information(a.cpu(), a)
    with pytest.raises(KeymorphHipError):
        ops.mutual_information(a, a.cpu())
    for bins in (7, 65, 0, -1, 16.5):
        with pytest.raises(ValueError):
            ops.mutual_information(a, a, bins)
    with pytest.raises(ValueError):
        ops.mutual_information(a, a, 32, (1.0, 0.0))
    with pytest.raises(ValueError):
        translate(a, torch.zeros(2, 3, device=DEV))
    with pytest.raises(ValueError):
        translate(a, torch.zeros(1, 3, device=DEV), "bicubic")
    assert ops.mutual_information(a, a, 8).shape == (1,) and ops.mutual_information(a, a, 64).shape == (1,)
