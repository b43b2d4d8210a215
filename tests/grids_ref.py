"""fp64 restatement of csrc/grids.hip (the implicit lattice, the affine grid and its adjoint, the thin-plate-spline evaluators
on the grid and on explicit points with every gradient, the augmentation matrix) and of the two kernels of csrc/losses.hip that
tests/sampler_ref.py left out (Jacobian determinant, argmax one-hot), with the bars and the case tables of their conformance
tests.  Inputs are the fp32 arrays the kernels get, cast exactly.  No GPU import.

u = eps32 / 2 (one fp32 rounding).  Every bar is derived from the operations the kernel performs, none from a run of it; all are
first-order in u.

  lattice      lin(i, n) is torch.linspace(-1, 1, n)[i] in fp32: step = fl(2 / (n - 1)), fma(step, i, -1) below the midpoint i <
               n / 2 and fma(-step, n - 1 - i, 1) from it on -- ONE rounding of an exact product-sum (the kernels' expression is
               contracted, -ffp-contract=fast).  lattice_single_rounding states that form; it equals torch's CPU values bit for bit
               and differs from the product-then-sum form (test_grids_reference_cpu.py).  An axis of one voxel is [-1].
  affine grid  a row is fma(m2, gx, fma(m0, gz, fl(m1 gy))) + m3 on exact lattice values (grid_coords.h): the product m1 gy is
               rounded and then passes three more roundings, m0 gz passes three, m2 gx two, m3 one:
                   |row - truth| <= u (3 |m0 gz| + 4 |m1 gy| + 2 |m2 gx| + |m3|).
  affine adjoint   dM[r][k] = sum_v g[v][r] p[v][k].  affine_grid_bwd_partial runs nb = min(1024, ceil(nvox / 4096)) blocks of 256
               threads; a thread adds k = ceil(nvox / (256 nb)) products into one fp32 accumulator (the first of them passes k
               roundings, fused or not), the block and grid sums are fp64, one rounding on the store:
                   |dM - truth| <= k u sum|g p| + u |truth|.
               The same kernel writes the four affine rows of the TPS-grid backward.  points_affine_rows_kernel (explicit
               points) is one block per sample: k = ceil(P / 256).
  TPS          U = d2 ln(r + e), d2 = |c - p|^2 + e, r = sqrt(d2), e = 1e-6, l = ln(r + e).  A bar is an ARITHMETIC bound plus a
               TRANSCENDENTAL ALLOWANCE.  Arithmetic, per (point, keypoint) pair:
                 d2     three rounded differences (2 u dz^2 each, <= 2 u d2 together), three links of the fma chain (<= u d2 each),
                        and the seed 1e-6f in place of 1e-6 (2.6e-14):  dd2 <= 5 u d2 + |1e-6f - 1e-6|.   dU/dd2 = l + r / (2 (r +
                        e)), so U moves by at most (|l| + 1/2) dd2.
                 log    2 log2(r + e) = log2(d2) + K y with y the integer reciprocal-square-root estimate (common.h): the
                        correction's error in natural-log units of l is <= 4.8e-8 / r (estimate within 4.8 % of 1 / r after
                        centring, log(1 + t) = t to t / 2 <= 5e-4 of itself; rsq_correction_error measures both on the CPU):
                        4.8e-8 r on U.  The fma that adds it rounds once (u |U|).
                 value  forward: d2 L rounds once, the weight w ln2 / 2 twice (constant, product): 4 u |U w| with the log's
                        rounding.  Backward dtheta_w: 2 u |U g| (the ln2 / 2 is applied to the chunk sum: 2 u more there).
                 sums   forward: T fused multiply-adds in keypoint order, term t passes T - t roundings; then the affine part (4
                        terms, each at most one product and three additions: 4 u A, A = |a0| + |a1 pz| + |a2 py| + |a3 px|) and
                        one addition u (A + S), S = sum_t |U w|.   Backward: a lane adds the voxels of a chunk of 8192 in order
                        (term j of n_c passes n_c - j roundings), the chunk sums are added in fp64, one rounding on the store.
                 dctrl  term = s G (c - p), s = sum_d w_d g_d (3 u sum|w g|), G = 2 l + r / (r + e) (kernel: fma(y, -1e-6 K',
                        fma(L, ln2, 1)): L's rounding, the ln2 constant, two fma roundings <= 4 u (2 |l| + 1)), s G, c - p and
                        the product with it one rounding each: 9 u M with M = sum|w g| (2 |l| + 1) |c - p|.  Approximations,
                        taken together: with t = e / r and t^ its estimate the kernel forms ln d2 + 2 t^ + 1 - t^ = ln d2 + 1 + t^,
                        and G = ln d2 + 2 ln(1 + t) + 1 / (1 + t) = ln d2 + 1 + t - t^3 / 3 + ... (the t^2 of the two series
                        cancel): |t^ - t| + t^3 <= 0.048 t + t^3; dG/dd2 <= 1.0005 / d2.  The row-hoisted arm (W % 256 == 0) adds a stage's 256 factors first and
                        multiplies once by c_z - p_z (c_y - p_y): 256 + 1 roundings, then one per stage.
                 dpts   tps_points_bwd_pts_kernel: d2 by three products and three additions (each square passes at most four:
                        dd2 <= 6 u d2 + 2.6e-14), r + e, L ln2 (constant, product), r rcp, the sum: 6 u (2 |l| + 1); s 3 u; s G,
                        c - p: 11 u M together; T + 3 terms in order.  No approximation; sqrt, log2 and rcp are hardware.
               Allowance: the accuracies of the hardware log2, sqrt and rcp are stated in no document, so none is assumed.  It is
               2 x the worst error of the fp32 CPU oracle against the fp64 truth on the same case, per output array (forward,
               dtheta_w, dctrl, dpts): the factor 2 because the kernel takes log2 of d2, which has twice the exponent range of ln
               r, through an instruction of unstated accuracy while the oracle calls libm.  The affine rows get none.
  augment      M = Mz (Ms (Mt (R3 (R2 R1)))), five 4 x 4 fp32 products, an element a sum of four products in order: 4 u |A| |B|
               per product, pushed through the nesting with the factors' own bounds (|A| E(B) + E(A) |B|); cosf / sinf enter with
               2 x the worst error of the fp32 CPU oracle's cos / sin on the case's own angles.
  Jacobian     J[a][c] = 0.5 f+ - 0.5 f- (halving is exact: one rounding, u |J0|), + 1 on the diagonal (u |J|).  det in the
               kernel's association: a minor ab - cd is at most two roundings per product, times its J one, and two additions of
               the three terms: each of the six triple products passes at most 5 roundings: 5 u sum_6 |J J J| + sum_e dJ_e
               |cofactor|_abs.  mean: the mean of the bars.  std = sqrt(var): sum_i |det_i - mean| bar_i / (n std) (the
               derivative of var), and sqrt(mean bar^2) where the truth's std is 0; the fp64 sums add 64 x 2^-53 of their
               magnitudes.  Counts of det <= 0 are exact where no truth other than an exact zero lies within its bar of zero.
  argmax       torch.argmax's rule: the first NaN if there is one, otherwise the first maximum (+0 == -0).
"""
import functools

import numpy as np
import torch

from oracle import keymorph_oracle as O

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
U = EPS32 / 2
E64 = 1e-6
E32 = float(np.float32(1e-6))
D_SEED = abs(E32 - E64)                   # the kernels' 1e-6f against the reference's 1e-6
LOG_CORR = 4.8e-8                         # / r, on ln(r + e): common.h; measured 4.755e-8 by rsq_correction_error
EST_REL = 0.048                           # the centred estimate of 1 / r; measured 0.0475
RSQ_CENTRE = float(np.float32(0.98636))
K_LOG2X2 = float(np.float32(2.0e-6) * np.float32(0.98636) / np.float32(0.6931471805599453))
VCHUNK, VSTAGE, KTILE = 8192, 256, 512
TPS_MAX_T = 2048


def _d(a):
    return np.asarray(a, np.float64)


def _t(a, dtype):
    return torch.from_numpy(np.array(a, copy=True)).to(dtype)


# ------------------------------------------------------------------------------------------------------------ lattice
def lattice(n):
    """the fp32 values of torch.linspace(-1, 1, n) on the CPU"""
    return torch.linspace(-1, 1, int(n)).numpy().astype(F32)


def lattice_step(n):
    return F32(2) / F32(n - 1) if n > 1 else F32(0)


def lattice_single_rounding(n):
    """fma(step, i, -1) for i < n / 2, fma(-step, n - 1 - i, 1) from there on, the product-sum exact in fp64 (24 + 12 bits) and
    rounded once; [-1] for n = 1"""
    if n == 1:
        return np.array([-1], F32)
    i = np.arange(n, dtype=np.float64)
    s = float(lattice_step(n))
    return np.where(i < n // 2, s * i - 1.0, 1.0 - s * (n - 1 - i)).astype(F32)


def lattice_two_roundings(n):
    """the same with the product rounded on its own: NOT what torch or the kernels compute"""
    if n == 1:
        return np.array([-1], F32)
    i = np.arange(n)
    s = lattice_step(n)
    return np.where(i < n // 2, F32(-1) + s * i.astype(F32), F32(1) - s * (n - 1 - i).astype(F32)).astype(F32)


def lattice_points(shape):
    """(D H W, 3) float32: the lattice in (z, y, x) order, x fastest"""
    z, y, x = np.meshgrid(*(lattice(n) for n in shape), indexing="ij")
    return np.stack([z, y, x], -1).reshape(-1, 3)


def identity_grid(shape):
    """(D, H, W, 3) float32: the lattice flipped to xyz, what affine_grid(identity) writes bit for bit"""
    return np.ascontiguousarray(lattice_points(shape)[:, ::-1]).reshape(*shape, 3)


# -------------------------------------------------------------------------------------------------------- affine grid
def affine_grid(M, shape, dtype=np.float64):
    """M (3, 4), rows (z, y, x) outputs -> (D, H, W, 3) in xyz order"""
    M, p = np.asarray(M, dtype), lattice_points(shape).astype(dtype)
    out = p @ M[:, :3].T + M[:, 3]
    return np.ascontiguousarray(out[:, ::-1]).reshape(*shape, 3)


def affine_grid_bar(M, shape):
    M, p = np.abs(_d(M)), np.abs(_d(lattice_points(shape)))
    b = U * (3 * p[:, 0:1] * M[:, 0] + 4 * p[:, 1:2] * M[:, 1] + 2 * p[:, 2:3] * M[:, 2] + M[:, 3])
    return np.ascontiguousarray(b[:, ::-1]).reshape(*shape, 3)


def affine_bwd_geometry(nvox):
    """(blocks, terms per thread) of affine_grid_bwd_partial"""
    nb = max(1, min(1024, -(-nvox // (256 * 16))))
    return nb, -(-nvox // (256 * nb))


def affine_grid_adjoint(cot, shape, dtype=np.float64):
    """cot (D, H, W, 3) in xyz order -> dM (3, 4) and sum|terms|"""
    g = np.asarray(cot, dtype).reshape(-1, 3)[:, ::-1]
    p1 = np.concatenate([lattice_points(shape).astype(dtype), np.ones((g.shape[0], 1), dtype)], 1)
    return g.T @ p1, np.abs(g).T @ np.abs(p1)


def emulate_strided_sum(terms, nthreads):
    """the kernels' own order in float32: thread i adds terms i, i + nthreads, ... in fp32 (products rounded on their own: fusing
    them only removes roundings), the threads are added in fp64, one rounding on the store.  terms (P, ...) float32"""
    terms = np.asarray(terms, F32)
    k = -(-terms.shape[0] // nthreads)
    buf = np.zeros((k * nthreads,) + terms.shape[1:], F32)
    buf[:terms.shape[0]] = terms
    buf = buf.reshape((k, nthreads) + terms.shape[1:])
    acc = np.zeros(buf.shape[1:], F32)
    for j in range(k):
        acc = acc + buf[j]
    return acc.astype(np.float64).sum(0).astype(F32)


def emulate_affine_adjoint(cot, shape):
    """affine_grid_bwd_partial + final in float32 / fp64 as the kernels order them -> dM (3, 4) float32"""
    g = np.asarray(cot, F32).reshape(-1, 3)[:, ::-1]
    p1 = np.concatenate([lattice_points(shape), np.ones((g.shape[0], 1), F32)], 1)
    return emulate_strided_sum(g[:, :, None] * p1[:, None, :], 256 * affine_bwd_geometry(g.shape[0])[0])


def affine_adjoint_bar(truth, mag, nvox):
    return affine_bwd_geometry(nvox)[1] * U * mag + U * np.abs(truth)


# ---------------------------------------------------------------------------------------------------------------- TPS
def rsq_estimate(d2):
    """tps_rsq_est: 0x5f3759df - (bits(d2) >> 1), exact integer arithmetic"""
    b = np.asarray(d2, F32).view(np.uint32)
    return (np.uint32(0x5f3759df) - (b >> np.uint32(1))).view(F32)


def rsq_correction_error(d2):
    """r x |K y ln2 / 2 - ln(1 + e / r)| for fp32 d2 >= 1e-6, in fp64: the quantity common.h bounds by 4.8e-8; and the relative
    error of the centred estimate of 1 / r"""
    d2 = np.asarray(d2, F32)
    r = np.sqrt(_d(d2))
    y = _d(rsq_estimate(d2))
    return r * np.abs(K_LOG2X2 * y * np.log(2.0) / 2 - np.log1p(E64 / r)), np.abs(RSQ_CENTRE * y * r - 1)


def tps_points(theta, ctrl, pts, dtype=np.float64):
    """theta (T + 4, 3), ctrl (T, 3), pts (P, 3) -> (P, 3): [1, p] theta_aff + sum_t U_t theta_w[t]"""
    th, c, p = (np.asarray(a, dtype) for a in (theta, ctrl, pts))
    T = c.shape[0]
    e = dtype(1e-6)
    diff = c[None] - p[:, None]
    r = np.sqrt((diff * diff).sum(-1) + e)
    Um = r ** 2 * np.log(r + e)
    return np.concatenate([np.ones((p.shape[0], 1), dtype), p], 1) @ th[T:] + Um @ th[:T]


def tps_grid(theta, ctrl, shape, dtype=np.float64):
    return np.ascontiguousarray(tps_points(theta, ctrl, lattice_points(shape), dtype)[:, ::-1]).reshape(*shape, 3)


def tps_autograd(theta, ctrl, pts, cot, dtype=torch.float64):
    """the oracle's own function on tensors of `dtype`: out, dtheta, dctrl, dpts as float64 arrays (one sample)"""
    a = [_t(x, dtype)[None].requires_grad_(True) for x in (theta, ctrl, pts)]
    out = O.tps_transform_points(*a)
    (out * _t(cot, dtype)[None]).sum().backward()
    return [out.detach()[0].double().numpy()] + [x.grad[0].double().numpy() for x in a]


def tps_bars(theta, ctrl, pts, cot, grid_shape=None):
    """arithmetic bars of one sample in the points convention (ij order; a grid's cotangent and output flipped by the caller):
    dict out (P, 3), dw (T, 3), daff (4, 3), dctrl (T, 3), dpts (P, 3; explicit points only).  grid_shape: the implicit-grid
    kernels (affine rows by affine_grid_bwd_partial, the row-hoisted backward where W % 256 == 0)"""
    th, c, p, g = _d(theta), _d(ctrl), _d(pts), _d(cot)
    T, P = c.shape[0], p.shape[0]
    w, a = th[:T], th[T:]
    rows = grid_shape is not None and grid_shape[2] % VSTAGE == 0
    diff = c[None] - p[:, None]                                   # (P, T, 3), exact in fp64
    d2 = (diff * diff).sum(-1) + E64
    r = np.sqrt(d2)
    l = np.log(r + E64)
    Uabs = np.abs(d2 * l)
    dd2 = 5 * U * d2 + D_SEED
    e_u = (np.abs(l) + 0.5) * dd2 + LOG_CORR * r                  # on U, before the roundings of its own value
    # position of a voxel in its chunk: term j of n_c passes n_c - j roundings
    j = np.arange(P)
    n_c = np.minimum(VCHUNK, P - (j // VCHUNK) * VCHUNK)
    pas = (n_c - j % VCHUNK).astype(np.float64)[:, None]          # (P, 1)
    bars = {}
    # forward
    A = np.abs(a[0]) + np.abs(p) @ np.abs(a[1:])
    S = Uabs @ np.abs(w)
    seq = (Uabs * (T - np.arange(T))) @ np.abs(w)
    bars["out"] = (e_u + 4 * U * Uabs) @ np.abs(w) + U * seq + 4 * U * A + U * (A + S)
    # dtheta_w
    ga = np.abs(g)
    truth_w = (d2 * l).T @ g
    bars["dw"] = (e_u + 2 * U * Uabs).T @ ga + U * (Uabs * pas).T @ ga + 2 * U * Uabs.T @ ga + U * np.abs(truth_w)
    # dctrl
    swg = ga @ np.abs(w).T                                        # (P, T): sum_d |w_d g_d|
    Dg = 2 * np.abs(l) + 1
    t = E64 / r
    apx = EST_REL * t + t ** 3 + 1.0005 * dd2 / d2
    M = (swg * Dg)[..., None] * np.abs(diff)                      # (P, T, 3)
    per = 9 * U * M + (swg * apx)[..., None] * np.abs(diff)
    G = 2 * l + r / (r + E64)
    truth_c = np.einsum("pt,ptk->tk", (g @ w.T) * G, diff)
    seq_c = (M * pas[..., None]).sum(0)
    if rows:
        hoisted = (VSTAGE + 1 + -(-np.minimum(VCHUNK, P) // VSTAGE)) * M.sum(0)
        seq_c[:, :2] = hoisted[:, :2]
    bars["dctrl"] = per.sum(0) + U * seq_c + U * np.abs(truth_c)
    # affine rows
    p1 = np.concatenate([np.ones((P, 1)), p], 1)
    truth_a, mag_a = p1.T @ g, np.abs(p1).T @ ga
    k = affine_bwd_geometry(P)[1] if grid_shape is not None else -(-P // 256)
    bars["daff"] = k * U * mag_a + U * np.abs(truth_a)
    # dpts (explicit points)
    if grid_shape is None:
        dd2p = 6 * U * d2 + D_SEED
        perp = 11 * U * M + (swg * 1.0005 * dd2p / d2)[..., None] * np.abs(diff)
        bars["dpts"] = perp.sum(1) + (T + 3) * U * (M.sum(1) + ga @ np.abs(a[1:]).T)
    return bars


ALLOWED = ("out", "dw", "dctrl", "dpts")         # the outputs that pass through a transcendental


def tps_truth(theta, ctrl, pts, cot, grid_shape=None):
    """one sample -> (truth, arith, allow, oracle_err): dicts over out, dw, daff, dctrl (, dpts), the allowance a scalar per
    array (0 for daff).  oracle_err of daff is that of the float32 emulation of the kernels' summation order: their lanes hold at
    most ceil(P / 256) terms before fp64 takes over, which a single fp32 sum over P terms on the CPU cannot match"""
    T = np.shape(ctrl)[0]
    t64 = tps_autograd(theta, ctrl, pts, cot)
    t32 = tps_autograd(theta, ctrl, pts, cot, torch.float32)
    split = lambda o: {"out": o[0], "dw": o[1][:T], "daff": o[1][T:], "dctrl": o[2], "dpts": o[3]}      # noqa: E731
    truth, orc = split(t64), split(t32)
    arith = tps_bars(theta, ctrl, pts, cot, grid_shape)
    if grid_shape is not None:
        truth.pop("dpts")
    p1 = np.concatenate([np.ones((np.shape(pts)[0], 1), F32), np.asarray(pts, F32)], 1)
    nthreads = 256 * (affine_bwd_geometry(p1.shape[0])[0] if grid_shape is not None else 1)
    orc["daff"] = emulate_strided_sum(p1[:, :, None] * np.asarray(cot, F32)[:, None, :], nthreads)      # the kernels' order
    oerr = {k: np.abs(orc[k] - truth[k]) for k in truth}
    allow = {k: (2 * float(oerr[k].max(initial=0.0)) if k in ALLOWED else 0.0) for k in truth}
    return truth, arith, allow, oerr


def tps_fwd_arm(shape):
    """the instance kmh_tps_grid_fwd launches: voxels per lane and row hoisting"""
    W = shape[2]
    return "w8" if W % 8 == 0 else ("w4" if W % 4 == 0 else "plain")


def tps_geometry(T, P, shape=None):
    """dispatch facts of a case as plain arithmetic"""
    tv = 8 if shape is not None and shape[2] % 8 == 0 else 4
    return {"fwd_arm": "explicit" if shape is None else tps_fwd_arm(shape), "fwd_blocks": -(-P // (256 * tv)),
            "vector_stores": P % 4 == 0, "bwd_rows": shape is not None and shape[2] % VSTAGE == 0, "chunks": -(-P // VCHUNK),
            "ragged_stage": (P % VCHUNK) % VSTAGE != 0, "stages_per_row": (shape[2] // VSTAGE if shape is not None else 0),
            "ktiles": -(-T // KTILE), "unroll_tail": T % 4, "lds_limit": T == TPS_MAX_T}


# ------------------------------------------------------------------------------------------------------- augmentation
def augment_matrix(scale, offset, theta, shear, dtype=torch.float64):
    """(B, 3), (B, 3), (B, 3), (B, 6) float32 -> (B, 4, 4): the oracle's function on tensors of `dtype`"""
    return O.augment_matrix(*(_t(a, dtype) for a in (scale, offset, theta, shear))).double().numpy()


def trig_allowance(theta):
    th = np.asarray(theta, F32)
    return 2 * float(max(np.abs(_d(np.cos(th)) - np.cos(_d(th))).max(), np.abs(_d(np.sin(th)) - np.sin(_d(th))).max()))


def augment_bar(scale, offset, theta, shear, trig=1.0):
    """(B, 4, 4) bound of five nested fp32 products with `trig` x the trigonometric allowance of the case"""
    sc, of, th, sh = (_d(a) for a in (scale, offset, theta, shear))
    B = sc.shape[0]
    eps = trig * trig_allowance(theta)
    eye = lambda: np.tile(np.eye(4), (B, 1, 1))                                                      # noqa: E731
    c, s = np.cos(th), np.sin(th)
    r1, r2, r3, ms, mt, mz = eye(), eye(), eye(), eye(), eye(), eye()
    e1, e2, e3 = np.zeros((B, 4, 4)), np.zeros((B, 4, 4)), np.zeros((B, 4, 4))
    for R, E, k, (i, j) in ((r1, e1, 0, (1, 2)), (r2, e2, 1, (2, 0)), (r3, e3, 2, (0, 1))):
        R[:, i, i], R[:, i, j], R[:, j, i], R[:, j, j] = c[:, k], -s[:, k], s[:, k], c[:, k]
        E[:, i, i] = E[:, i, j] = E[:, j, i] = E[:, j, j] = eps
    for k in range(3):
        ms[:, k, k], mt[:, k, 3] = sc[:, k], of[:, k]
    for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))):
        mz[:, i, j] = sh[:, k]

    def mm(A, EA, Bm, EB):
        absA, absB = np.abs(A), np.abs(Bm)
        return A @ Bm, absA @ EB + EA @ absB + EA @ EB + 4 * U * (absA @ absB)

    zero = np.zeros((B, 4, 4))
    v, e = mm(r2, e2, r1, e1)
    v, e = mm(r3, e3, v, e)
    for m in (mt, ms, mz):
        v, e = mm(m, zero, v, e)
    return e


AUGMENT_B = (1, 64, 65)


def augment_case(B):
    """B = 1: angle 0, zero shear, unit scale (the identity, exactly).  B = 64: the special angles (0, +-pi, pi / 2, +-2 pi as
    fp32) in the first samples, random angles after them, generic parameters.  B = 65: random, generic (a second block)"""
    r = np.random.default_rng([B, 31])
    if B == 1:
        return (np.ones((1, 3), F32), np.zeros((1, 3), F32), np.zeros((1, 3), F32), np.zeros((1, 6), F32))
    theta = r.uniform(-np.pi, np.pi, (B, 3)).astype(F32)
    if B == 64:
        sp = np.array([0, np.pi, -np.pi, np.pi / 2, 2 * np.pi, -2 * np.pi], F32)
        theta[:6] = np.stack([sp, np.roll(sp, 1), np.roll(sp, 2)], 1)
        theta[6] = 0
    scale, offset, shear = (1 + 0.2 * r.standard_normal((B, 3))).astype(F32), (0.2 * r.standard_normal((B, 3))).astype(F32), \
        (0.1 * r.standard_normal((B, 6))).astype(F32)
    if B == 64:
        scale[6], shear[6], shear[7] = 1, 0, 0
    return scale, offset, theta, shear


# ----------------------------------------------------------------------------------------------------------- Jacobian
def jacobian_det(disp, dtype=torch.float64):
    """disp (3, D, H, W) -> (D - 4, H - 4, W - 4): the oracle's central differences and expansion on tensors of `dtype`"""
    return O.jacobian_determinant(_t(disp, dtype)[None]).double().numpy()


def jacobian_bar(disp):
    """per-voxel bound of the fp32 determinant (module docstring)"""
    f = _d(disp)
    D, H, W = f.shape[1:]
    def sh(ax, k):                            # the interior (cropped by 2) shifted by k along ax
        s = [slice(2, n - 2) for n in (D, H, W)]
        s[ax] = slice(2 + k, (D, H, W)[ax] - 2 + k)
        return (slice(None),) + tuple(s)

    J = np.stack([0.5 * f[sh(ax, 1)] - 0.5 * f[sh(ax, -1)] for ax in range(3)])          # [axis][component]
    dJ = U * np.abs(J)
    for k in range(3):
        J[k, k] += 1.0
        dJ[k, k] += U * np.abs(J[k, k])
    Ja = np.abs(J)
    six = 0.0
    bar = 0.0
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for jx in range(3):
            j1, j2 = (jx + 1) % 3, (jx + 2) % 3
            cof = Ja[i1, j1] * Ja[i2, j2] + Ja[i1, j2] * Ja[i2, j1]
            bar = bar + dJ[i, jx] * cof
            if i == 0:
                six = six + Ja[0, jx] * cof
    return bar + 5 * U * six


def jacobian_stats(det, bar):
    """{mean, std (ddof 0), count of det <= 0} of fp64 determinants and the bars of mean and std"""
    det, bar = _d(det).ravel(), _d(bar).ravel()
    n = det.size
    mean, std = det.mean(), det.std()
    fl = 64 * 2.0 ** -53
    bmean = bar.mean() + fl * np.abs(det).mean()
    if std > 0:
        bstd = (np.abs(det - mean) * bar).sum() / (n * std) + fl * ((det * det).mean() + mean * mean) / (2 * std)
    else:
        bstd = float(np.sqrt((bar * bar).mean()))
    return (mean, std, int((det <= 0).sum())), (bmean, bstd)


JAC_CASES = ("one_interior", "small", "small_fold", "exact_zero", "big")


@functools.lru_cache(maxsize=None)
def jacobian_case(name):
    """(3, D, H, W) float32, read-only.  exact_zero: disp_z = -z (voxel units), so J[0][0] = 0 and the other entries of its
    column are 0: every determinant is exactly 0.  small_fold: displacements of several voxels.  big: 106^3, past the 4096 x 256
    interior voxels of one grid pass, smooth, 13 688 folded voxels, the nearest determinant 8 bars from zero"""
    shape = {"one_interior": (5, 5, 5), "small": (5, 6, 9), "small_fold": (5, 6, 9), "exact_zero": (5, 6, 9), "big": (106, 106, 106)}[name]
    r = np.random.default_rng([len(name), shape[2], 11])
    if name == "big":
        z, y, x = np.meshgrid(*(np.linspace(-1, 1, n) for n in shape), indexing="ij")
        d = (6 * np.stack([4 * np.sin(3 * y) * x, 5 * np.cos(2 * z + x), 3 * z * y + np.sin(4 * x)])).astype(F32)
    else:
        d = (r.standard_normal((3,) + shape) * (3.0 if name == "small_fold" else 0.2)).astype(F32)
    if name == "exact_zero":
        d[0] = -np.arange(shape[0], dtype=F32)[:, None, None]
    d.setflags(write=False)
    return d


# ------------------------------------------------------------------------------------------------------------- argmax
def argmax_onehot(pred):
    """pred (N, C, V) -> one-hot float32 of torch.argmax over the channels (first NaN, else first maximum)"""
    x = np.asarray(pred, F32)
    nan = np.isnan(x)
    idx = np.where(nan.any(1), nan.argmax(1), np.where(nan, -np.inf, x).argmax(1))        # argmax: the first of equals
    return (np.arange(x.shape[1])[None, :, None] == idx[:, None, :]).astype(F32)


ARGMAX_C = (1, 2, 5)
ARGMAX_V = (1, 255, 256, 257)
ARGMAX_CLASSES = ("random", "all_equal", "signed_zero", "inf", "nan_first", "nan_middle", "nan_last", "nan_two")


def argmax_case(cls, C, V, N=2):
    r = np.random.default_rng([sum(map(ord, cls)), C, V])
    x = (np.round(r.standard_normal((N, C, V)) * 2) / 2).astype(F32)          # ties everywhere
    if cls == "all_equal":
        x[:] = x[:, :1]
    elif cls == "signed_zero":
        x[:] = np.where(r.random((N, C, V)) < 0.5, F32(0.0), F32(-0.0))
    elif cls == "inf":
        x[r.random((N, C, V)) < 0.3] = np.inf
        x[r.random((N, C, V)) < 0.3] = -np.inf
        x[:, :, 0] = -np.inf
    elif cls == "nan_first":
        x[:, 0] = np.nan
    elif cls == "nan_middle":
        x[:, C // 2] = np.nan
    elif cls == "nan_last":
        x[:, C - 1] = np.nan
    elif cls == "nan_two":
        x[:, C - 1] = np.nan
        x[:, max(C - 3, 0), ::2] = np.nan
    elif cls != "random":
        raise KeyError(cls)
    return x


# -------------------------------------------------------------------------------------------------------- case tables
LATTICE_N = tuple(range(1, 131)) + (255, 256, 257)
LATTICE_CHECKED_N = tuple(range(2, 300)) + (511, 512, 513, 1024, 1366, 2049)


def lattice_shapes():
    return [tuple(n if a == ax else 2 for a in range(3)) for ax in range(3) for n in LATTICE_N]


AFFINE_SHAPES = ((5, 9, 13), (6, 7, 8), (1, 1, 3), (1, 7, 8), (6, 1, 8), (6, 7, 1), (1, 1, 1))
AFFINE_BIG = (3, 1024, 1366)              # 4 196 352 voxels: just past 1024 blocks x 4096, the loop's second trip
AFFINE_MATRICES = ("identity", "generic", "scaled", "zero")


def affine_matrix(name, N=3):
    r = np.random.default_rng([len(name), 5])
    eye = np.tile(np.eye(3, 4, dtype=F32), (N, 1, 1))
    if name == "identity":
        return eye
    if name == "zero":
        return np.zeros((N, 3, 4), F32)
    M = (eye + 0.3 * r.standard_normal((N, 3, 4))).astype(F32)
    if name == "scaled":
        M = (M * np.where(r.random((N, 3, 4)) < 0.5, 1e3, 1e-3)).astype(F32)
    elif name != "generic":
        raise KeyError(name)
    return M


def affine_cotangent(kind, shape, N):
    """random: standard normal.  cancelling: +-1 alternating along the flattened volume plus 1e-4 noise -- the sums are ~1e-4 of
    sum|terms|, so the bound and not luck carries the comparison"""
    nvox = int(np.prod(shape))
    r = np.random.default_rng([nvox, N, len(kind)])
    g = r.standard_normal((N, nvox, 3), dtype=F32)
    if kind == "cancelling":
        g = (np.where(np.arange(nvox) % 2 == 0, F32(1), F32(-1))[None, :, None] + F32(1e-4) * g).astype(F32)
    return g.reshape((N,) + tuple(shape) + (3,))


# name: (shape, T, class, N)
TPS_GRID_CASES = {
    "w8":            ((3, 5, 8), 4, "random", 3),
    "w8_two_blocks": ((5, 9, 56), 130, "random", 1),
    "w4_tile2":      ((3, 5, 12), 513, "random", 1),
    "w4_lds_limit":  ((2, 3, 4), 2048, "random", 1),
    "w4_t512":       ((2, 3, 4), 512, "random", 1),
    "w4_wzero":      ((3, 5, 12), 5, "wzero", 3),
    "plain_nodes":   ((3, 5, 7), 5, "nodes", 3),
    "plain_vec_twin": ((4, 5, 9), 16, "twin", 1),
    "d1_unit":       ((1, 5, 8), 1, "unit", 1),
    "h1_outside":    ((3, 1, 7), 4, "outside", 1),
    "two_chunks":    ((5, 9, 190), 5, "random", 1),
    "rows_two_chunks": ((2, 17, 256), 130, "random", 1),
    "rows_two_stages": ((1, 3, 512), 4, "nodes", 3),
}
# name: (T, P, class, N)
TPS_POINTS_CASES = {
    "p1":      (4, 1, "random", 3),
    "p3":      (5, 3, "random", 1),
    "p4":      (16, 4, "random", 1),
    "p72_mixed": (40, 72, "mixed", 3),
    "p70":     (40, 70, "random", 1),
    "p1025":   (130, 1025, "random", 1),
    "p8193":   (16, 8193, "random", 1),
    "self64":  (64, 64, "self", 3),
    "self512": (512, 512, "self", 1),
    "tile2":   (513, 70, "random", 1),
    "wzero":   (5, 4, "wzero", 1),
    "t1_unit": (1, 3, "unit", 1),
}


def _keypoints(cls, T, N, r, shape=None):
    ctrl = r.uniform(-0.8, 0.8, (N, T, 3)).astype(F32)
    theta = (0.3 * r.standard_normal((N, T + 4, 3))).astype(F32)
    if cls in ("nodes", "unit") and shape is not None:
        D, H, W = shape
        corners = [(0, 0, 0), (D - 1, H - 1, W - 1), (0, H - 1, 0), (D - 1, 0, W - 1)]
        axes = [lattice(n) for n in shape]
        for n in range(N):
            for t in range(T):
                iz, iy, ix = corners[t] if t < 4 else (int(r.integers(0, D)), int(r.integers(0, H)), int(r.integers(0, W)))
                ctrl[n, t] = (axes[0][iz], axes[1][iy], axes[2][ix])
    if cls == "unit":
        theta[:] = 0
        theta[:, 0] = 1
    elif cls == "twin":
        ctrl[:, 1] = ctrl[:, 0]
    elif cls == "outside":
        ctrl = (np.where(r.random((N, T, 3)) < 0.5, F32(3), F32(-3))).astype(F32)
        ctrl[:, 1:] += (0.1 * r.standard_normal((N, T - 1, 3))).astype(F32)
    elif cls == "wzero":
        theta[:, :T] = 0
    return theta, ctrl


@functools.lru_cache(maxsize=None)
def tps_grid_case(name):
    """-> theta (N, T + 4, 3), ctrl (N, T, 3), cot (N, D, H, W, 3; xyz order), shape; float32, read-only"""
    shape, T, cls, N = TPS_GRID_CASES[name]
    r = np.random.default_rng([sum(map(ord, name)), T, N])
    theta, ctrl = _keypoints(cls, T, N, r, shape)
    cot = r.standard_normal((N,) + shape + (3,), dtype=F32)
    for a in (theta, ctrl, cot):
        a.setflags(write=False)
    return theta, ctrl, cot, shape


@functools.lru_cache(maxsize=None)
def tps_points_case(name):
    """-> theta, ctrl, pts (N, P, 3), cot (N, P, 3); float32, read-only.  self: pts == ctrl; mixed: every other point is a
    keypoint, the rest random in [-0.9, 0.9]"""
    T, P, cls, N = TPS_POINTS_CASES[name]
    r = np.random.default_rng([sum(map(ord, name)), T, P, N])
    theta, ctrl = _keypoints(cls, T, N, r)
    pts = r.uniform(-0.9, 0.9, (N, P, 3)).astype(F32)
    if cls == "self":
        pts = ctrl.copy()
    elif cls == "mixed":
        pts[:, ::2] = ctrl[:, np.arange(0, P, 2) % T]
    elif cls == "unit":
        pts[:, 0] = ctrl[:, 0]
    cot = r.standard_normal((N, P, 3), dtype=F32)
    for a in (theta, ctrl, pts, cot):
        a.setflags(write=False)
    return theta, ctrl, pts, cot


@functools.lru_cache(maxsize=None)
def tps_grid_truth(name, n):
    """sample n of a grid case in the points convention (cotangent and outputs in ij order): tps_truth's tuple"""
    theta, ctrl, cot, shape = tps_grid_case(name)
    return tps_truth(theta[n], ctrl[n], lattice_points(shape), cot[n].reshape(-1, 3)[:, ::-1], shape)


@functools.lru_cache(maxsize=None)
def tps_points_truth(name, n):
    theta, ctrl, pts, cot = tps_points_case(name)
    return tps_truth(theta[n], ctrl[n], pts[n], cot[n])
