"""fp64 numpy restatement of the closed-form stage (csrc/fits.hip: affine_fit, rigid_fit, affine_inverse, com3d;
csrc/grids.hip: affine_points) and the case table of its conformance tests.  Nothing here goes through torch's SVD
autograd: gradients of the restatement are central differences (vjp_fd), whose two step sizes bound their own error.

Every op takes ONE sample (fp32 arrays are promoted to fp64); the tests loop over a batch.

Classes of the fit cases (tests/test_fits_reference_cpu.py asserts that every case sits in its class):
  A  full rank: sigma_3 / sigma_1 >= 1e-3 of the rigid fit's H, and cond(S) <= 1e10 of the affine fit's normal matrix.
     The reference is a function of its inputs: equality against fp64.
  B  rank 2 with a unique proper optimum (sigma_2 / sigma_1 >= 1e-3, sigma_3 / sigma_1 <= 1e-12).  The reference's own
     output depends on LAPACK's sign of the null vector: properties only.
  C  rank <= 1 (sigma_2 / sigma_1 <= 1e-12): finite, orthogonal, T consistent.  Nothing else.

The bound of the fp64-inside kernels (fits, inverse), forwards and gradients alike:  |got - truth| <= 8 eps32 max|truth|
+ 8 floor.  The floor is measured here on the CPU from the restatement alone (ranges over the table):
  affine forward    normal equations in fp64 against lstsq (the truth): 2e-16 .. 5e-14 at offset 0 (cond(S) 4 .. 9e4),
                    2e-9 .. 2e-8 at offset 100 (cond(S) 3e9 .. 6e9), 6e-7 .. 8e-6 at offset 1000 (cond(S) 4e13 .. 6e13, past
                    class A's 1e10: listed by name in AFFINE_COND_LIMIT).
  affine backward   the analytic adjoint of the normal equations in fp64 against the same in long double (64-bit mantissa
                    where the platform has it), which is also the truth: fp64 autograd of the oracle equals it to 1e-12 on
                    the well-conditioned cases but is no yardstick at an offset, where its dw misses the long double
                    value by 1e-3 of 180 at offset 100 and by 85 of 1900 at offset 1000 (the fp64 adjoint: 1e-6 and 5e-2).
                    Relative to max|gradient|: <= 2e-11 at offset 0, <= 6e-8 at offset 100; at offset 1000 dx <= 4e-6,
                    dy <= 9e-9, dw <= 5e-5 -- there, and only there, the floor and not eps32 carries the bar.
  rigid, finite-difference gradients (the exactly symmetric clouds): |vjp_fd(h = 1e-6) - vjp_fd(h = 1e-5)|, 6e-10 .. 6e-9
                    for dx and dy (1e-9 .. 2e-8 of max|gradient|), up to 4e-7 for dw (7e-8 of its maximum).
  rigid, fp64 autograd of the oracle as the truth (everywhere else): 0; vjp_fd agrees with it to 1e-9.

Observed on gfx950 (MI355X): where eps32 carries the bar every error of M, dx, dy, dw is <= 0.52 eps32 max|truth| -- the one
rounding of the fp64 result; where the floor carries it (affine dx and dw at offset 1000) <= 0.46 of the bar; dw of clouds
that an affine map fits exactly (tetrahedron, exact symmetric clouds) is pure cancellation, truth ~0: 5e-12 against a bar
of 8e-12 (prism_exact-one_heavy) is the closest any case comes.
"""
import functools

import numpy as np

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def _d(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------ affine fit
def _design(x, w):
    x = _d(x)
    X = np.concatenate([x, np.ones((x.shape[0], 1))], 1)                  # (K, 4)
    wv = np.ones(x.shape[0]) if w is None else _d(w)
    return X, wv


def affine_fit(x, y, w=None):
    """the truth: least squares on the sqrt(w)-scaled homogeneous design matrix.  x, y (K, 3), w (K,) | None -> (3, 4)"""
    X, wv = _design(x, w)
    r = np.sqrt(wv)[:, None]
    sol = np.linalg.lstsq(X * r, _d(y) * r, rcond=None)[0]                # (4, 3)
    return sol.T


def affine_normal_matrix(x, w=None):
    X, wv = _design(x, w)
    return (X * wv[:, None]).T @ X


def affine_fit_normal(x, y, w=None):
    """the reference's route (keypoint_aligners.py:76-114): M = Y W X^T (X W X^T)^-1.  Its distance from affine_fit is the
    conditioning floor of any fp64 normal-equations solver."""
    X, wv = _design(x, w)
    XW = X * wv[:, None]
    return _d(y).T @ (XW @ np.linalg.inv(XW.T @ X))


def _inv_gj(a):
    """Gauss-Jordan inverse with partial pivoting in the dtype of `a` (np.linalg has no long double)"""
    n = a.shape[0]
    m = np.concatenate([a.copy(), np.eye(n, dtype=a.dtype)], 1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(m[c:, c])))
        if p != c:
            m[[c, p]] = m[[p, c]]
        m[c] = m[c] / m[c, c]
        for r in range(n):
            if r != c:
                m[r] = m[r] - m[r, c] * m[c]
    return m[:, n:]


def affine_fit_vjp(x, y, w, cot, dtype=np.float64, inv=_inv_gj):
    """analytic adjoint of the normal equations in `dtype`: (dx, dy, dw).  S = sum w X X^T, C = sum w y X^T, M = C S^-1;
    dC = G S^-1, dS = -M^T dC."""
    x, y, cot = (np.asarray(_d(a), dtype=dtype) for a in (x, y, cot))
    K = x.shape[0]
    X = np.concatenate([x, np.ones((K, 1), dtype=dtype)], 1)
    wv = np.ones(K, dtype=dtype) if w is None else np.asarray(_d(w), dtype=dtype)
    XW = X * wv[:, None]
    Si = inv(XW.T @ X)
    M = (y.T @ XW) @ Si
    dC = cot @ Si.T
    dS = -(M.T @ dC)
    dSs = dS + dS.T
    dX = wv[:, None] * (X @ dSs.T + y @ dC)                               # (K, 4)
    dy = wv[:, None] * (X @ dC.T)
    dw = 0.5 * np.einsum("ki,ij,kj->k", X, dSs, X) + np.einsum("kr,rj,kj->k", y, dC, X)
    return dX[:, :3], dy, dw


def affine_grad_floor(x, y, w, cot):
    """|fp64 adjoint - long double adjoint| per gradient (dx, dy, dw): the largest of three fp64 evaluations that round
    differently (Gauss-Jordan, LAPACK's inverse, the points summed in reverse order) -- one draw of rounding noise is a
    shaky estimate of its own scale where the truth is all cancellation (dw of a cloud that an affine map fits exactly)"""
    hi = affine_fit_vjp(x, y, w, cot, np.longdouble)
    rev = lambda a: None if a is None else np.asarray(a)[::-1]           # noqa: E731
    draws = [affine_fit_vjp(x, y, w, cot), affine_fit_vjp(x, y, w, cot, inv=np.linalg.inv),
             [g[::-1] for g in affine_fit_vjp(rev(x), rev(y), rev(w), cot)]]
    return [max(float(np.abs(d[i] - hi[i]).max()) for d in draws) for i in range(3)]


# ------------------------------------------------------------------------------------------------------------- rigid fit
def _rigid_moments(p1, p2, w):
    p1, p2, w = _d(p1), _d(p2), _d(w)
    if w is None:
        c1, c2 = p1.mean(0), p2.mean(0)
        q1, q2 = p1 - c1, p2 - c2
    else:
        c1, c2 = (p1 * w[:, None]).sum(0), (p2 * w[:, None]).sum(0)       # NOT divided by sum(w)
        q1, q2 = (p1 - c1) * w[:, None], (p2 - c2) * w[:, None]
    return c1, c2, q1, q2


def rigid_fit(p1, p2, w=None, full=False):
    """keypoint_aligners.py:151-213 through the polar factor: R0 = V U^T of H = q1^T q2, R = diag(1, 1, sign det R0) R0 (the
    last ROW scaled, as the reference scales V's), T = c2 - R c1.  (K, 3) -> (3, 4) [, singular values of H, det R0]"""
    c1, c2, q1, q2 = _rigid_moments(p1, p2, w)
    U, s, Vt = np.linalg.svd(q1.T @ q2)
    R = Vt.T @ U.T
    det0 = float(np.linalg.det(R))
    R[2] *= np.sign(det0)
    M = np.concatenate([R, (c2 - R @ c1)[:, None]], 1)
    return (M, s, det0) if full else M


def kabsch_proper(p1, p2, w=None):
    """the textbook proper rotation V diag(1, 1, det(V U^T)) U^T: the optimum over SO(3) (property cases only)"""
    c1, c2, q1, q2 = _rigid_moments(p1, p2, w)
    U, s, Vt = np.linalg.svd(q1.T @ q2)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    return np.concatenate([R, (c2 - R @ c1)[:, None]], 1)


def rigid_objective(R, p1, p2, w=None):
    """the reference's objective sum |q2 - R q1|^2 and its scale sum |q2|^2"""
    _, _, q1, q2 = _rigid_moments(p1, p2, w)
    return float(((q2 - q1 @ _d(R).T) ** 2).sum()), float((q2 ** 2).sum())


def rigid_centroids(p1, p2, w=None):
    return _rigid_moments(p1, p2, w)[:2]


# ------------------------------------------------------------------------------------------- inverse, points, centre of mass
def affine_inverse(M):
    """(3, 4) -> top three rows of inv([M; 0 0 0 1])"""
    A = np.concatenate([_d(M), [[0.0, 0.0, 0.0, 1.0]]], 0)
    return np.linalg.inv(A)[:3]


def affine_inverse_vjp(M, cot):
    """dA = -B^T G B^T with B = A^-1 and G = [cot; 0]: analytic, in fp64 (vjp_fd agrees, test_fits_reference_cpu)"""
    B = np.linalg.inv(np.concatenate([_d(M), [[0.0, 0.0, 0.0, 1.0]]], 0))
    G = np.concatenate([_d(cot), np.zeros((1, 4))], 0)
    return (-(B.T @ G @ B.T))[:3]


def affine_points(M, pts):
    """(3, 4), (P, 3) -> (P, 3)"""
    M, pts = _d(M), _d(pts)
    return pts @ M[:, :3].T + M[:, 3]


def affine_points_vjp(M, pts, cot):
    M, pts, cot = _d(M), _d(pts), _d(cot)
    dM = np.concatenate([cot.T @ pts, cot.sum(0)[:, None]], 1)
    return dM, cot @ M[:, :3]


def _lin(size, ax, linspace):
    return np.asarray(linspace(size), dtype=np.float64).reshape([-1 if a == ax else 1 for a in range(3)])


def _linspace64(size):
    return np.linspace(0.0, 1.0, size)


def center_of_mass(feat, linspace=_linspace64):
    """keymorph/layers.py:78-134 with its F.relu (:97) and linspace(0, 1, size): (N, K, D, H, W) -> (N, K, 3), (z, y, x).
    The truth takes the coordinates i / (size - 1) in fp64; `linspace` swaps in the fp32 ones the oracle builds (4e-8 apart)."""
    v = np.maximum(_d(feat), 0.0)
    tot = v.sum((2, 3, 4)) + 1e-8
    out = [(v * _lin(v.shape[2 + ax], ax, linspace)).sum((2, 3, 4)) / tot for ax in range(3)]
    return np.stack(out, -1) * 2.0 - 1.0


def center_of_mass_vjp(feat, cot, linspace=_linspace64):
    """analytic: d pts_a / d v = 2 (lin_a - m_a) / tot on v > 0, exactly 0 on v <= 0 (relu)"""
    f = _d(feat)
    v = np.maximum(f, 0.0)
    tot = (v.sum((2, 3, 4)) + 1e-8)[:, :, None, None, None]
    g = np.zeros_like(v)
    for ax in range(3):
        lin = _lin(v.shape[2 + ax], ax, linspace)
        m = (v * lin).sum((2, 3, 4), keepdims=True) / tot
        g += _d(cot)[:, :, ax, None, None, None] * 2.0 * (lin - m) / tot
    return np.where(f > 0, g, 0.0)


# ------------------------------------------------------------------------------------------------------ finite differences
def _fd(f, args, cot, h):
    args = [None if a is None else _d(a).copy() for a in args]
    grads = []
    for i, a in enumerate(args):
        if a is None:
            grads.append(None)
            continue
        g = np.zeros_like(a)
        flat, gf = a.reshape(-1), g.reshape(-1)
        for j in range(flat.size):
            keep = flat[j]
            flat[j] = keep + h
            up = f(*args)
            flat[j] = keep - h
            dn = f(*args)
            flat[j] = keep
            gf[j] = ((up - dn) * cot).sum() / (2.0 * h)
        grads.append(g)
    return grads


def vjp_fd(f, args, cot, h=(1e-6, 1e-5)):
    """central differences of sum(f(*args) * cot) for every argument that is not None, at both step sizes.
    Returns (gradients at h[0], per-gradient uncertainty = max |difference between the two step sizes|)."""
    a, b = _fd(f, args, _d(cot), h[0]), _fd(f, args, _d(cot), h[1])
    unc = [None if x is None else float(np.abs(x - y).max()) for x, y in zip(a, b)]
    return a, unc


# -------------------------------------------------------------------------------------------------------------- case table
def _rot(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


ROT90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])            # exact in fp32: the symmetry survives


def _generic(rng, K, offset=0.0):
    """the generic well-conditioned pair of test_matrix_fit_fwd_bwd: x in [-0.8, 0.8]^3 (+ offset), y = A x + 0.1 + noise"""
    x = rng.random((K, 3)) * 1.6 - 0.8
    A = np.eye(3) + 0.2 * rng.standard_normal((3, 3))
    y = x @ A.T + 0.1 + 0.05 * rng.standard_normal((K, 3))
    return x + offset, y + offset


def _tetrahedron(rng):
    x = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.5]]) - 0.125
    A = np.eye(3) + 0.2 * rng.standard_normal((3, 3))
    return x, x @ A.T + 0.1


def _reflection(rng, K):
    x = rng.random((K, 3)) * 1.6 - 0.8
    Q = _rot(rng) @ np.diag([1.0, 1.0, -1.0])
    return x, x @ Q.T + 0.02 * rng.standard_normal((K, 3))


def _near_coplanar(rng, K):
    x = rng.random((K, 3)) * 1.6 - 0.8
    x[:, 2] *= 0.05                                                       # sigma_3 / sigma_1 ~ 2e-3 (it goes with the square)
    y = x @ _rot(rng).T + 0.1
    y += 1e-3 * rng.standard_normal((K, 3)) * [1, 1, 0.05]
    return x, y


def _cube(reps=1):
    v = np.array([[a, b, c] for a in (-0.5, 0.5) for b in (-0.5, 0.5) for c in (-0.5, 0.5)])
    return np.tile(v, (reps, 1))


def _prism(reps=1):
    return _cube(reps) * [1.0, 1.0, 0.4]                                  # z = +-0.2: sigma = (2, 2, 0.32) unweighted


def _lattice(n):
    a = (np.arange(n) - (n - 1) / 2.0) * 0.25                             # exact in fp32, like the cube's +-0.5
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)


def _symmetric(base, rng, jitter):
    """a symmetric cloud and its exact quarter turn (+ a translation that is exact in fp32); jitter breaks the symmetry"""
    x = base.copy()
    y = x @ ROT90.T + [0.25, -0.125, 0.5]
    if jitter:
        x = x + jitter * rng.standard_normal(x.shape)
        y = y + jitter * rng.standard_normal(y.shape)
    return x, y


WEIGHTS = ("none", "normalised", "sum0.5", "sum3", "quarter_zero", "one_heavy")


def make_weights(kind, K, rng, uniform=False):
    """none | normalised | summing to 0.5 | to 3 | a quarter exactly zero | one weight 0.97, the rest sharing 0.03.
    uniform: equal weights (they keep a symmetric cloud symmetric) where the kind leaves the values free."""
    if kind == "none":
        return None
    w = np.ones(K) if uniform else rng.random(K) + 0.1
    if kind == "quarter_zero":
        w[rng.permutation(K)[:K // 4]] = 0.0
    if kind == "one_heavy":
        j = int(rng.integers(K))
        w[j] = 0.0
        w = w / w.sum() * 0.03
        w[j] = 0.97
        return w
    return w / w.sum() * {"sum0.5": 0.5, "sum3": 3.0}.get(kind, 1.0)


def _case(name, cls, x, y, w, grad="autograd", kinds=("affine", "rigid"), note=""):
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=F32)          # noqa: E731
    return {"name": name, "cls": cls, "x": f(x), "y": f(y), "w": f(w), "grad": grad, "kinds": kinds, "note": note}


# Which weighting a cloud gets for which fit -- the rules that keep a case in class A (measured figures in brackets):
#   quarter_zero needs K >= 8, to leave an affine fit well more than four points;
#   one_heavy squares into H (q = (p - c) w) and leaves it nearly rank 1: sigma_3 / sigma_1 >= 2e-3 up to K = 65 [7e-4 at 256];
#   weights that do not sum to 1 put the centroid sum(w p) of an offset cloud far off the cloud, and H is rank 1 again
#   [sigma_3 / sigma_1 1e-6 at offset 100, sum 3], so the rigid fit of offset clouds takes weights of sum 1 only; the same
#   moves the near-coplanar cloud under 1e-3 [1.3e-4];
#   one_heavy at an offset takes the affine cond(S) past 1e10 [2.3e10 at offset 100].
def _kinds(tag, K, wk):
    kinds = ["affine", "rigid"]
    if (wk == "quarter_zero" and K < 8) or (wk == "one_heavy" and K < 5):
        return ()
    offset, flat = "offset" in tag, "near_coplanar" in tag
    if wk == "one_heavy" and (K > 65 or flat):
        kinds.remove("rigid")
    if wk in ("sum0.5", "sum3") and (offset or flat):
        kinds.remove("rigid")
    if wk == "one_heavy" and offset:
        kinds.remove("affine")
    return tuple(kinds)


# cond(S) of the affine normal matrix at offset 1000 is 3e13 .. 6e13: past class A's 1e10, and kept because real-world
# millimetre coordinates look like this; its floor (normal equations against lstsq, 1e-6 .. 4e-6) carries the bound.
AFFINE_COND_LIMIT = {"offset1000": 1e14}


def affine_cond_limit(name):
    return next((v for k, v in AFFINE_COND_LIMIT.items() if k in name), 1e10)


@functools.lru_cache(maxsize=None)
def fit_cases():
    """the class-A table: one sample per case.  grad = "fd" marks the exactly symmetric clouds (equal singular values), where
    fp64 autograd through torch.linalg.svd is not finite and vjp_fd is the truth."""
    rng = np.random.default_rng(20250)
    out = []

    def add(tag, K, make, fd=False):
        for wk in WEIGHTS:
            kinds = _kinds(tag, K, wk)
            if not kinds:
                continue
            x, y = make()
            # an exactly symmetric cloud stays symmetric under equal weights only
            uniform = fd and wk in ("normalised", "sum0.5", "sum3")
            w = make_weights(wk, K, rng, uniform)
            g = "fd" if fd and (wk == "none" or uniform) else "autograd"
            out.append(_case(f"{tag}-{wk}", "A", x, y, w, g, kinds))

    out.append(_case("K4_tetrahedron-none", "A", *_tetrahedron(rng), None, note="affine interpolates"))
    out.append(_case("K4_tetrahedron-sum3", "A", *_tetrahedron(rng), make_weights("sum3", 4, rng)))
    for K in (5, 63, 64, 65, 255, 256, 257, 512, 1000):
        add(f"K{K}_generic", K, lambda K=K: _generic(rng, K))
    add("K50_reflection", 50, lambda: _reflection(rng, 50))
    add("K300_reflection", 300, lambda: _reflection(rng, 300))
    add("K50_near_coplanar", 50, lambda: _near_coplanar(rng, 50))
    for tag, base in (("cube", _cube()), ("prism", _prism()), ("lattice3", _lattice(3))):
        add(f"{tag}_exact", len(base), lambda b=base: _symmetric(b, rng, 0.0), fd=True)
        add(f"{tag}_jitter", len(base), lambda b=base: _symmetric(b, rng, 1e-3))
    add("K50_offset100", 50, lambda: _generic(rng, 50, 100.0))
    add("K300_offset100", 300, lambda: _generic(rng, 300, 100.0))
    add("K50_offset1000", 50, lambda: _generic(rng, 50, 1000.0))
    return out


@functools.lru_cache(maxsize=None)
def batch_case():
    """N = 37 samples at K = 64 that mix every class-A cloud (the symmetric ones as 8 copies of the cube / prism and the
    4 x 4 x 4 lattice), all weighted (one launch takes one weight tensor) with a weighting that keeps the sample in class A
    for both fits: (x, y, w, per-sample gradient mode, names)"""
    rng = np.random.default_rng(37)
    K = 64
    makers = [
        ("generic", lambda: _generic(rng, K), False), ("reflection", lambda: _reflection(rng, K), False),
        ("near_coplanar", lambda: _near_coplanar(rng, K), False),
        ("cube_exact", lambda: _symmetric(_cube(8), rng, 0.0), True),
        ("cube_jitter", lambda: _symmetric(_cube(8), rng, 1e-3), False),
        ("prism_exact", lambda: _symmetric(_prism(8), rng, 0.0), True),
        ("prism_jitter", lambda: _symmetric(_prism(8), rng, 1e-3), False),
        ("lattice4_exact", lambda: _symmetric(_lattice(4), rng, 0.0), True),
        ("lattice4_jitter", lambda: _symmetric(_lattice(4), rng, 1e-3), False),
        ("offset100", lambda: _generic(rng, K, 100.0), False), ("offset1000", lambda: _generic(rng, K, 1000.0), False),
    ]
    xs, ys, ws, modes, names = [], [], [], [], []
    for n in range(37):
        tag, make, sym = makers[n % len(makers)]
        allowed = [wk for wk in WEIGHTS[1:] if len(_kinds(tag, K, wk)) == 2]
        wk = allowed[(n // len(makers) + n) % len(allowed)]
        uniform = sym and wk in ("normalised", "sum0.5", "sum3")
        x, y = make()
        xs.append(x), ys.append(y), ws.append(make_weights(wk, K, rng, uniform))
        modes.append("fd" if uniform else "autograd")
        names.append(f"{tag}-{wk}")
    f = lambda a: np.ascontiguousarray(np.stack(a), dtype=F32)          # noqa: E731
    return f(xs), f(ys), f(ws), modes, names


@functools.lru_cache(maxsize=None)
def property_cases():
    """classes B and C (rigid only)"""
    rng = np.random.default_rng(77)
    out = []
    # B: both clouds exactly in z = 0, rotated in the plane
    x = rng.random((40, 3)) * 1.6 - 0.8
    x[:, 2] = 0.0
    c, s = np.cos(0.7), np.sin(0.7)
    y = x @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + [0.1, -0.2, 0.0]
    y[:, :2] += 0.01 * rng.standard_normal((40, 2))
    for wk in ("none", "normalised", "sum3"):
        out.append(_case(f"planar_z0-{wk}", "B", x, y, make_weights(wk, 40, rng), kinds=("rigid",)))
    x, y = _generic(rng, 3)
    for wk in ("none", "normalised"):
        out.append(_case(f"K3_generic-{wk}", "B", x, y, make_weights(wk, 3, rng), kinds=("rigid",)))
    # C
    x, y = _generic(rng, 2)
    out.append(_case("K2-none", "C", x, y, None, kinds=("rigid",)))
    out.append(_case("K2-normalised", "C", x, y, make_weights("normalised", 2, rng), kinds=("rigid",)))
    x, y = _generic(rng, 1)
    out.append(_case("K1-none", "C", x, y, None, kinds=("rigid",)))
    out.append(_case("K1-weight1", "C", x, y, np.ones(1), kinds=("rigid",)))
    t = np.linspace(-1, 1, 20)[:, None]
    x = t * [0.5, 0.25, -0.125] + [0.125, 0.0, 0.25]                      # exact in fp32: exactly collinear
    y = t * [0.25, -0.5, 0.125] - 0.125
    out.append(_case("collinear-none", "C", x, y, None, kinds=("rigid",)))
    out.append(_case("collinear-normalised", "C", x, y, make_weights("normalised", 20, rng), kinds=("rigid",)))
    x, y = _generic(rng, 30)
    w = np.zeros(30)
    w[7] = 1.0
    out.append(_case("all_weight_on_one_point", "C", x, y, w, kinds=("rigid",)))
    return out


def cotangent(seed, shape=(3, 4)):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


def bound(truth, floor=0.0):
    """the shared rule of the fp64-inside kernels"""
    return 8.0 * EPS32 * float(np.abs(truth).max()) + 8.0 * floor


def oracle_vjp(kind, x, y, w, cot):
    """fp64 autograd of oracle/keymorph_oracle.py's fit of one sample: (M, [dx, dy, dw | None])"""
    import torch
    from oracle import keymorph_oracle as O
    t = lambda a: None if a is None else torch.tensor(_d(a)[None], dtype=torch.float64, requires_grad=True)      # noqa: E731
    xt, yt, wt = t(x), t(y), t(w)
    M = (O.affine_fit if kind == "affine" else O.rigid_fit)(xt, yt, wt)
    (M * torch.tensor(_d(cot))).sum().backward()
    return M[0].detach().numpy(), [None if a is None else a.grad[0].numpy() for a in (xt, yt, wt)]


def fit_truth(kind, x, y, w, cot, mode="autograd"):
    """(M, floor of M, [dx, dy, dw | None], their floors) of one sample, as the module docstring states them"""
    if kind == "affine":
        M = affine_fit(x, y, w)
        floor = float(np.abs(affine_fit_normal(x, y, w) - M).max())
        grads = [np.asarray(g, dtype=np.float64) for g in affine_fit_vjp(x, y, w, cot, np.longdouble)]
        gfl = affine_grad_floor(x, y, w, cot)
        if w is None:
            grads[2] = None
        return M, floor, grads, [None if g is None else f for g, f in zip(grads, gfl)]
    M = rigid_fit(x, y, w)
    if mode == "fd":
        grads, unc = vjp_fd(rigid_fit, (x, y, w), cot)
        return M, 0.0, grads, unc
    grads = oracle_vjp(kind, x, y, w, cot)[1]
    return M, 0.0, grads, [None if g is None else 0.0 for g in grads]


# ----------------------------------------------------------------------------------------------- inverse / points / com cases
@functools.lru_cache(maxsize=None)
def inverse_cases():
    """(name, M (N, 3, 4) float32) for N in {1, 64, 65}"""
    rng = np.random.default_rng(5)
    out = []
    for N in (1, 64, 65):
        out.append((f"near_identity_N{N}", np.eye(3, 4) + 0.2 * rng.standard_normal((N, 3, 4))))
        S = np.zeros((N, 3, 4))
        for n in range(N):
            sc = 10.0 ** rng.uniform(-3, 3, 3)
            sh = np.eye(3) + np.triu(0.5 * rng.standard_normal((3, 3)), 1)
            S[n, :, :3] = _rot(rng) @ np.diag(sc) @ sh
            S[n, :, 3] = rng.uniform(-500, 500, 3)
        out.append((f"scales_shear_translation_N{N}", S))
        Rf = np.zeros((N, 3, 4))
        for n in range(N):
            Rf[n, :, :3] = _rot(rng) @ np.diag([1.0, 1.0, -1.0]) * rng.uniform(0.5, 2.0)
            Rf[n, :, 3] = rng.uniform(-1, 1, 3)
        out.append((f"reflection_N{N}", Rf))
    return [(n, np.ascontiguousarray(m, dtype=F32)) for n, m in out]


@functools.lru_cache(maxsize=None)
def points_cases():
    """(name, M (N, 3, 4), pts (N, P, 3)) for P in {1, 63, 256, 257, 5000} x N in {1, 3}"""
    rng = np.random.default_rng(6)
    out = []
    for P in (1, 63, 256, 257, 5000):
        for N in (1, 3):
            M = np.eye(3, 4) + 0.3 * rng.standard_normal((N, 3, 4))
            pts = rng.random((N, P, 3)) * 2 - 1
            out.append((f"P{P}_N{N}", np.ascontiguousarray(M, dtype=F32), np.ascontiguousarray(pts, dtype=F32)))
    return out


COM_SHAPES = ((1, 1, 1, 1, 1), (1, 2, 1, 1, 70), (2, 3, 5, 1, 7), (1, 2, 9, 10, 11), (2, 3, 40, 33, 47))
COM_CONTENTS = ("relu", "negatives", "dead_channel", "hot_voxel", "pedestal")


def com_volume(shape, content, seed=0):
    """relu: a ReLU'd map, ~70 % exact zeros | negatives: a normal map | dead_channel: as negatives with channel (0, 0) all
    <= 0 (zeros and negatives) | hot_voxel: one positive voxel per channel, the rest exact zeros | pedestal: 1 + 0.01 U
    with one +50 peak"""
    rng = np.random.default_rng(1000 + seed)
    V = int(np.prod(shape[2:]))
    if content == "relu":
        f = np.maximum(rng.standard_normal(shape) - 0.52, 0.0)
        if V == 1:
            f[...] = 0.75
    elif content in ("negatives", "dead_channel"):
        f = rng.standard_normal(shape)
        if V == 1:
            f[...] = 0.75
        if content == "dead_channel":
            f[0, 0] = -np.abs(f[0, 0]) * (rng.random(shape[2:]) < 0.5)
    elif content == "hot_voxel":
        f = np.zeros(shape)
        flat = f.reshape(shape[0], shape[1], V)
        for n in range(shape[0]):
            for k in range(shape[1]):
                flat[n, k, rng.integers(V)] = 3.0
    else:
        f = 1.0 + 0.01 * rng.random(shape)
        flat = f.reshape(shape[0], shape[1], V)
        for n in range(shape[0]):
            for k in range(shape[1]):
                flat[n, k, rng.integers(V)] += 50.0
    return np.ascontiguousarray(f, dtype=F32)
