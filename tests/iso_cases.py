"""Inputs and references for isotropic total variation: loss.IsoTVRegularizer, the two launches of
include/sphrt_iso.h (csrc/loss.hip: sphrt_iso_primal_f64, sphrt_iso_dual_f64) and the iso branch
of `retrieval.primal_dual` and `retrieval.chambolle_pock` — no tests here, no GPU dependency and no
library call.  The edge rules are pd_cases.neighbours', the rational fma cg_cases', the clamp
fista_cases', the fidelity terms and their conjugates cp_cases'.

  value    `iso_value`: the penalty written as loops over voxels.
  kernels  `primal_ref` / `dual_ref`: one element of either launch in the header's order, Python
           floats (IEEE double operations, math.sqrt correctly rounded) and the rational fma;
           `exact_dual_case`: Pythagorean triples scaled by powers of two, every intermediate exact.
  solver   `iso_dense`: the iteration on a dense system (D the weighted difference matrix, rows
           grouped by voxel); `certify`: as pd_cases.certify, for any ball-feasible q
           min over the box of 1/2 x^T N x - (b - D^T q)^T x is a lower bound of the minimum."""
import math
from fractions import Fraction

import numpy as np

import cg_cases as cc
import cp_cases as cp
import fista_cases as fc
import pd_cases as pc

U = 2.0 ** -53
BALL = Fraction(1) + 12 * Fraction(1, 2 ** 53)      # sum q^2 <= radius^2 (1 + 12 u): sphrt_iso.h
LAM_TV = pc.LAM_TV
TV_WEIGHTS = pc.TV_WEIGHTS
WEIGHTS = [(1.0, 0.5, 2.0), (0.0, 0.5, 2.0), (1.0, 0.0, 2.0), (1.0, 0.5, 0.0)]   # each off in turn


def kernel_cases():
    """[(shape, wrap, weights)]: pd_cases.SHAPES, ring open and closed, each weight 0 in turn."""
    return [(shape, w, wt) for shape, wraps in pc.SHAPES for w in wraps for wt in WEIGHTS]


def has_of(weights, shape):
    return [w > 0 and n > 1 for w, n in zip(weights, shape)]


# ---- the penalty -------------------------------------------------------------------------------------
def iso_value(d, weights, wrap):
    """P(d) by loops: every leading axis a batch axis; an edge belongs to its lower voxel, the
    wrap edge to the ring's last voxel, a missing edge adds 0."""
    d = np.asarray(d, dtype=np.float64)
    nr, ne, na = d.shape[-3:]
    vol = d.reshape((-1, nr, ne, na))
    total = 0.0
    for b in range(vol.shape[0]):
        for r in range(nr):
            for e in range(ne):
                for a in range(na):
                    s, here = 0.0, vol[b, r, e, a]
                    if weights[0] > 0 and r + 1 < nr:
                        s += (weights[0] * (vol[b, r + 1, e, a] - here)) ** 2
                    if weights[1] > 0 and e + 1 < ne:
                        s += (weights[1] * (vol[b, r, e + 1, a] - here)) ** 2
                    if weights[2] > 0 and na > 1 and (a + 1 < na or wrap):
                        s += (weights[2] * (vol[b, r, e, (a + 1) % na] - here)) ** 2
                    total += math.sqrt(s)
    return total / d.size


# ---- the launches, one element -----------------------------------------------------------------------
def primal_ref(i, x, g, q, lo, up, weights, c_damp, tau, lower, upper):
    """One element of sphrt_iso_primal_f64 -> (x_new, its term of MM)."""
    xi = float(x[i])
    gp = cc.fma(c_damp, xi, float(g[i]))
    s = 0.0
    for ax in range(3):
        if lo[ax, i] >= 0:
            s = cc.fma(weights[ax], float(q[ax][lo[ax, i]]), s)
        if up[ax, i] >= 0:
            s = cc.fma(-weights[ax], float(q[ax][i]), s)
    xn = fc.clamp_ref(cc.fma(-tau, gp + s, xi), lower, upper)
    d = xn - xi
    return xn, d * d


def _sqrt(v):
    return math.sqrt(v) if v >= 0 else math.nan      # (v is NaN or >= 0: a sum of squares)


def dual_ref(i, x_new, x_old, q, up, weights, radius, sigma):
    """One voxel of sphrt_iso_dual_f64 -> ([q_r, q_e, q_a] at slot i (None: no edge, untouched),
    its term of QQ)."""
    def xb(j):
        return cc.fma(2.0, float(x_new[j]), -float(x_old[j]))
    v, n2 = [None, None, None], 0.0
    for ax in range(3):
        j = up[ax, i]
        if j < 0:
            continue
        e = weights[ax] * (xb(j) - xb(i))
        v[ax] = cc.fma(sigma, e, float(q[ax][i]))
        n2 = n2 + _mul(v[ax], v[ax])
    nrm = _sqrt(n2) if not math.isnan(n2) else math.nan
    out, t = [None, None, None], 0.0
    scale = _div(radius, nrm) if nrm > radius else None
    for ax in range(3):
        if v[ax] is None:
            continue
        out[ax] = v[ax] if scale is None else _mul(v[ax], scale)
        d = out[ax] - float(q[ax][i])
        t = t + _mul(d, d)
    return out, t


def _mul(a, b):
    """a * b in IEEE double (Python raises on nothing here, but inf * 0 must be NaN)."""
    with np.errstate(all='ignore'):
        return float(np.float64(a) * np.float64(b))


def _div(a, b):
    with np.errstate(all='ignore'):
        return float(np.float64(a) / np.float64(b))


# ---- the dual launch on exact data -------------------------------------------------------------------
QUADS = [(1, 2, 2, 3), (2, 3, 6, 7), (3, 4, 12, 13), (4, 4, 7, 9)]
PAIRS = [(3, 4, 5), (5, 12, 13)]


def exact_dual_case(shape, wrap, weights, seed):
    """Inputs on which every operation of sphrt_iso_dual_f64 is exact -> (x_new, x_old = 0, q,
    sigma, radius, want (3, n) as float64 from Fractions, side (n): -1 inside, 0 the tie, +1
    outside).  x_new = x_old = 0, so e = 0 and v = q exactly: the voxel's present axes hold the
    legs of a Pythagorean quadruple (three axes present), of a triple (two) or one number (one),
    in random order and with random signs, times 2^-j with j in {-1, 0, 1} drawn per voxel.  A
    launch has one radius R for all voxels: R = (the quadruple's norm) * (the triple's norm), the
    quadruple's legs are multiplied by the triple's norm and the other way round, so every
    voxel's norm is R 2^-j — the radius is the norm times 2^j.  n2, nrm and scale = 2^j are then
    exact, and the stored q is v 2^j (outside, j = -1) or v (inside, and the tie j = 0), to the
    bit.  `seed` picks the quadruple and the triple."""
    n = math.prod(shape)
    has = has_of(weights, shape)
    _, up = pc.neighbours(shape, wrap, has)
    rng = np.random.default_rng(seed)
    quad, pair = QUADS[seed % len(QUADS)], PAIRS[seed % len(PAIRS)]
    R = quad[3] * pair[2]
    q = np.zeros((3, n))
    side = np.zeros(n, dtype=np.int64)
    want = np.zeros((3, n))
    present = up >= 0
    count = present.sum(axis=0)
    for i in range(n):
        axes = np.flatnonzero(present[:, i])
        if len(axes) == 0:
            continue
        j = int(rng.integers(-1, 2))                    # radius = |v| 2^j... |v| = R 2^-j
        legs = {3: [c * pair[2] for c in quad[:3]], 2: [c * quad[3] for c in pair[:2]],
                1: [R]}[len(axes)]
        legs = [legs[k] for k in rng.permutation(len(legs))]
        for ax, leg in zip(axes, legs):
            q[ax, i] = float(rng.choice([-1.0, 1.0])) * leg * 2.0 ** -j
        side[i] = -1 if j > 0 else (0 if j == 0 else 1)
        # Fractions: |v| = R 2^-j against the radius R
        vf = [Fraction(q[ax, i]) for ax in axes]
        nf2 = sum(f * f for f in vf)
        assert nf2 == (Fraction(R) / Fraction(2) ** j) ** 2
        for ax, f in zip(axes, vf):
            want[ax, i] = float(f * Fraction(2) ** j) if j < 0 else float(f)
    assert count.max() == sum(has)
    return np.zeros(n), np.zeros(n), q, 0.5, float(R), want, side


def ball_excess(q, up, radius):
    """max over voxels of sum_ax q_ax^2 / radius^2 as a Fraction (present axes only; 0 if none)."""
    worst, r2 = Fraction(0), Fraction(radius) ** 2
    for i in range(q.shape[1]):
        s = sum((Fraction(float(q[ax, i])) ** 2 for ax in range(3) if up[ax, i] >= 0), Fraction(0))
        worst = max(worst, s / r2)
    return worst


# ---- the solver against dense algebra ------------------------------------------------------------------
def iso_matrix(shape, wrap, weights):
    """(Dw, voxel of every row, B): the dense weighted forward-difference matrix, rows ordered by
    axis, then by the edge's dual slot (its lower voxel), and B = 4 sum of w_ax^2 over the axes
    with edges."""
    D, axis, _ = pc.tv_matrix(shape, wrap, weights)
    has = has_of(weights, shape)
    _, up = pc.neighbours(shape, wrap, has)
    voxel = np.concatenate([np.flatnonzero(up[ax] >= 0) for ax in range(3)]).astype(np.int64)
    w = np.asarray(weights, dtype=np.float64)
    Dw = D * w[axis][:, None] if len(D) else D.reshape(0, math.prod(shape))
    return Dw, voxel, 4.0 * sum(wt * wt for wt, h in zip(weights, has) if h)


def norms(v, voxel, n):
    """The 2-norm of every voxel's rows of v -> (n,)."""
    n2 = np.zeros(n)
    np.add.at(n2, voxel, v * v)
    return np.sqrt(n2)


def project(v, voxel, n, radius):
    nrm = norms(v, voxel, n)
    scale = np.where(nrm > radius, radius / np.where(nrm > radius, nrm, 1.0), 1.0)
    return v * scale[voxel]


def iso_dense(N, b, D, voxel, radius, lower, upper, L, ratio, K, B, x0=None, q0=None, keep=True):
    """The iso branch of `retrieval.primal_dual` restated on the dense system, as
    pd_cases.pd_dense is for the abs term -> (x_0 .. x_K or the last, q_K, MM, QQ)."""
    tau, sigma = pc.pd_steps(L, ratio, B)
    n = len(b)
    x = np.clip(np.zeros_like(b) if x0 is None else np.asarray(x0, dtype=np.float64), lower, upper)
    q = np.zeros(len(D)) if q0 is None else np.asarray(q0, dtype=np.float64)
    xs, mm, qq = [x], [], []
    for _ in range(K):
        u = x - tau * ((N @ x - b) + D.T @ q)
        x_new = np.where(u < lower, lower, np.where(u > upper, upper, u))
        q_new = project(q + sigma * (D @ (2 * x_new - x)), voxel, n, radius)
        mm.append(float(((x_new - x) ** 2).sum()))
        qq.append(float(((q_new - q) ** 2).sum()))
        x, q = x_new, q_new
        if keep:
            xs.append(x)
    return (xs if keep else x), q, mm, qq


def primal_value(N, b, D, voxel, radius, x):
    ld = np.longdouble
    N, b, D, x = (np.asarray(v, dtype=ld) for v in (N, b, D, x))
    v = D @ x
    n2 = np.zeros(len(x), dtype=ld)
    np.add.at(n2, voxel, v * v)
    return 0.5 * x @ (N @ x) - b @ x + ld(radius) * np.sqrt(n2).sum()


def radius_of(N, b, D, voxel, radius, x, q, lower, upper):
    """pd_cases.radius_of for the ball: q is scaled by 1 / (1 + 12 u) first, after which every
    voxel's triple must lie in the ball (checked in extended precision, whose own rounding the
    scaling's slack of 12 u - 9 u covers)."""
    x = np.asarray(x, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64) / (1.0 + 12 * U)
    assert np.all((x >= lower) & (x <= upper))
    n2 = np.zeros(len(x), dtype=np.longdouble)
    np.add.at(n2, voxel, q.astype(np.longdouble) ** 2)
    assert np.all(n2 <= np.longdouble(radius) ** 2), float((n2 / np.longdouble(radius) ** 2).max())
    lam_min = float(np.linalg.eigvalsh(N)[0])
    assert lam_min > 0
    rhs = b - D.T @ q
    try:
        z = fc.bounded_minimiser(N, rhs, lower, upper, max_iterations=20000)
    except AssertionError:
        z, step = x, 1.0 / float(np.linalg.eigvalsh(N)[-1])
        for _ in range(2000):
            z = np.clip(z - step * (N @ z - rhs), lower, upper)
    gap = float(primal_value(N, b, D, voxel, radius, x)
                - pc.dual_lower_bound(N, rhs, z, lower, upper, lam_min))
    size = float(0.5 * np.abs(x) @ (np.abs(N) @ np.abs(x)) + (np.abs(b) + np.abs(rhs)) @ np.abs(x)
                 + radius * norms(D @ x, voxel, len(x)).sum())
    err = 2.0 * len(x) * float(np.finfo(np.longdouble).eps) * size
    assert gap >= -err, (gap, err)
    return math.sqrt(2.0 * (max(gap, 0.0) + err) / lam_min)


def certify(N, b, D, voxel, radius, lower, upper, L, B, ratio=pc.DUAL_RATIO, chunk=2000,
            max_chunks=50):
    """-> (x*, q*, the certificate's radius): `iso_dense` until x stalls (no change over a chunk
    beyond 1e-15 relative) and q with it to 1e-12 of the ball's radius — a projected triple
    carries rounding noise of a few ulp where a clamped one holds the bound's own bits, and where
    a voxel's differences vanish its q is not unique — or for max_chunks chunks, then
    `radius_of`: the certificate holds for whatever (x, q) it is given, and its radius says how
    good they are."""
    x, q = None, None
    for _ in range(max_chunks):
        x_new, q_new, _, _ = iso_dense(N, b, D, voxel, radius, lower, upper, L, ratio, chunk, B,
                                       x0=x, q0=q, keep=False)
        still = x is not None and np.abs(x_new - x).max() <= 1e-15 * np.abs(x_new).max() \
            and np.abs(q_new - q).max() <= 1e-12 * radius
        x, q = x_new, q_new
        if still:
            break
    return x, q, radius_of(N, b, D, voxel, radius, x, q, lower, upper)


def ball_shares(q, voxel, n, radius):
    """(share of voxels flat at the minimiser: |q_i| < r (1 - 1e-9); share that carry a jump)."""
    nrm = norms(q, voxel, n)
    flat = nrm < radius * (1 - 1e-9)
    return float(flat.mean()), float((~flat).mean())


def flat_dual(q, up):
    return cp.flat_dual(q, up)


def tv_term(wrap):
    from sph_raytracer_amd.loss import IsoTVRegularizer
    return LAM_TV * IsoTVRegularizer(weights=TV_WEIGHTS, wrap_a=wrap)


# ---- chambolle_pock's duality gap with the iso term ----------------------------------------------------
def cp_gap(case, x, info):
    """cp_cases.gap_of for the iso term (ring closed, as cp_cases.tv_edges): J with r sum |Dw x|_i,
    D(p, q) with q scaled into the ball by 1 / (1 + 12 u)."""
    name, kind, tv, masked, damp, lower, upper = case
    op, y, mask, A = cp.problem(name)
    shape = tuple(op.grid.shape)
    n = math.prod(shape)
    s, _ = cp.ray_factors(y, mask, masked)
    Dw, voxel, _ = iso_matrix(shape, True, TV_WEIGHTS)
    _, up = pc.neighbours(shape, True, (1, 1, 1))
    r = LAM_TV / n
    xn = x.detach().cpu().numpy().reshape(-1).astype(np.float64)
    p = info['ray_dual'].detach().cpu().numpy().reshape(-1).astype(np.float64)
    q = flat_dual(info['dual'], up) / (1.0 + 12 * U)
    assert np.all(norms(q, voxel, n) <= r)
    yn = y.numpy().reshape(-1)
    J = cp.primal_value(kind, A, s, yn, None, damp, xn) + r * float(norms(Dw @ xn, voxel, n).sum())
    Dv = cp.dual_value(kind, A, s, yn, (Dw, None, None), damp, lower, upper, p, q)
    return J, Dv, (J - Dv) / abs(J)


def cp_solve(case, **kw):
    """chambolle_pock on a case of `cp_cases.solver_cases` with the iso term for its TV term."""
    from sph_raytracer_amd.retrieval import chambolle_pock
    name, kind, tv, masked, damp, lower, upper = case
    op, y, mask, _ = cp.problem(name)
    fns = [cp.fidelity(kind, mask if masked else 1), tv_term(True)]
    return chambolle_pock(op, y, fns, damp=damp, lower=lower, upper=upper,
                          num_iterations=kw.pop('iterations', cp.ITERATIONS), **kw)


def cp_cases():
    return [c for c in cp.solver_cases() if c[2]]


# ---- recorded measurements (test_iso_cpu.py repeats them) ----------------------------------------------
# pd_cases.MEASURED's rule, with iso_dense against the certified minimiser: the same problems,
# variants and bounds, L as `primal_dual` estimates it, dual_ratio 1, the TV term's ring closed on
# the unmasked variants (pd_cases.tv_wrap).  K is the first iteration from which the relative
# error stays under STAYS_UNDER; ITERATIONS the largest K; LIMIT 100 times the largest error any
# case has at ITERATIONS, at least the certificate's RADIUS_MAX.
RADIUS_MAX = pc.RADIUS_MAX
STAYS_UNDER = pc.STAYS_UNDER
ITERATIONS = 1513         # the largest K of MEASURED
LIMIT = 2.0e-4            # 100 x 1.99e-06, the largest error at 1513 iterations
# (problem, masked, smooth term's wrap_a, bounded): (K, the error at ITERATIONS, the radius)
MEASURED = {
    ('tiny', False, None, True): (710, 4.86e-11, 4.86e-08),
    ('tiny', False, None, False): (1470, 1.43e-06, 4.69e-08),
    ('tiny', True, None, True): (451, 8.72e-15, 5.2e-08),
    ('tiny', True, None, False): (1513, 1.99e-06, 5.12e-08),
    ('tiny', False, True, True): (256, 0, 2.77e-08),
    ('tiny', False, True, False): (506, 0, 2.87e-08),
    ('tiny', True, False, True): (246, 0, 2.73e-08),
    ('tiny', True, False, False): (504, 0, 2.63e-08),
    ('two_workgroups', False, None, True): (860, 1.01e-08, 7.7e-08),
    ('two_workgroups', False, None, False): (1394, 8.43e-07, 1.19e-07),
    ('two_workgroups', True, None, True): (930, 1.45e-08, 7.27e-08),
    ('two_workgroups', True, None, False): (1398, 7.98e-07, 1.12e-07),
    ('two_workgroups', False, True, True): (390, 0, 6.72e-08),
    ('two_workgroups', False, True, False): (1124, 3.11e-08, 7.59e-08),
    ('two_workgroups', True, False, True): (401, 2.09e-07, 6.09e-08),
    ('two_workgroups', True, False, False): (1081, 1.57e-08, 7.26e-08),
}
# chambolle_pock with the iso term: cp_cases.MEASURED's rule — the relative duality gap of the
# generic path after cp_cases.ITERATIONS iterations on the TV cases of cp_cases.solver_cases, and
# per kind 100 x the largest, rounded up in the third digit, at least cp_cases.GAP_FLOOR
CP_MEASURED = {
    'tiny-square-tv-unit-nodamp-box': 4.08e-15,
    'tiny-square-tv-masked-damp-box': 4.01e-16,
    'tiny-square-tv-masked-damp-lower0': 4.26e-16,
    'two_workgroups-square-tv-masked-damp-box': 1.23e-16,
    'tiny-abs-tv-unit-nodamp-box': 0.000319,
    'tiny-abs-tv-masked-damp-box': 1.47e-05,
    'tiny-abs-tv-masked-damp-lower0': 4.3e-06,
    'two_workgroups-abs-tv-masked-damp-box': 0.000308,
    'tiny-huber-tv-unit-nodamp-box': 1.08e-09,
    'tiny-huber-tv-masked-damp-box': 4.4e-16,
    'tiny-huber-tv-masked-damp-lower0': 9.4e-09,
    'two_workgroups-huber-tv-masked-damp-box': 0,
    'tiny-poisson-tv-unit-nodamp-box': 1.36e-08,
    'tiny-poisson-tv-masked-damp-box': 1.43e-08,
    'tiny-poisson-tv-masked-damp-lower0': 1.44e-08,
    'two_workgroups-poisson-tv-masked-damp-box': 9.61e-09,
}
CP_GAP_LIMIT = {'square': 1e-11, 'abs': 0.0319, 'huber': 9.4e-07, 'poisson': 1.44e-06}
