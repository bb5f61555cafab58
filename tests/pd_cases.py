"""Inputs and references for the primal-dual kernels (csrc/loss.hip: sphrt_pd_primal_f64,
sphrt_pd_dual_f64, declared in include/sphrt_pd.h) and for `retrieval.primal_dual`, shared by
test_pd_cpu.py (which shows on the references alone that the cases hold what they claim) and the
GPU files.  No GPU dependency and no library call: numpy, Python integers and Fractions; exact
value set, guards and the rational fma are loop_cases', the summation orders cg_cases', the
bounded minimiser fista_cases'.

  edges    `neighbours` restates the edge rules with numpy's take / roll on an index volume (an
           edge belongs to its lower voxel; the azimuth wrap edge to the ring's last voxel;
           na = 2 with a wrap: two edges; a ring of one: none), not with index arithmetic.
  exact    x, g, q, x_new, x_old multiples of 1/8; tau, sigma, c_damp, c_ax and the bounds small
           dyadic rationals: every output and every workgroup's partial sum is an exact multiple
           of a power of two, so a wrong neighbour, a missed wrap edge, a wrong clamp branch or
           a dropped wave total is a wrong integer.
  random   scalars that are no dyadic rationals: the element sequence as exact rationals rounded
           once per documented operation (cg_cases.fma), partial sums in the documented
           workgroup order (cg_cases.block_partials).
  special  signed zeros, denormals, infinities and NaN in each operand, and infinite bounds.

The last section is what `retrieval.primal_dual` itself is held to: the algorithm restated on
the dense system of cg_cases.dense_system with D as a dense matrix (`pd_dense`), and a minimiser
certified without the code under test (`certify`: a duality gap and strong convexity)."""
import math

import numpy as np

import cg_cases as cc
import fista_cases as fc
import loop_cases as lc

THREADS, GUARD = lc.THREADS, lc.GUARD
INF, NAN = lc.INF, lc.NAN

# (shape, [wrap_a ...]): the smallest that can still go wrong — one voxel; one axis; the double
# edge of a ring of two; a power-of-two block; 315 voxels (edges across a workgroup boundary);
# 274 365 (the grid-stride loop's second element: more than 1024 * 256)
SHAPES = [((1, 1, 1), [False, True]), ((1, 5, 1), [False, True]), ((3, 1, 2), [False, True]),
          ((4, 8, 16), [False, True]), ((5, 7, 9), [False, True]), ((67, 63, 65), [False, True])]
HAS = [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)]          # each has_* off in turn


def kernel_cases():
    """[(shape, wrap, has)]: every shape with the wrap on and off and each axis off in turn."""
    return [(shape, w, h) for shape, wraps in SHAPES for w in wraps for h in HAS]


# ---- the edge rules ----------------------------------------------------------------------------------
def neighbours(shape, wrap, has):
    """-> (lo, up), int64 (3, n): lo[ax, i] the lower neighbour of voxel i when an edge of axis ax
    arrives at i, up[ax, i] its upper neighbour when one leaves it (whose dual slot is i), -1
    where there is none."""
    n = math.prod(shape)
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    lo, up = -np.ones((3, n), dtype=np.int64), -np.ones((3, n), dtype=np.int64)
    for ax in range(3):
        if not has[ax] or shape[ax] < 2:
            continue
        if ax == 2 and wrap:
            up[ax] = np.roll(idx, -1, axis=2).reshape(-1)
            lo[ax] = np.roll(idx, 1, axis=2).reshape(-1)
        else:
            below = idx.take(range(shape[ax] - 1), axis=ax).reshape(-1)
            above = idx.take(range(1, shape[ax]), axis=ax).reshape(-1)
            up[ax, below] = above
            lo[ax, above] = below
    return lo, up


def adjoint_sum(q, lo, up):
    """s = D^T q as the kernel adds it, for every voxel at once: from +0.0, per axis the arriving
    edge (+), then the leaving one (-).  q: (3, n)."""
    s = np.zeros(q.shape[1])
    with np.errstate(all='ignore'):
        for ax in range(3):
            m = lo[ax] >= 0
            s[m] = s[m] + q[ax][lo[ax][m]]
            m = up[ax] >= 0
            s[m] = s[m] - q[ax][m]
    return s


# ---- the documented sequences, one element -------------------------------------------------------------
def primal_ref(i, x, g, q, lo, up, c_damp, tau, lower, upper):
    """One element of sphrt_pd_primal_f64 -> (x_new, its term of MM); Python floats (IEEE double
    operations) and the rational fma."""
    xi = float(x[i])
    gp = cc.fma(c_damp, xi, float(g[i]))
    s = 0.0
    for ax in range(3):
        if lo[ax, i] >= 0:
            s = s + float(q[ax][lo[ax, i]])
        if up[ax, i] >= 0:
            s = s - float(q[ax][i])
    xn = fc.clamp_ref(cc.fma(-tau, gp + s, xi), lower, upper)
    d = xn - xi
    return xn, d * d


def primal_unfused(i, x, g, q, lo, up, c_damp, tau, lower, upper):
    """Its neighbour, equal in real arithmetic: multiplies and adds, two roundings each."""
    s = float(adjoint_sum(np.asarray(q), lo, up)[i])
    return fc.clamp_ref(float(x[i]) - tau * ((c_damp * float(x[i]) + float(g[i])) + s), lower,
                        upper)


def dual_ref(i, x_new, x_old, q, up, sigma, c_ax):
    """One voxel of sphrt_pd_dual_f64 -> ([q_r, q_e, q_a] at slot i (None: no edge, untouched),
    its term of QQ)."""
    def xb(j):
        return cc.fma(2.0, float(x_new[j]), -float(x_old[j]))
    out, t = [None, None, None], 0.0
    for ax in range(3):
        j = up[ax, i]
        if j < 0:
            continue
        qo = float(q[ax][i])
        qn = fc.clamp_ref(cc.fma(sigma, xb(j) - xb(i), qo), -c_ax[ax], c_ax[ax])
        out[ax] = qn
        d = qn - qo
        t = t + d * d
    return out, t


def dual_terms(q_new, q_old, up):
    """Every voxel's term of QQ from the new and the old dual (numpy float64: the same IEEE
    operations): the axes' squared changes added in the order r, e, a onto +0.0."""
    t = np.zeros(q_new.shape[1])
    with np.errstate(all='ignore'):
        for ax in range(3):
            m = up[ax] >= 0
            d = q_new[ax][m] - q_old[ax][m]
            t[m] = t[m] + d * d
    return t


# ---- exact cases ---------------------------------------------------------------------------------------
# (c_damp, tau, lower, upper) and (sigma, c_r, c_e, c_a) as (numerator, denominator) pairs,
# denominators powers of two
EXACT_PRIMAL = [((1, 2), (1, 4), (-16, 1), (16, 1)), ((0, 1), (1, 8), (-12, 1), (35, 2)),
                ((3, 8), (1, 2), (-81, 4), (27, 1))]
EXACT_DUAL = [((1, 4), (16, 1), (24, 1), (8, 1)), ((1, 8), (35, 2), (10, 1), (81, 4)),
              ((3, 2), (48, 1), (0, 1), (33, 1))]


def exact_vectors(shape, seed):
    """x, g (n), q (3, n) and x_new, x_old (n): multiples of 1/8, |value| <= 64."""
    n = math.prod(shape)
    x, g, xn, xo = (lc.exact_values(n, seed + k) for k in range(4))
    q = np.stack([lc.exact_values(n, seed + 4 + k) for k in range(3)])
    return x, g, q, xn, xo


def exact_primal(x, g, q, lo, up, c_damp, tau, lower, upper):
    """-> (x_new, part_mm, branch) in integer arithmetic; branch -1 / 0 / +1 by the clamp taken."""
    (cn, cd), (tn, td), (ln, ld), (un, ud) = c_damp, tau, lower, upper
    n, unit = len(x), 8 * cd * td
    xi, gi = cc._ints(x, 8), cc._ints(g, 8)
    qi = np.stack([cc._ints(v, 8) for v in q])
    si = np.zeros(n, dtype=np.int64)
    for ax in range(3):
        m = lo[ax] >= 0
        si[m] += qi[ax][lo[ax][m]]
        m = up[ax] >= 0
        si[m] -= qi[ax][m]
    gs = cn * xi + cd * gi + cd * si                        # gp + s in 1 / (8 cd)
    u = xi * (cd * td) - tn * gs                            # in 1 / unit
    assert (ln * unit) % ld == 0 and (un * unit) % ud == 0
    lo_i, hi_i = ln * unit // ld, un * unit // ud
    branch = np.where(u < lo_i, -1, np.where(u > hi_i, 1, 0))
    xn = np.clip(u, lo_i, hi_i)
    s_mm = lc._per_workgroup((xn - xi * (cd * td)) ** 2, n)
    assert s_mm.max() < 2 ** 53 and np.abs(u).max() < 2 ** 40
    return xn.astype(np.float64) / unit, s_mm.astype(np.float64) / (unit * unit), branch


def exact_dual(x_new, x_old, q, up, sigma, c_ax):
    """-> (q_new (3, n), part_qq, branch (3, n): -1 / 0 / +1, and 2 where there is no edge)."""
    (sn, sd) = sigma
    n, unit = len(x_new), 8 * sd
    xb = 2 * cc._ints(x_new, 8) - cc._ints(x_old, 8)
    qi = np.stack([cc._ints(v, 8) for v in q])
    q_new, branch = qi * sd, np.full((3, n), 2, dtype=np.int64)
    term = np.zeros(n, dtype=np.int64)
    for ax in range(3):
        m = up[ax] >= 0
        cn_, cd_ = c_ax[ax]
        assert (cn_ * unit) % cd_ == 0
        cl = cn_ * unit // cd_
        v = sd * qi[ax][m] + sn * (xb[up[ax][m]] - xb[m])
        branch[ax][m] = np.where(v < -cl, -1, np.where(v > cl, 1, 0))
        q_new[ax][m] = np.clip(v, -cl, cl)
        term[m] += (q_new[ax][m] - sd * qi[ax][m]) ** 2
    s_qq = lc._per_workgroup(term, n)
    assert s_qq.max() < 2 ** 53
    out = q_new.astype(np.float64) / unit
    for ax in range(3):                       # (the lower clamp stores -c_ax: -0.0 for c_ax = 0)
        out[ax][branch[ax] == -1] = -(c_ax[ax][0] / c_ax[ax][1])
    return out, s_qq.astype(np.float64) / (unit * unit), branch


# ---- random cases --------------------------------------------------------------------------------------
RANDOM_C_DAMP = [0.3, 0.0]


def random_vectors(shape, seed):
    """x, g (n), q (3, n), x_new, x_old (n), of one scale."""
    rng, n = np.random.default_rng(seed), math.prod(shape)
    x, g = rng.standard_normal(n), rng.standard_normal(n)
    q = rng.standard_normal((3, n))
    return x, g, q, rng.standard_normal(n), rng.standard_normal(n)


def random_scalars(n):
    """(tau, lower, upper, sigma, (c_r, c_e, c_a)): no dyadic rationals; each clamp branch of
    either kernel takes a fair share."""
    return 0.37 + 1e-3 * (n % 11), -0.61, 0.67, 0.23 + 1e-3 * (n % 7), (0.9, 1.1, 0.7)


# ---- special values ------------------------------------------------------------------------------------
SPECIALS = [0.0, -0.0, 5e-324, -5e-324, 2.2e-308, 1e-160, -1e160, 1e308, -1e308, INF, -INF, NAN]
SPECIAL_SHAPE = (5, 7, 9)
SPECIAL_BOUNDS = fc.SPECIAL_BOUNDS
SPECIAL_C = [(0.9, 1.1, 0.7), (1e308, 0.0, 5e-324)]   # (an infinite clamp is refused on the host)


def special_vectors(seed):
    """random_vectors over SPECIAL_SHAPE with every SPECIALS value planted in each operand in
    turn (x, g, the three q, x_new, x_old), at voxels spread over both workgroups -> (the
    vectors, the planted voxel indices)."""
    x, g, q, xn, xo = (v.copy() for v in random_vectors(SPECIAL_SHAPE, seed))
    n, where = len(x), []
    targets = [x, g, q[0], q[1], q[2], xn, xo]
    for k, tgt in enumerate(targets):
        for j, val in enumerate(SPECIALS):
            i = (17 * k + 23 * j + 5) % n
            tgt[i] = val
            where.append(i)
    return (x, g, q, xn, xo), np.unique(where)


# ---- the solver against dense algebra ------------------------------------------------------------------
LOWER, UPPER = fc.LOWER, fc.UPPER
LAM_TV = 0.02                 # see `certify`: some edges flat, some not, on every case
TV_WEIGHTS = (1.0, 0.5, 2.0)
DUAL_RATIO = 1.0
K_CAP = 20000
VARIANTS = [(False, None), (True, None), (False, True), (True, False)]   # (masked, smooth wrap)


def tv_wrap(masked):
    """The TV term's wrap_a of a variant: the ring closed on the unmasked variants, open on the
    masked ones — of VARIANTS' two unmasked and two masked entries one each has a square smooth
    term, so the TV ring occurs closed and open with and without it."""
    return not masked


def tv_matrix(shape, wrap, weights):
    """(D, axis of every row) — the dense forward-difference matrix over the axes that have
    edges (weight > 0 and length > 1), rows ordered by axis, then by the edge's dual slot."""
    has = [w > 0 and n > 1 for w, n in zip(weights, shape)]
    _, up = neighbours(shape, wrap, has)
    n = math.prod(shape)
    rows, axis = [], []
    for ax in range(3):
        for i in np.flatnonzero(up[ax] >= 0):
            row = np.zeros(n)
            row[up[ax, i]] += 1.0
            row[i] -= 1.0
            rows.append(row)
            axis.append(ax)
    return np.array(rows), np.array(axis), 4.0 * sum(has)


def pd_steps(L, ratio, B):
    return 1.0 / ((1.0 + ratio) * L), ratio * L / B


def pd_dense(N, b, D, c, lower, upper, L, ratio, K, B, x0=None, q0=None, keep=True):
    """`retrieval.primal_dual`'s algorithm restated on the dense system (grad = N x - b, the
    damping term inside N; c: the clamp of every row of D) -> (the iterates x_0 .. x_K, or the
    last one only, q_K, MM_0 .. MM_{K-1}, QQ_0 .. QQ_{K-1})."""
    tau, sigma = pd_steps(L, ratio, B)
    x = np.clip(np.zeros_like(b) if x0 is None else np.asarray(x0, dtype=np.float64), lower, upper)
    q = np.zeros(len(D)) if q0 is None else np.asarray(q0, dtype=np.float64)
    xs, mm, qq = [x], [], []
    for _ in range(K):
        u = x - tau * ((N @ x - b) + D.T @ q)
        x_new = np.where(u < lower, lower, np.where(u > upper, upper, u))
        v = q + sigma * (D @ (2 * x_new - x))
        q_new = np.where(v < -c, -c, np.where(v > c, c, v))
        mm.append(float(((x_new - x) ** 2).sum()))
        qq.append(float(((q_new - q) ** 2).sum()))
        x, q = x_new, q_new
        if keep:
            xs.append(x)
    return (xs if keep else x), q, mm, qq


def primal_value(N, b, D, c, x):
    """P(x) = 1/2 x^T N x - b^T x + sum c |D x| in extended precision."""
    N, b, D, c, x = (np.asarray(v, dtype=np.longdouble) for v in (N, b, D, c, x))
    return 0.5 * x @ (N @ x) - b @ x + (c * np.abs(D @ x)).sum()


def dual_lower_bound(N, rhs, z, lower, upper, lam_min):
    """A rigorous lower bound of min over the box of phi(x) = 1/2 x^T N x - rhs^T x, from any
    point z of the box and N >= lam_min I: phi(x) >= phi(z) + grad^T (x - z) + lam_min / 2
    |x - z|^2, minimised over the box coordinate by coordinate (extended precision)."""
    ld = np.longdouble
    N, rhs, z = (np.asarray(v, dtype=ld) for v in (N, rhs, z))
    grad = N @ z - rhs
    step = np.clip(-grad / ld(lam_min), ld(lower) - z, ld(upper) - z)
    return 0.5 * z @ (N @ z) - rhs @ z + (grad * step + 0.5 * ld(lam_min) * step * step).sum()


def certify(N, b, D, c, lower, upper, L, B, ratio=DUAL_RATIO, chunk=2000, max_chunks=400):
    """-> (x*, q*, radius): `pd_dense` run until it stalls (no change of x or q over a chunk of
    iterations beyond 1e-15 relative), and the certificate of its end point, built without the
    code under test.  For every |q| <= c, P(x) >= 1/2 x^T N x - (b - D^T q)^T x, so the minimum
    of the right-hand side over the box — found with fista_cases.bounded_minimiser, bounded from
    below by `dual_lower_bound` — is a lower bound of min P; P is lam_min-strongly convex, so the
    true minimiser x satisfies |x - x*| <= sqrt(2 (P(x*) - dual) / lam_min) = radius."""
    x, q = None, None
    for _ in range(max_chunks):
        x_new, q_new, _, _ = pd_dense(N, b, D, c, lower, upper, L, ratio, chunk, B, x0=x, q0=q,
                                      keep=False)
        still = x is not None and np.abs(x_new - x).max() <= 1e-15 * np.abs(x_new).max() \
            and np.abs(q_new - q).max() <= 1e-15 * c.max()
        x, q = x_new, q_new
        if still:
            break
    else:
        raise AssertionError('certify: pd_dense did not stall')
    return x, q, radius_of(N, b, D, c, x, q, lower, upper)


def radius_of(N, b, D, c, x, q, lower, upper):
    """The radius of `certify`'s ball around x, from any x inside the box and any |q| <= c."""
    x, q = np.asarray(x, dtype=np.float64), np.asarray(q, dtype=np.float64)
    assert np.all((x >= lower) & (x <= upper)) and np.all(np.abs(q) <= c)
    lam_min = float(np.linalg.eigvalsh(N)[0])
    assert lam_min > 0
    rhs = b - D.T @ q
    try:
        z = fc.bounded_minimiser(N, rhs, lower, upper, max_iterations=20000)
    except AssertionError:
        # (no strict complementarity — q* is not unique, and a voxel may sit on its bound with a
        # zero multiplier: projected gradient from x; the lower bound holds for any z)
        z, step = x, 1.0 / float(np.linalg.eigvalsh(N)[-1])
        for _ in range(2000):
            z = np.clip(z - step * (N @ z - rhs), lower, upper)
    gap = float(primal_value(N, b, D, c, x) - dual_lower_bound(N, rhs, z, lower, upper, lam_min))
    # what rounding can have added to or taken from the gap: two values, each a sum of products
    # over n voxels in extended precision, of terms of this size
    size = float(0.5 * np.abs(x) @ (np.abs(N) @ np.abs(x)) + (np.abs(b) + np.abs(rhs)) @ np.abs(x)
                 + (c * np.abs(D @ x)).sum())
    err = 2.0 * len(x) * float(np.finfo(np.longdouble).eps) * size
    assert gap >= -err, (gap, err)
    return math.sqrt(2.0 * (max(gap, 0.0) + err) / lam_min)


def edge_shares(q, c):
    """(share of edges that are flat at the minimiser: |q| < c; share that carry a jump: |q| = c)."""
    flat = np.abs(q) < c
    return float(flat.mean()), float((~flat).mean())


def first_stays_under(errors, bound):
    return fc.first_stays_under(errors, bound)


# The iteration count the solver tests run and the limit they hold the solution to, measured with
# pd_dense against the certified minimiser (test_pd_cpu.py repeats the measurement;
# tools/pd_study.py prints this table): over cg_cases' tiny (4 x 3 x 6) and two_workgroups (257
# rays, 5 x 6 x 10) problems, the four mask / smooth variants of each, with the bounds 0.35 / 0.65
# and without, L as `primal_dual` estimates it and dual_ratio 1.  The certificate's radius is at
# most RADIUS_MAX relative to |x*| on every case; STAYS_UNDER is chosen a decade above it (the
# bound cannot be tighter than what the certificate supports); K is the largest iteration count
# at which pd_dense's relative error first stays under STAYS_UNDER, and LIMIT 100 times the
# largest error any case has at ITERATIONS (for another summation order and the float64
# atomics), RADIUS_MAX at least.
RADIUS_MAX = 2e-7
STAYS_UNDER = 2e-6
ITERATIONS = 1513         # the largest K of MEASURED
LIMIT = 2.0e-4            # 100 x 1.99e-06, the largest error at 1513 iterations
# (problem, masked, smooth term's wrap_a, bounded): (K, the error at ITERATIONS, the radius)
MEASURED = {
    ('tiny', False, None, True): (779, 3.72e-10, 4.89e-08),
    ('tiny', False, None, False): (1470, 1.43e-06, 4.68e-08),
    ('tiny', True, None, True): (802, 8.11e-10, 4.51e-08),
    ('tiny', True, None, False): (1513, 1.99e-06, 5.03e-08),
    ('tiny', False, True, True): (354, 0, 2.61e-08),
    ('tiny', False, True, False): (496, 0, 2.61e-08),
    ('tiny', True, False, True): (364, 0, 2.54e-08),
    ('tiny', True, False, False): (506, 0, 2.63e-08),
    ('two_workgroups', False, None, True): (1189, 1.51e-07, 7.6e-08),
    ('two_workgroups', False, None, False): (1451, 1.23e-06, 1.16e-07),
    ('two_workgroups', True, None, True): (1179, 1.33e-07, 7.3e-08),
    ('two_workgroups', True, None, False): (1444, 1.16e-06, 1.09e-07),
    ('two_workgroups', False, True, True): (394, 0, 6.55e-08),
    ('two_workgroups', False, True, False): (1122, 3.03e-08, 7.57e-08),
    ('two_workgroups', True, False, True): (366, 0, 6.23e-08),
    ('two_workgroups', True, False, False): (1081, 1.56e-08, 6.98e-08),
}
