"""Inputs and references for the projected-gradient kernels (csrc/loss.hip: sphrt_pg_step_f64,
sphrt_pg_momentum_f64) and for `retrieval.fista`, shared by test_fista_cpu.py (which shows on the
references alone that the cases hold what they claim) and the two GPU files.  No GPU dependency
and no library call: numpy, Python integers and Fractions; lengths, exact value set, guards and
the rational fma are loop_cases', the summation orders cg_cases'.

  exact    vectors of multiples of 1/8 (loop_cases.exact_values); step, c_damp, omega[j] and the
           bounds small dyadic rationals: every output element and every workgroup's partial sum
           is an exact multiple of a power of two in any order, so a wrong stride, a dropped wave
           total or a wrong clamp branch is a wrong integer.  Integer rows for part_gd whose
           totals are > 0, < 0 and exactly 0.
  random   normal vectors, a step and bounds that are no dyadic rationals: the elementwise
           sequence as exact rationals rounded once (loop_cases.fma) on a sample, the partial
           sums from the documented workgroup order (cg_cases.block_partials), GD from
           cg_cases.kernel_sum.
  special  signed zeros, denormals, infinities and NaN in each operand and in GD, and infinite
           bounds, through the documented sequence.

The last section is what `retrieval.fista` itself is held to: the bound-constrained minimiser of
the dense system of cg_cases.dense_system (projected gradient, then a polish on the free set,
the KKT conditions asserted), and the algorithm restated on the dense system."""
import math

import numpy as np

import cg_cases as cc
import loop_cases as lc

THREADS, LENGTHS, GUARD = lc.THREADS, lc.LENGTHS, lc.GUARD
INF, NAN = lc.INF, lc.NAN


# ---- the documented sequences, one element ----------------------------------------------------------
def clamp_ref(u, lower, upper):
    """The two compares as written: a NaN u fails both and stays NaN."""
    return lower if u < lower else (upper if u > upper else u)


def _mul(a, b):
    with np.errstate(all='ignore'):
        return float(np.float64(a) * np.float64(b))


def _sub(a, b):
    with np.errstate(all='ignore'):
        return float(np.float64(a) - np.float64(b))


def step_ref(z, g, x_old, c_damp, step, lower, upper):
    """One element of sphrt_pg_step_f64 -> (x_new, its term of GD, its term of MM)."""
    gp = cc.fma(c_damp, z, g)
    xn = clamp_ref(cc.fma(-step, gp, z), lower, upper)
    dz = _sub(z, xn)
    return xn, _mul(gp, _sub(xn, x_old)), _mul(dz, dz)


def step_unfused(z, g, x_old, c_damp, step, lower, upper):
    """Its neighbour, equal in real arithmetic: multiplies and adds, two roundings each."""
    gp = c_damp * z + g
    return clamp_ref(z - step * gp, lower, upper)


def j_ref(gd, j_in, n_omega):
    """j of sphrt_pg_momentum_f64 (a NaN GD fails the compare: no restart)."""
    return 1 if gd > 0 else min(j_in + 1, n_omega - 1)


def momentum_ref(x_new, x_old, omega_j):
    return cc.fma(omega_j, _sub(x_new, x_old), x_new)


# ---- exact cases ---------------------------------------------------------------------------------------
# (c_damp, step, lower, upper) as (numerator, denominator) pairs, denominators powers of two
EXACT_STEPS = [((1, 2), (1, 4), (-16, 1), (16, 1)), ((0, 1), (1, 2), (-12, 1), (35, 2)),
               ((3, 8), (1, 8), (-81, 4), (27, 1))]
EXACT_OMEGA = [0.5, 0.75, 0.25, 0.375, 0.125, 0.625, 0.875, 1.0]    # (eighths; omega[1] != 0 here)
EXACT_J_IN = [0, 3, 6, 7]                                           # (7 + 1 is held at 7)


def exact_vectors(n, seed):
    """z, g, x_old: multiples of 1/8, |value| <= 64."""
    return tuple(lc.exact_values(n, seed + k) for k in range(3))


def exact_step(z, g, x_old, c_damp, step, lower, upper):
    """-> (x_new, part_gd, part_mm, branch) in integer arithmetic; branch: -1 / 0 / +1 where the
    lower bound, no bound, the upper bound was taken."""
    (cn, cd), (sn, sd), (ln, ld), (un, ud) = c_damp, step, lower, upper
    n, unit = len(z), 8 * cd * sd
    zi, gi, xo = cc._ints(z, 8), cc._ints(g, 8), cc._ints(x_old, 8)
    gp = cn * zi + cd * gi                                   # in 1 / (8 cd)
    u = zi * (cd * sd) - sn * gp                             # in 1 / unit
    assert (ln * unit) % ld == 0 and (un * unit) % ud == 0
    lo, hi = ln * unit // ld, un * unit // ud
    branch = np.where(u < lo, -1, np.where(u > hi, 1, 0))
    xn = np.clip(u, lo, hi)
    s_gd = lc._per_workgroup(gp * (xn - xo * (cd * sd)), n)  # in 1 / (8 cd unit)
    s_mm = lc._per_workgroup((zi * (cd * sd) - xn) ** 2, n)  # in 1 / unit^2
    assert max(np.abs(s_gd).max(), s_mm.max()) < 2 ** 53
    return (xn.astype(np.float64) / unit, s_gd.astype(np.float64) / (8 * cd * unit),
            s_mm.astype(np.float64) / (unit * unit), branch)


def gd_partials(n, sign, seed):
    """Integer partial sums, one per workgroup of a launch over n elements, whose total (in any
    order) is > 0, < 0 or exactly 0 as `sign` says; with more than one partial, of mixed signs."""
    g = lc.grid_of(n)
    k = np.random.default_rng(seed).integers(-8, 9, size=g)
    k[-1] = sign * (1 + abs(int(k[:-1].sum()))) - int(k[:-1].sum()) if sign else -int(k[:-1].sum())
    return k.astype(np.float64)


def exact_momentum(x_new, x_old, omega_j):
    """-> z for omega_j a multiple of 1/8."""
    w = int(omega_j * 8)
    assert w / 8 == omega_j
    xn, xo = cc._ints(x_new, 8), cc._ints(x_old, 8)
    return (8 * xn + w * (xn - xo)).astype(np.float64) / 64.0


# ---- random cases --------------------------------------------------------------------------------------
RANDOM_C_DAMP = [0.3, 0.0, 0.125]     # (gp = c z + g is exact in numpy for the last two)


def random_vectors(n, seed):
    """z, g, x_old of one scale (so that the step moves z by its own order)."""
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(n) for _ in range(3))


def random_scalars(n):
    """(step, lower, upper): no dyadic rationals; about a quarter of u under and over."""
    return 0.37 + 1e-3 * (n % 11), -0.61, 0.67


def random_partials(n, seed, sign):
    """A row of partial sums of mixed signs whose total depends on the order of summation."""
    rng = np.random.default_rng(seed)
    g = lc.grid_of(n)
    v = rng.standard_normal(g) * 10.0 ** rng.integers(-3, 4, size=g)
    return v + sign * (abs(cc.kernel_sum(v)) + 1.0) / g


# ---- special values ------------------------------------------------------------------------------------
SPECIAL_ELEMENTS = [
    # (z, g, x_old)
    (0.0, -0.0, 0.0), (-0.0, 0.0, -0.0), (-0.0, -0.0, 0.0), (5e-324, -5e-324, 5e-324),
    (-5e-324, 5e-324, 0.0), (2.2e-308, 1e-160, -2.2e-308), (1e160, 1e160, -1e160),
    (1e308, -1e308, 1e308), (INF, 1.0, 1.0), (-INF, 1.0, 1.0), (1.0, INF, 1.0), (1.0, -INF, 1.0),
    (1.0, 1.0, INF), (1.0, 1.0, -INF), (INF, INF, INF), (-INF, INF, -INF), (NAN, 1.0, 1.0),
    (1.0, NAN, 1.0), (1.0, 1.0, NAN), (0.5, 0.25, 0.5), (-0.5, 0.0, 0.0),
]
SPECIAL_BOUNDS = [(0.0, INF), (-INF, INF), (-1.0, 1.0), (-INF, 0.5), (-0.0, 5e-324)]
# (GD as two partial sums, what the compare GD > 0 gives)
SPECIAL_GD = [((0.0, 0.0), False), ((-0.0, -0.0), False), ((5e-324, 0.0), True),
              ((0.0, -5e-324), False), ((INF, 1.0), True), ((1.0, -INF), False),
              ((INF, -INF), False), ((NAN, 1.0), False), ((1.0, NAN), False),
              ((1e308, 1e308), True), ((-1e308, -1e308), False), ((1.0, -1.0), False)]


def special_vectors(n, seed):
    """Random vectors with the special elements planted in both workgroups of n = 300 and at
    its ragged end -> (z, g, x_old, their indices)."""
    z, g, xo = (v.copy() for v in random_vectors(n, seed))
    where = []
    for base in (3, 250, n - len(SPECIAL_ELEMENTS)):
        for k, tup in enumerate(SPECIAL_ELEMENTS):
            z[base + k], g[base + k], xo[base + k] = tup
            where.append(base + k)
    return z, g, xo, np.array(where)


# ---- the solver against dense algebra ------------------------------------------------------------------
# The iteration count the solver tests run and the limit they hold the solution to, measured
# with fista_dense against bounded_minimiser (test_fista_cpu.py repeats the measurement): over
# the 4 x 3 x 6 problem and the 257-ray problem, the four mask / smooth variants of each, with
# the bounds 0.35 / 0.65 and without bounds, K is the largest iteration count at which
# fista_dense's relative error first stays under 1e-12, and the limit is 100 times the largest
# error any of them has at K (for another summation order and the atomics), 1e-12 at least.
LOWER, UPPER = 0.35, 0.65
STAYS_UNDER = 1e-12
ITERATIONS = 252          # the largest K of MEASURED
LIMIT = 8.6e-11           # 100 x 8.55e-13, the largest error at 252 iterations
# (problem, masked, smooth term's wrap_a, bounded): (K, the error at 252 iterations), with L as
# `fista` estimates it (10 power steps, margin 0.3); tools/fista_study.py prints this table
MEASURED = {
    ('tiny', False, None, True): (248, 4.51e-13),
    ('tiny', False, None, False): (212, 1.73e-14),
    ('tiny', True, None, True): (229, 2.86e-13),
    ('tiny', True, None, False): (223, 6.11e-14),
    ('tiny', False, True, True): (68, 3.67e-16),
    ('tiny', False, True, False): (126, 3.27e-16),
    ('tiny', True, False, True): (72, 3.72e-16),
    ('tiny', True, False, False): (133, 4.88e-16),
    ('two_workgroups', False, None, True): (235, 2.14e-13),
    ('two_workgroups', False, None, False): (252, 8.55e-13),
    ('two_workgroups', True, None, True): (239, 1.08e-13),
    ('two_workgroups', True, None, False): (238, 3.06e-13),
    ('two_workgroups', False, True, True): (124, 4.03e-16),
    ('two_workgroups', False, True, False): (226, 2.25e-14),
    ('two_workgroups', True, False, True): (117, 5.17e-16),
    ('two_workgroups', True, False, False): (223, 1.53e-14),
}


def active_sets(x, lower, upper):
    return x <= lower, x >= upper


def bounded_minimiser(N, b, lower, upper, patience=200, max_iterations=200000):
    """argmin 1/2 x^T N x - b^T x over lower <= x <= upper (either may be infinite), N symmetric
    positive definite: projected gradient with the step 1 / lambda_max until the active set has
    not changed for `patience` iterations, then the free set solved exactly with the bound
    voxels held (N_FF x_F = b_F - N_FB x_B).  The KKT conditions are asserted — the gradient at
    most 1e-12 |b| on the free set and of the right sign on each bound — and strict
    complementarity: at bound voxels |gradient| >= 1e-6 |b|_inf.  If the polished point fails
    them, the active set was not final yet and the iteration goes on."""
    N, b = np.asarray(N, dtype=np.float64), np.asarray(b, dtype=np.float64)
    step = 1.0 / float(np.linalg.eigvalsh(N)[-1])
    x = np.clip(np.zeros_like(b), lower, upper)
    sets, still, why = None, 0, 'no stable active set'
    for _ in range(max_iterations):
        x = np.clip(x - step * (N @ x - b), lower, upper)
        now = active_sets(x, lower, upper)
        still = still + 1 if sets is not None and all(
            np.array_equal(a, c) for a, c in zip(sets, now)) else 0
        sets = now
        if still < patience:
            continue
        still = 0
        lo, hi = sets
        free = ~(lo | hi)
        p = np.where(lo, lower, np.where(hi, upper, 0.0))
        if free.any():
            p[free] = np.linalg.solve(N[np.ix_(free, free)],
                                      b[free] - N[np.ix_(free, ~free)] @ p[~free])
        grad = N @ p - b
        checks = {
            'free voxels inside the bounds': bool(np.all((p[free] > lower) & (p[free] < upper))),
            'gradient on the free set': bool(np.all(np.abs(grad[free]) <= 1e-12 * np.linalg.norm(b))),
            'sign at the lower bound': bool(np.all(grad[lo] > 0)),
            'sign at the upper bound': bool(np.all(grad[hi] < 0)),
            'strict complementarity': bool(np.all(np.abs(grad[~free]) >= 1e-6 * np.abs(b).max())),
        }
        if all(checks.values()):
            return p
        why = [k for k, ok in checks.items() if not ok]
    raise AssertionError(f'bounded_minimiser: KKT conditions not met ({why})')


def omega_table(K):
    """OMEGA[0] = OMEGA[1] = 0, OMEGA[j] = (t_j - 1) / t_{j+1}, t_1 = 1: length K + 1."""
    omega, tj = [0.0], 1.0
    for _ in range(K):
        tn = (1.0 + math.sqrt(1.0 + 4.0 * tj * tj)) / 2.0
        omega.append((tj - 1.0) / tn)
        tj = tn
    return omega


def fista_dense(N, b, L, lower, upper, K, x0=None):
    """`retrieval.fista`'s algorithm restated on the dense system (grad = N z - b, the damping
    term inside N) -> (the iterates x_0 .. x_K, the restarts, MM_0 .. MM_{K-1})."""
    omega, step = omega_table(K), 1.0 / L
    x = np.clip(np.zeros_like(b) if x0 is None else np.asarray(x0, dtype=np.float64), lower, upper)
    z, j, xs, restarts, mm = x, 0, [x], [], []
    for k in range(K):
        g = N @ z - b
        u = z - step * g
        x_new = np.where(u < lower, lower, np.where(u > upper, upper, u))
        gd = float(g @ (x_new - x))
        mm.append(float(((z - x_new) ** 2).sum()))
        if gd > 0:
            j = 1
            if k >= 1:
                restarts.append(k)
        else:
            j += 1
        z = x_new + omega[j] * (x_new - x)
        x = x_new
        xs.append(x)
    return xs, restarts, mm


def first_stays_under(errors, bound=STAYS_UNDER):
    """The first k from which every later entry of `errors` is under `bound` (None: the last
    one is not)."""
    over = [k for k, e in enumerate(errors) if not e < bound]
    k = over[-1] + 1 if over else 0
    return k if k < len(errors) else None


def shares(x, lower, upper):
    """(share of voxels on the lower bound, on the upper bound, free)."""
    lo, hi = active_sets(np.asarray(x), lower, upper)
    return float(lo.mean()), float(hi.mean()), float((~(lo | hi)).mean())
