"""Inputs and references for the conjugate-gradient kernels (csrc/loss.hip: sphrt_cg_curvature_f64,
sphrt_cg_update_f64, sphrt_cg_direction_f64), shared by test_cg_cpu.py (which shows on the
references alone that the cases hold what they claim) and test_gpu_cg_kernels.py (which holds
the kernels to them).  No GPU dependency and no library call: numpy, Python integers and
Fractions; lengths, exact value set and guards are loop_cases'.

  exact    vectors of multiples of 1/8 (loop_cases.exact_values) and partial sums that are
           integers whose totals have a power-of-two ratio, so alpha and beta are small dyadic
           rationals whatever order the partials are summed in: every updated element and every
           workgroup's partial sum is then an exact multiple of a power of two, and a dropped
           wave total, a wrong stride or a partial left out of alpha is a wrong integer.
  random   normal vectors and partial sums: alpha and beta from the documented summation order
           restated in numpy (`kernel_sum`), the elementwise updates as exact rationals rounded
           once (loop_cases.fma) on a sample, which tells an fma from a multiply and an add, and
           the partial sums from the documented workgroup order (`block_partials`).

The last section is what test_cg_cpu.py and test_gpu_cg.py hold `retrieval.cg` itself to: the
dense system taken from the loss classes by autograd, its condition number, the Krylov
minimiser (torch is imported there, by the functions that differentiate)."""
import math

import numpy as np

import loop_cases as lc

THREADS, LENGTHS, GUARD = lc.THREADS, lc.LENGTHS, lc.GUARD
INF, NAN = lc.INF, lc.NAN


# ---- the documented summation orders -----------------------------------------------------------
def _wave_tree(v):
    """Lane 0 of the xor butterfly 32, 16, ..., 1 over the last axis (64 lanes), then the four
    wave totals in order onto +0.0.  v: (..., 256) -> (...)."""
    v = v.reshape(v.shape[:-1] + (4, 64))
    for half in (32, 16, 8, 4, 2, 1):
        v = v[..., :half] + v[..., half:2 * half]
    v = v[..., 0]
    return (((0.0 + v[..., 0]) + v[..., 1]) + v[..., 2]) + v[..., 3]


def kernel_sum(part):
    """SUM(part) of include/sphrt.h: thread t adds part[t], part[t + 256], ... (below n_part <=
    1024) in that order onto +0.0, then the wave tree.  (A thread past n_part holds +0.0; adding
    +0.0 to a sum that began as 0.0 + x changes nothing, so the padding is exact.)"""
    part = np.asarray(part, dtype=np.float64)
    assert part.ndim == 1 and 1 <= len(part) <= lc.MAX_BLOCKS
    pad = np.zeros(4 * THREADS)
    pad[:len(part)] = part
    pad = pad.reshape(4, THREADS)
    with np.errstate(all='ignore'):
        return float(_wave_tree((((0.0 + pad[0]) + pad[1]) + pad[2]) + pad[3]))


def block_partials(terms):
    """The partial sums a launch leaves of `terms` (one per element): thread t of workgroup b
    adds its elements b * 256 + t + k * 256 * grid in order onto +0.0, then the wave tree."""
    terms = np.asarray(terms, dtype=np.float64)
    n, g = len(terms), lc.grid_of(len(terms))
    passes = -(-n // (THREADS * g))
    pad = np.zeros(passes * g * THREADS)
    pad[:n] = terms
    pad = pad.reshape(passes, g, THREADS)
    with np.errstate(all='ignore'):
        acc = np.zeros((g, THREADS))
        for k in range(passes):
            acc = acc + pad[k]
        return _wave_tree(acc)


# ---- the scalar guards ---------------------------------------------------------------------------
def _div(a, b):
    with np.errstate(all='ignore'):
        return float(np.float64(a) / np.float64(b))


def alpha_ref(rr, php, rr_stop):
    """alpha of sphrt_cg_update_f64 from the two totals (rr_stop None: the NULL pointer)."""
    q = _div(rr, php)
    if (rr_stop is not None and rr <= rr_stop) or not php > 0 or math.isinf(q) or math.isnan(q):
        return 0.0
    return q


def beta_ref(rr_new, rr_old, rr_stop):
    """beta of sphrt_cg_direction_f64."""
    if (rr_stop is not None and rr_old <= rr_stop) or not rr_old > 0:
        return 0.0
    return _div(rr_new, rr_old)


# ---- exact cases ---------------------------------------------------------------------------------
DYADIC = [(1, 4), (2, 1), (1, 1), (3, 8)]      # alpha / beta as (numerator, denominator)


def exact_vectors(n, seed):
    """x, r, p, h: multiples of 1/8, |value| <= 64."""
    return tuple(lc.exact_values(n, seed + k) for k in range(4))


def dyadic_partials(n, num, den, seed):
    """(top, bottom): integer partial sums, one per workgroup of a launch over n elements, with
    top_j = num * k_j and bottom_j = den * k_j, k_j in 1..8: SUM(top) / SUM(bottom) is num / den
    exactly in any order (every sum is a small integer)."""
    k = np.random.default_rng(seed).integers(1, 9, size=lc.grid_of(n)).astype(np.float64)
    return num * k, den * k


def _ints(x, unit):
    k = np.asarray(x, dtype=np.float64) * unit
    ki = k.astype(np.int64)
    assert np.array_equal(ki.astype(np.float64), k)
    return ki


def exact_curvature(p, h, num, den):
    """-> (new h, partial sums of p * h) for c_damp = num / den, in integer arithmetic (h in
    1/(8 den), the products in 1/(64 den))."""
    hi = num * _ints(p, 8) + den * _ints(h, 8)
    s = lc._per_workgroup(_ints(p, 8) * hi, len(p))
    assert np.abs(s).max() < 2 ** 53
    return hi.astype(np.float64) / (8 * den), s.astype(np.float64) / (64 * den)


def exact_update(x, r, p, h, num, den):
    """-> (new x, new r, partial sums of r * r) for alpha = num / den."""
    xi = den * _ints(x, 8) + num * _ints(p, 8)
    ri = den * _ints(r, 8) - num * _ints(h, 8)
    s = lc._per_workgroup(ri * ri, len(x))
    assert s.max() < 2 ** 53
    u = 8 * den
    return xi.astype(np.float64) / u, ri.astype(np.float64) / u, s.astype(np.float64) / (u * u)


def exact_direction(p, r, num, den):
    """-> new p for beta = num / den."""
    return (num * _ints(p, 8) + den * _ints(r, 8)).astype(np.float64) / (8 * den)


# ---- random cases --------------------------------------------------------------------------------
def random_vectors(n, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3) for _ in range(4))


def random_partials(n, seed):
    """Two rows of positive partial sums whose totals depend on the order they are summed in."""
    rng = np.random.default_rng(seed)
    g = lc.grid_of(n)
    return rng.random(g) * 10.0 ** rng.integers(-3, 4, size=g), rng.random(g) + 0.5


def sample(n, seed, cap=256):
    """Indices the rational restatement is evaluated at: both ends and random ones."""
    idx = np.random.default_rng(seed).permutation(n)[:cap]
    return np.unique(np.concatenate([idx, [0, n - 1]]))


def fma(a, b, c):
    """loop_cases.fma on Python floats (numpy scalars would warn on inf * 0)."""
    return lc.fma(float(a), float(b), float(c))


def update_ref(x, r, p, h, alpha):
    """One element of sphrt_cg_update_f64: (fma(alpha, p, x), fma(-alpha, h, r))."""
    return fma(alpha, p, x), fma(-alpha, h, r)


def update_unfused(x, r, p, h, alpha):
    """Its neighbour, equal in real arithmetic: a multiply and an add, two roundings."""
    return x + alpha * p, r - alpha * h


# ---- special values ------------------------------------------------------------------------------
SPECIAL_ELEMENTS = [
    # (x, r, p, h): what the documented sequence makes of them is computed by lc.fma
    (0.0, -0.0, 0.0, -0.0), (-0.0, -0.0, -0.0, 0.0), (5e-324, -5e-324, 5e-324, 5e-324),
    (2.2e-308, 1e-160, -2.2e-308, 1e-160), (1e160, 1e160, 1e160, -1e160),
    (INF, 1.0, 1.0, 1.0), (1.0, -INF, 1.0, 1.0), (1.0, 1.0, INF, 1.0), (1.0, 1.0, 1.0, -INF),
    (INF, INF, -INF, INF), (NAN, 1.0, 1.0, 1.0), (1.0, NAN, 1.0, 1.0), (1.0, 1.0, NAN, 1.0),
    (1.0, 1.0, 1.0, NAN), (1e308, 1e308, 1e308, -1e308),
]


# ---- the solver against dense algebra ------------------------------------------------------------
# What test_cg_cpu.py and test_gpu_cg.py hold `retrieval.cg` to, over any operator that autograd
# can differentiate.  The system is taken from the loss classes, not from cg's own algebra: with
# J(x) = sum of the loss terms + damp * mean(x^2) (written here in torch), grad J(x) = N x - b, so
# b = -grad J(0) and column i of N is grad J(e_i) - grad J(0), e_i the unit volumes, each through
# the operator's forward and its backward.
KAPPA_MAX = 100.0
ITERATIONS = 200      # 2 sqrt(k) ((sqrt(k) - 1) / (sqrt(k) + 1))^200 < 1e-15 at k = 100
SOLVE_TOL = 1e-10     # what remains is rounding of order k * 2^-53 ~ 1e-14: four decades of margin
KRYLOV_TOL = 1e-9


def total(f, y, loss_fns, damp, x):
    """The objective cg minimises, from the loss classes themselves."""
    val = sum(fn(f, y, x, x) for fn in loss_fns)
    return val + damp * (x ** 2).mean() if damp else val


def grad_total(f, y, loss_fns, damp, x):
    import torch as tr
    leaf = x.detach().clone().requires_grad_()
    g, = tr.autograd.grad(total(f, y, loss_fns, damp, leaf), leaf)
    return g.detach()


def dense_system(f, y, loss_fns, damp, shape):
    """(N, b) as float64 numpy arrays, from grad J at zero and at the unit volumes."""
    import torch as tr
    zero = tr.zeros(shape, dtype=tr.float64, device=y.device)
    g0 = grad_total(f, y, loss_fns, damp, zero).reshape(-1)
    cols = []
    for i in range(zero.numel()):
        e = zero.clone()
        e.view(-1)[i] = 1.0
        cols.append(grad_total(f, y, loss_fns, damp, e).reshape(-1) - g0)
    N = tr.stack(cols, dim=1).cpu().numpy()
    return 0.5 * (N + N.T), -g0.cpu().numpy(), float(np.abs(N - N.T).max())


def damp_for(N0, n_vox):
    """A damp that brings the system N0 + (2 damp / V) I under a condition number of KAPPA_MAX:
    (lmax + c) / (lmin + c) <= K for c >= (lmax - K lmin) / (K - 1).  lmin >= 0 of a positive
    semi-definite N0 is dropped (voxels no ray crosses make it exactly 0) and K taken as half of
    KAPPA_MAX, so the bound holds with room for the rounding of the eigenvalues."""
    lmax = float(np.linalg.eigvalsh(N0)[-1])
    return lmax / (KAPPA_MAX / 2 - 1.0) * n_vox / 2.0


def condition(N):
    ev = np.linalg.eigvalsh(N)
    return float(ev[-1] / ev[0])


def krylov_minimiser(N, b, k):
    """argmin of the N-norm error over span{b, N b, ..., N^(k-1) b}: what k CG iterations from
    zero give in exact arithmetic.  Over an orthonormal basis Q of the span, x = Q c with
    (Q^T N Q) c = Q^T b."""
    K = [b]
    for _ in range(k - 1):
        K.append(N @ K[-1])
    Q, _ = np.linalg.qr(np.stack(K, axis=1))
    return Q @ np.linalg.solve(Q.T @ N @ Q, Q.T @ b)


def rel_err(a, b):
    return float(np.linalg.norm(np.asarray(a).reshape(-1) - b) / np.linalg.norm(b))
