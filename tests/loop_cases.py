"""Inputs and references for the retrieval loop's elementwise kernels (csrc/loss.hip: residual,
regulariser, one-launch Adam), shared by test_loop_cases_cpu.py (which shows on the references
alone that the cases hold what they claim) and test_gpu_loop_kernels.py (which holds the kernels
to them).  No GPU dependency and no library call: numpy, Python integers and Fractions.

Three things a launch of these kernels can get wrong without the older tests noticing:
  lengths   loss_grid caps a launch at 1024 workgroups of 256, so up to 262144 elements a thread
            owns one element, the one adam_neg_kernel pre-loads before its barrier; LENGTHS goes
            round the wave, workgroup and launch edges and on to three and four per thread.
  sums      on the exact value set every sum is exact in float64 in any order, so a workgroup's
            partial is one integer, and a dropped wave total or a wrong stride is a wrong
            integer instead of a difference inside a tolerance.
  values    signed zeros, denormals, g * g under- and overflow, infinities and NaN (SPECIALS),
            and an exact-rational restatement of the documented FOREACH operation sequence
            (foreach_step_ref) that tells the documented forms from their neighbours."""
import math
from fractions import Fraction

import numpy as np

THREADS, MAX_BLOCKS = 256, 1024          # kLossThreads, kLossMaxBlocks
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 262143, 262144, 262145, 786433]
STRIDE = THREADS * MAX_BLOCKS            # 262144: elements per pass of a full launch
GUARD = 64                               # NaN elements on either side of every output buffer


def grid_of(n):
    """sphrt_loss_partials restated: ceil(n / 256) workgroups, at least 1, at most 1024."""
    b = (n + THREADS - 1) // THREADS
    return min(max(b, 1), MAX_BLOCKS)


def elems_per_thread(n):
    """How many elements each launched thread owns: thread t takes t, t + S, t + 2S, ... < n
    with S = 256 * grid_of(n).  -> int64 array over the launch's threads."""
    s = THREADS * grid_of(n)
    t = np.arange(s, dtype=np.int64)
    return np.where(t < n, (n - 1 - t) // s + 1, 0)


def steps_of(n):
    return 3 if n >= 262143 else 20


# ---- exact value set ---------------------------------------------------------------------------
def exact_values(n, seed):
    """n multiples of 1/8 with |value| <= 64, signs mixed, the first and the last element
    negative (so a quarter of every length, n = 1 included, is negative, and the ragged last
    element of a launch always has a term in the regulariser's sum)."""
    k = np.random.default_rng(seed).integers(-512, 513, size=n)
    for i in (0, n - 1):
        k[i] = -(abs(int(k[i])) % 512) - 1
    return k.astype(np.float64) / 8.0


def residual_inputs(n):
    """(yhat, y) of the exact set whose last elements differ: the ragged last element always has
    a term in the residual's sum."""
    yhat, y = exact_values(n, 2 * n + 1), exact_values(n, 2 * n + 2)
    if y[-1] == yhat[-1]:
        y[-1] = -y[-1]
    return yhat, y


def _eighths(x):
    k = np.asarray(x, dtype=np.float64) * 8.0
    ki = k.astype(np.int64)
    assert np.array_equal(ki.astype(np.float64), k) and np.abs(ki).max() <= 512
    return ki


def _per_workgroup(terms, n):
    """Integer terms summed per owning workgroup: element i belongs to (i // 256) mod grid."""
    g = grid_of(n)
    out = np.zeros(g, dtype=np.int64)
    np.add.at(out, (np.arange(n, dtype=np.int64) // THREADS) % g, terms)
    return out


def neg_partials_ref(d, n):
    """Per workgroup, the exact sum of |min(d_i, 0)| over the elements it owns (integer
    arithmetic in eighths; the float64 result is exact)."""
    k = _eighths(d[:n])
    s = _per_workgroup(np.where(k < 0, -k, 0), n)
    assert s.max() < 2 ** 53
    return s.astype(np.float64) / 8.0


def sq_partials_ref(yhat, y, n):
    """Per workgroup, the exact sum of (yhat_i - y_i)^2 (integer arithmetic in 64ths)."""
    r = _eighths(yhat[:n]) - _eighths(np.asarray(y[:n], dtype=np.float64))
    s = _per_workgroup(r * r, n)
    assert s.max() < 2 ** 53
    return s.astype(np.float64) / 64.0


# ---- special value set -------------------------------------------------------------------------
INF, NAN = float('inf'), float('nan')
SPECIALS = [0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-160, -1e-160, 1e160, -1e160,
            INF, -INF, NAN]
SPECIAL_V = [0.0, 5e-324, 1e300]


def special_tuples():
    """(p, g, exp_avg, exp_avg_sq): every SPECIALS value as a parameter and as a gradient beside
    benign partners, every SPECIAL_V second moment with a zero and a non-zero gradient, and the
    combinations where two of them meet (signed zeros throughout, g * g underflow and overflow,
    opposite infinities, NaN in every slot)."""
    out = [(s, 0.75, 0.125, 0.01) for s in SPECIALS]
    out += [(0.5, s, 0.125, 0.01) for s in SPECIALS]
    out += [(0.5, g, m, v) for v in SPECIAL_V for g, m in ((0.25, 0.125), (0.0, 0.0))]
    out += [(-0.0, 0.0, 0.0, 0.0), (0.0, -0.0, -0.0, 0.0), (-0.0, -0.0, -0.0, 0.0),
            (0.0, 0.0, 0.0, 0.0), (-5e-324, 5e-324, 0.0, 0.0), (5e-324, -5e-324, -5e-324, 5e-324),
            (1e-160, 1e-160, 0.0, 0.0), (-1e-160, -1e-160, 1e-160, 5e-324),
            (1e160, 1e160, 0.0, 1e300), (-1e160, -1e160, 1e160, 1e300),
            (INF, -INF, 0.0, 0.0), (-INF, INF, 0.0, 1e300), (-INF, -INF, 0.0, 0.0),
            (NAN, NAN, 0.0, 0.0), (-2.2e-308, 2.2e-308, -2.2e-308, 5e-324)]
    return out


LAST_TUPLE = (-1e160, 1e-160, 0.125, 1e300)      # the last element of every length
_BASES = (20, STRIDE + 5, 2 * STRIDE + 7)        # one copy of every tuple per stride of 786433


def special_placement(n):
    """[(index, tuple)]: tuple j at _BASES[c] + j for every copy c that fits below the last
    element, and LAST_TUPLE at n - 1."""
    tuples = special_tuples()
    out = [(b + j, tup) for b in _BASES for j, tup in enumerate(tuples) if b + j < n - 1]
    return out + [(n - 1, LAST_TUPLE)]


def plant(n, p, g, m, v):
    """Write the special tuples into the four float64 arrays (in place) -> their indices."""
    idx = []
    for i, (a, b, c, d) in special_placement(n):
        p[i], g[i], m[i], v[i] = a, b, c, d
        idx.append(i)
    return np.asarray(idx, dtype=np.int64)


def sample_indices(n, special_idx, seed, cap=512):
    """Every special index plus random ones, at most `cap` in all (the emulator's sample)."""
    special_idx = np.unique(special_idx)
    assert len(special_idx) <= cap
    rest = np.setdiff1d(np.arange(n, dtype=np.int64), special_idx)
    extra = np.random.default_rng(seed).permutation(rest)[:cap - len(special_idx)]
    return np.sort(np.concatenate([special_idx, extra]))


# ---- the FOREACH step, exact-rational ------------------------------------------------------------
def _finite(x):
    return not (math.isinf(x) or math.isnan(x))


def fma(a, b, c):
    """round(a * b + c) with one rounding: the exact rational, then float().  Non-finite operands
    and exact zeros by the IEEE rules (0 * inf is NaN; an exact zero sum is +0 unless both
    addends are -0; an underflow keeps the exact result's sign)."""
    if math.isnan(a) or math.isnan(b) or math.isnan(c):
        return NAN
    if not (_finite(a) and _finite(b)):
        return a * b + c                      # inf * 0 = NaN, inf + -inf = NaN, else +-inf
    if not _finite(c):
        return c
    if a == 0.0 or b == 0.0:
        return a * b + c                      # a signed zero plus c: one IEEE add, exact
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        return 0.0                            # a non-zero product cancelled by c
    try:
        return float(exact)
    except OverflowError:
        return INF if exact > 0 else -INF


def _sqrt(x):
    return NAN if math.isnan(x) or x < 0 else math.sqrt(x)


def bias_corrections(hyper, t):
    """(step_size, bc2_sqrt) as retrieval._split_adam computes them (Python floats)."""
    st = float(t)
    return (hyper['lr'] / (1 - hyper['beta1'] ** st)) * -1, (1 - hyper['beta2'] ** st) ** 0.5


def foreach_step_ref(p, g, m, v, hyper, t, c_neg, form='documented'):
    """One element's FOREACH step -> (p, exp_avg, exp_avg_sq): the sequence documented above
    adam_neg_kernel, operation by operation.  `form` swaps one operation for a neighbour that is
    equal in real arithmetic ('unfused_v': beta2 * v + ob2 * g * g in single operations;
    'lerp_large': the large-weight lerp form whatever the weight), for the test that the
    emulator can tell them apart."""
    beta1, beta2, eps, wd = hyper['beta1'], hyper['beta2'], hyper['eps'], hyper['wd']
    step_size, bc2s = bias_corrections(hyper, t)
    if c_neg is not None and p < 0.0:
        g = g - c_neg
    if wd != 0:
        g = fma(wd, p, g)
    ob1, ob2 = 1 - beta1, 1 - beta2
    if abs(ob1) < 0.5 and form != 'lerp_large':
        m_new = fma(ob1, g - m, m)
    else:
        m_new = fma(-(g - m), 1.0 - ob1, g)
    if form == 'unfused_v':
        v_new = beta2 * v + ob2 * g * g
    else:
        v_new = fma(ob2, g * g, v * beta2)
    den = _sqrt(v_new)
    den = den / bc2s
    den = den + eps
    return fma(step_size, m_new / den, p), m_new, v_new


# ---- the inputs of one length --------------------------------------------------------------------
def adam_inputs(n, seed):
    """{'p', 'm', 'v': float64 arrays, 'g': one array per step, 'special': indices}: randn
    parameters, randn gradients spanning four decades and non-zero moments (with zero moments the
    two lerp forms are one rounding of the same number at step 1, and a moment read from the
    wrong element is a zero read for a zero), with the special tuples planted (their gradients
    again at every step)."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n)
    # moments as one step of the default betas from zero leaves them, for a gradient of the
    # first step's size: the second moment and (1 - beta2) g^2 are then of one magnitude
    m, v = 1e-3 * rng.standard_normal(n), 1e-3 * (1e-2 * rng.standard_normal(n)) ** 2
    gs = [rng.standard_normal(n) * 10.0 ** (it % 4 - 2) for it in range(steps_of(n))]
    special = plant(n, p, gs[0], m, v)
    for g in gs[1:]:
        plant(n, np.empty(n), g, np.empty(n), np.empty(n))
    return {'p': p, 'm': m, 'v': v, 'g': gs, 'special': special}


def same_or_both_nan(a, b):
    """Two floats bit for bit (so -0.0 != +0.0), or both NaN (payloads are not compared)."""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)
