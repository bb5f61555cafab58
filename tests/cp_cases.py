"""Cases, references and every bound of the tests of retrieval.chambolle_pock and of its ray-side
launch sphrt_cp_ray_dual_f64 (include/sphrt_cp.h) — no tests here; numpy and torch on the CPU,
no library call.  test_cp_cpu.py shows on the CPU that the references hold what they claim and
that the recorded numbers reproduce; the GPU files hold the kernel and the direct path to them.

  proxes      random (a, sigma, s, y) per kind, with s = 0, y = 0 and arguments on both sides of
              every clamp, and the optimality condition p in d phi(z), z = (a - p) / sigma, as a
              relative violation (`prox_violation`);
  restatement the launch op by op in torch (`ray_dual_ref`; the fmas by `fma_eft` on the device
              or `fma_exact` through rationals on the host), with the partial
              sums in the documented workgroup order (cg_cases.block_partials);
  solver      the two small problems of pd_cases (4 x 3 x 6 over 72 rays, 5 x 6 x 10 over 257
              rays) with the dense matrix of the CPU oracle: the primal value J(x), the dual
              value D(p, q) with phi* written out per kind, the relative gap.

Every number used as a bound stands below with the CPU measurement it came from
(tools/cp_study.py prints them):

  PROX_BOUND        16 x PROX_MEASURED, the largest relative violation `_cp_prox` itself shows in
                    float64 on the draws of `prox_draws`;
  GAP_LIMIT         per kind, 100 x the largest relative duality gap in MEASURED, each at
                    ITERATIONS iterations of the generic path with the default dual_ratio (at
                    least GAP_FLOOR, what the recomputation resolves);
  SENSITIVITY       per GPU configuration, how far x, p and q of the CPU reference move after
                    SENS_ITERATIONS iterations when the oracle matrix's row and column sums are
                    formed in the opposite order (CpuOperator(reverse=True), as
                    tools/gd_sensitivity.py measures gd); the GPU tests allow 16 x that, at
                    least 1e-13 of the largest magnitude (`bounds`: gd_cases' rule).
"""
import functools
import math

import numpy as np

import pd_cases as pc

KINDS = ['square', 'abs', 'huber', 'poisson']
KIND_ID = {k: i for i, k in enumerate(KINDS)}       # SPHRT_CP_*
LAM_F = 1.5
HUBER_DELTA = 0.05
POISSON_EPS = 1e-8
LOWER, UPPER = pc.LOWER, pc.UPPER
DAMP = 0.05                   # the damped variants' damp (c = 2 damp / V)


def par_of(kind):
    return {'huber': HUBER_DELTA, 'poisson': POISSON_EPS}.get(kind, 0.0)


def fidelity(kind, mask=1):
    from sph_raytracer_amd.loss import AbsLoss, HuberLoss, PoissonLoss, SquareLoss
    kw = dict(projection_mask=mask)
    fn = {'square': lambda: SquareLoss(**kw), 'abs': lambda: AbsLoss(**kw),
          'huber': lambda: HuberLoss(delta=HUBER_DELTA, **kw),
          'poisson': lambda: PoissonLoss(eps=POISSON_EPS, **kw)}[kind]()
    return LAM_F * fn


def tv_term(wrap=True):
    from sph_raytracer_amd.loss import SmoothRegularizer
    return pc.LAM_TV * SmoothRegularizer(weights=pc.TV_WEIGHTS, kind='abs', wrap_a=wrap)


# ---- the proxes ------------------------------------------------------------------------------------
def prox_draws(kind, seed=0, n=400):
    """(a, sigma, s, y): n random draws per kind over several decades, the first few with s = 0,
    then y = 0, then arguments placed on both sides of (and on) every clamp."""
    rng = np.random.default_rng(1000 * KIND_ID[kind] + seed)
    sigma = 10.0 ** rng.uniform(-3, 1, n)
    s = 10.0 ** rng.uniform(-3, 0, n)
    y = rng.standard_normal(n) if kind != 'poisson' else 10.0 ** rng.uniform(-2, 1, n)
    a = rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)
    s[:8] = 0.0
    y[8:24] = 0.0
    # around the clamps: t = a - sigma y at -s b, +s b (b the bound's factor) and a little
    # to either side
    b = {'abs': 1.0, 'huber': HUBER_DELTA}.get(kind)
    if b is not None:
        k = np.arange(24, 84)
        scale = (1.0 + sigma[k] / s[k]) if kind == 'huber' else 1.0
        side = np.tile([-1.0, 1.0], 30)
        off = np.repeat([0.0, 1e-3, -1e-3, 0.5, -0.5, 2.0], 10)
        a[k] = sigma[k] * y[k] + side * s[k] * b * scale * (1.0 + off)
    if kind == 'poisson':            # far to either side of s, where the root cancels
        k = np.arange(24, 64)
        a[k] = s[k] * np.tile([30.0, -30.0, 1.0, 1e3], 10)
    return a, sigma, s, y


def prox_violation(kind, a, sigma, s, y, p):
    """How far p is from d phi(z) at z = (a - p) / sigma, relative to the size of the operands:
    abs inside the clamp |z - y| (z must be y), on it the wrong-signed part of z - y; the other
    kinds |p - phi'(z)|.  s = 0 rows must be +0.0 exactly (violation inf otherwise)."""
    par = par_of(kind)
    with np.errstate(all='ignore'):
        z = (a - p) / sigma
        r = z - y
        zs = (np.abs(a) + np.abs(p)) / sigma + np.abs(y)       # the size of z - y's operands
        ps = np.abs(a) + sigma * np.abs(y) + s                 # the size of p's operands
        if kind == 'abs':
            inside = np.abs(p) < s
            v = np.where(inside, np.abs(r) / zs, np.maximum(0.0, -np.sign(p) * r) / zs)
            v = np.where(np.abs(p) > s, np.inf, v)
        elif kind == 'huber':
            v = np.abs(p - s * np.clip(r, -par, par)) / ps
            v = np.where(np.abs(p) > s * par, np.inf, v)
        elif kind == 'square':
            v = np.abs(p - 2 * s * r) / ps
        else:
            v = np.abs(p - s * (1 - y / (z + par))) / ps
            # y = 0: phi = s z on z + eps >= 0, whose subdifferential is s inside and
            # (-inf, s] at the end z = -eps
            # (either reading may hold to rounding: the smaller of the two)
            end = np.minimum(np.abs(z + par) / zs,
                             np.where(z + par >= 0, np.abs(p - s) / ps, np.inf))
            v = np.where(y == 0, end, v)
            v = np.where(p > s, np.inf, v)
    zero = s == 0
    ok = (p[zero] == 0) & ~np.signbit(p[zero])
    v = v.copy()
    v[zero] = np.where(ok, 0.0, np.inf)
    return v


# the largest violation retrieval._cp_prox shows on prox_draws(kind), float64, CPU
PROX_MEASURED = {'square': 5.34e-14, 'abs': 1.01e-16, 'huber': 3.85e-15, 'poisson': 2.99e-09}
PROX_BOUND = {k: 16 * v for k, v in PROX_MEASURED.items()}


# ---- the launch, op by op --------------------------------------------------------------------------
def fma_exact(a, b, c):
    """fma(a, b, c) on float64 torch tensors through exact rationals on the host (loop_cases.fma:
    one rounding, IEEE special values): for small lengths and the special-value cases."""
    import torch as tr

    import loop_cases as lc
    a, b, c = tr.broadcast_tensors(a, b, c)
    an, bn, cn = (v.cpu().numpy().reshape(-1) for v in (a, b, c))
    flat = np.array([lc.fma(float(u), float(v), float(w)) for u, v, w in zip(an, bn, cn)])
    return tr.from_numpy(flat).reshape(c.shape).to(c.device)


def fma_eft(a, b, c):
    """fma(a, b, c) by error-free transformations in float64 elementwise torch ops, on the
    tensors' device: a * b = hi + lo exactly (Veltkamp split, Dekker product), hi + c = s + e
    exactly (Knuth two-sum), then s + (e + lo).  One rounding unless the exact sum lies within
    2^-106 |s| of a rounding tie (a chance of 2^-52 per element) — for finite operands whose
    products neither overflow nor fall under 2^-968: the random cases.  test_cp_cpu.py holds it
    to fma_exact on a sample."""
    def split(v):
        t_ = v * 134217729.0          # 2^27 + 1
        h = t_ - (t_ - v)
        return h, v - h
    hi = a * b
    ah, al = split(a)
    bh, bl = split(b)
    lo = ((ah * bh - hi) + ah * bl + al * bh) + al * bl
    s_ = hi + c
    bb = s_ - hi
    e = (hi - (s_ - bb)) + (c - bb)
    return s_ + (e + lo)


def ray_dual_ref(kind, z_new, z_old, y, s, w, sigma, p, order=None, fma=None):
    """sphrt_cp_ray_dual_f64 restated in torch on the tensors' device, in the header's order ->
    (p_new, p_adj or None, the terms of part_pp, the terms of part_fid), the terms per thread j.
    `fma`: the fused multiply-add to use (default fma_eft, on the device; fma_exact for special
    values); every other operation is torch's elementwise one on the device."""
    import torch as tr
    fma = fma or fma_eft
    par = par_of(kind)
    idx = order.long() if order is not None else tr.arange(len(p), device=p.device)
    zn, zo, m, sv, wv, po = (v[idx] for v in (z_new, z_old, y.to(tr.float64), s, w, p))
    sg = tr.full_like(po, float(sigma))
    two = tr.full_like(po, 2.0)
    zb = fma(two, zn, -zo)
    a = fma(sg, zb, po)
    tt = fma(-sg, m, a)
    r = zn - m
    if kind == 'square':
        pn = tt / (1.0 + sg / (2.0 * sv))
        h = r * r
    elif kind == 'abs':
        pn = tr.where(tt < -sv, -sv, tr.where(tt > sv, sv, tt))
        h = r.abs()
    elif kind == 'huber':
        u, b = tt / (1.0 + sg / sv), sv * par
        pn = tr.where(u < -b, -b, tr.where(u > b, b, u))
        zz = r.abs()
        h = tr.where(zz < par, (0.5 * zz) * zz, par * (zz - 0.5 * par))
    else:
        a1 = fma(sg, tr.full_like(po, par), a)
        d, e = a1 - sv, a1 + sv
        disc = fma((4.0 * sg) * sv, m, d * d)
        v = 0.5 * (e - tr.sqrt(disc))
        pn = tr.where(v > sv, sv, v)
        h = zn - m * tr.log(zn + par)
    pn = tr.where(sv == 0, tr.zeros_like(pn), pn)
    p_new = p.clone()
    p_new[idx] = pn
    dp = pn - po
    return p_new, (pn.clone() if order is not None else None), dp * dp, wv * h


# ---- the solver's problems ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(name, reverse=False):
    """(CpuOperator, y >= 0, mask, dense A) of 'tiny' / 'two_workgroups': test_pd_cpu's problems,
    the measurements clamped at 0 (counts), the matrix column by column from the oracle."""
    import torch as tr
    from cpu_operator import CpuOperator
    from test_pd_cpu import _operator
    op, y, mask = _operator(name)
    if reverse:
        op = CpuOperator(op.grid, op.geom, reverse=True)
    shape = tuple(op.grid.shape)
    # counts: none below zero, and none on a ray that misses the grid (its integral is 0 whatever
    # x is; a positive count there would leave the Poisson term's dual at -s y / eps, which no
    # iteration count of a test reaches)
    seen = op(tr.ones(shape, dtype=tr.float64)) > 0
    y = tr.where(seen, y.clamp(min=0.0), tr.zeros_like(y))
    cols = []
    for i in range(math.prod(shape)):
        e = tr.zeros(shape, dtype=tr.float64)
        e.view(-1)[i] = 1.0
        cols.append(op(e).reshape(-1))
    return op, y, mask, tr.stack(cols, dim=1).numpy()


def terms(kind, tv, mask=1):
    return [fidelity(kind, mask)] + ([tv_term()] if tv else [])


# (problem, kind, tv, masked, damp, lower, upper): each kind with and without TV; without mask
# and damp, with both, with lower = 0 and no upper bound (damped: the dual value stays finite);
# and the two-workgroup problem once per kind and TV
def solver_cases():
    out = []
    for kind in KINDS:
        for tv in (False, True):
            out += [('tiny', kind, tv, False, 0.0, LOWER, UPPER),
                    ('tiny', kind, tv, True, DAMP, LOWER, UPPER),
                    ('tiny', kind, tv, True, DAMP, 0.0, None),
                    ('two_workgroups', kind, tv, True, DAMP, LOWER, UPPER)]
    return out


def case_id(case):
    name, kind, tv, masked, damp, lower, upper = case
    return (f'{name}-{kind}-{"tv" if tv else "notv"}-{"masked" if masked else "unit"}-'
            f'{"damp" if damp else "nodamp"}-{"box" if upper is not None else "lower0"}')


def ray_factors(y, mask, masked):
    """(s, w) per ray as float64 numpy vectors."""
    m = y.numel()
    w = mask.numpy().reshape(-1) if masked else np.ones(m)
    return LAM_F / m * w, w


def phi(kind, s, y, z):
    par = par_of(kind)
    r = z - y
    if kind == 'square':
        return s * r * r
    if kind == 'abs':
        return s * np.abs(r)
    if kind == 'huber':
        zz = np.abs(r)
        return s * np.where(zz < par, 0.5 * zz * zz, par * (zz - 0.5 * par))
    with np.errstate(all='ignore'):
        return s * (z - y * np.log(z + par))


def phi_conj(kind, s, y, p):
    """phi_i*(p_i), +inf outside its domain; s = 0 rows: 0 at p = 0."""
    par = par_of(kind)
    with np.errstate(all='ignore'):
        if kind == 'square':
            v = y * p + np.where(s > 0, p * p / (4 * s), 0.0)
            dom = (s > 0) | (p == 0)
        elif kind == 'abs':
            v, dom = y * p, np.abs(p) <= s
        elif kind == 'huber':
            v = y * p + np.where(s > 0, p * p / (2 * s), 0.0)
            dom = np.abs(p) <= s * par
        else:
            # sup_z p z - s (z - y log(z + eps)) = -s y + (s - p) eps + s y log(s y / (s - p))
            sy = s * y
            lg = np.where(sy > 0, sy * np.log(sy / (s - p)), 0.0)
            v = -sy + (s - p) * par + lg
            dom = (p < s) | ((p == s) & (sy == 0))
    return np.where(dom, v, np.inf)


def tv_edges(shape, tv):
    """(D, c per edge, up) of the TV term on a volume of `shape` (ring closed), or None."""
    if not tv:
        return None
    D, axis, _ = pc.tv_matrix(shape, True, pc.TV_WEIGHTS)
    c = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS)[axis] / math.prod(shape)
    _, up = pc.neighbours(shape, True, (1, 1, 1))
    return D, c, up


def flat_dual(q, up):
    qn = q.detach().cpu().numpy().reshape(3, -1)
    return np.concatenate([qn[ax][up[ax] >= 0] for ax in range(3)])


def primal_value(kind, A, s, y, edges, damp, x):
    val = phi(kind, s, y, A @ x).sum() + damp * np.mean(x * x)
    if edges is not None:
        val += (edges[1] * np.abs(edges[0] @ x)).sum()
    return float(val)


def dual_value(kind, A, s, y, edges, damp, lower, upper, p, q):
    """D(p, q) = -sum phi*(p) + sum_j min over the box of c/2 x^2 + x v_j, v = A^T p + D^T q."""
    v = A.T @ p
    if edges is not None:
        v = v + edges[0].T @ q
    c = 2 * damp / len(v)
    lo = -math.inf if lower is None else lower
    hi = math.inf if upper is None else upper
    with np.errstate(all='ignore'):
        if c > 0:
            xs = np.clip(-v / c, lo, hi)
        else:
            xs = np.where(v > 0, lo, np.where(v < 0, hi, 0.0))
        box = np.where(v == 0, 0.0, xs * v) + 0.5 * c * np.where(np.isinf(xs), 0.0, xs) ** 2
    return float(-phi_conj(kind, s, y, p).sum() + box.sum())


def rounded32(y):
    """y rounded to float32 and back: what a float32 y is promoted to, exactly."""
    return y.float().double()


def gap_of(case, x, info, y32=False):
    """(J(x), D(p, q), the relative gap (J - D) / |J|) of a solve of `case`, recomputed from the
    dense matrix without the solver (y32: for the measurements rounded to float32)."""
    name, kind, tv, masked, damp, lower, upper = case
    op, y, mask, A = problem(name)
    y = rounded32(y) if y32 else y
    s, _ = ray_factors(y, mask, masked)
    edges = tv_edges(tuple(op.grid.shape), tv)
    xn = x.detach().cpu().numpy().reshape(-1).astype(np.float64)
    p = info['ray_dual'].detach().cpu().numpy().reshape(-1).astype(np.float64)
    q = flat_dual(info['dual'], edges[2]) if tv else None
    yn = y.numpy().reshape(-1)
    J = primal_value(kind, A, s, yn, edges, damp, xn)
    Dv = dual_value(kind, A, s, yn, edges, damp, lower, upper, p, q)
    return J, Dv, (J - Dv) / abs(J)


def solve_case(case, run=None, reverse=False, iterations=None, y32=False, **kw):
    """chambolle_pock (the generic path: CPU tensors) on a case -> (x, y_hat, info); y32: on the
    measurements rounded to float32 (as float64: the values a float32 y is promoted to)."""
    from sph_raytracer_amd.retrieval import chambolle_pock
    name, kind, tv, masked, damp, lower, upper = case
    op, y, mask, _ = problem(name, reverse)
    y = rounded32(y) if y32 else y
    return (run or chambolle_pock)(op, y, terms(kind, tv, mask if masked else 1), damp=damp,
                                   lower=lower, upper=upper,
                                   num_iterations=iterations or ITERATIONS, **kw)


# the rounding slack of weak duality D <= J: both are sums of at most ~600 terms of size |J|
WEAK_DUALITY_SLACK = 1e-13

ITERATIONS = 3000
# case id -> the relative gap after ITERATIONS iterations (tools/cp_study.py)
MEASURED = {
    'tiny-square-notv-unit-nodamp-box': 6.17e-15,
    'tiny-square-notv-masked-damp-box': 0,
    'tiny-square-notv-masked-damp-lower0': 3.31e-16,
    'two_workgroups-square-notv-masked-damp-box': 1.7e-16,
    'tiny-square-tv-unit-nodamp-box': 2.27e-14,
    'tiny-square-tv-masked-damp-box': 0,
    'tiny-square-tv-masked-damp-lower0': 0,
    'two_workgroups-square-tv-masked-damp-box': 0,
    'tiny-abs-notv-unit-nodamp-box': 0.000605,
    'tiny-abs-notv-masked-damp-box': 1.72e-05,
    'tiny-abs-notv-masked-damp-lower0': 1.72e-15,
    'two_workgroups-abs-notv-masked-damp-box': 2.16e-05,
    'tiny-abs-tv-unit-nodamp-box': 0.00196,
    'tiny-abs-tv-masked-damp-box': 2.16e-13,
    'tiny-abs-tv-masked-damp-lower0': 3.6e-11,
    'two_workgroups-abs-tv-masked-damp-box': 0.000261,
    'tiny-huber-notv-unit-nodamp-box': 1.82e-09,
    'tiny-huber-notv-masked-damp-box': -1.62e-16,
    'tiny-huber-notv-masked-damp-lower0': 2.06e-16,
    'two_workgroups-huber-notv-masked-damp-box': 1.94e-16,
    'tiny-huber-tv-unit-nodamp-box': 7.2e-15,
    'tiny-huber-tv-masked-damp-box': 0,
    'tiny-huber-tv-masked-damp-lower0': 1.55e-16,
    'two_workgroups-huber-tv-masked-damp-box': -1.5e-16,
    'tiny-poisson-notv-unit-nodamp-box': 1.37e-08,
    'tiny-poisson-notv-masked-damp-box': 1.44e-08,
    'tiny-poisson-notv-masked-damp-lower0': 1.45e-08,
    'two_workgroups-poisson-notv-masked-damp-box': 9.67e-09,
    'tiny-poisson-tv-unit-nodamp-box': 1.36e-08,
    'tiny-poisson-tv-masked-damp-box': 1.43e-08,
    'tiny-poisson-tv-masked-damp-lower0': 1.44e-08,
    'two_workgroups-poisson-tv-masked-damp-box': 9.6e-09,
}
# What the recomputation of J and D itself resolves: each is a sum of up to ~700 terms of the size
# of J, so their difference carries ~700 * 2^-53 ~ 1e-13 |J| of rounding; two decades above it.
GAP_FLOOR = 1e-11
# per kind: 100 x the largest gap of the kind's cases above, rounded up in the third digit, at
# least GAP_FLOOR (no kind's limit is looser than 100 x the largest gap of all: 0.196)
GAP_LIMIT = {'square': 1e-11, 'abs': 0.196, 'huber': 1.82e-07, 'poisson': 1.45e-06}

# ---- the GPU configurations and the CPU reference's sensitivity ----------------------------------------
SENS_ITERATIONS = ITERATIONS


def gpu_cases():
    """(problem, kind, tv, masked): every kind with and without TV on the tiny problem, masked
    and not; the two-workgroup problem masked with TV."""
    out = []
    for kind in KINDS:
        out += [('tiny', kind, False, False), ('tiny', kind, True, True),
                ('two_workgroups', kind, True, True)]
    return out


def gpu_case(cfg):
    name, kind, tv, masked = cfg
    return (name, kind, tv, masked, DAMP, LOWER, UPPER)


def sensitivity(cfg):
    """max |x - x'|, max |p - p'|, max |q - q'| between the CPU reference and the same solve over
    the matrix with its sums reversed, after SENS_ITERATIONS iterations."""
    a = solve_case(gpu_case(cfg), iterations=SENS_ITERATIONS)
    b = solve_case(gpu_case(cfg), iterations=SENS_ITERATIONS, reverse=True)
    d = [float((a[0] - b[0]).abs().max()),
         float((a[2]['ray_dual'] - b[2]['ray_dual']).abs().max())]
    d.append(float((a[2]['dual'] - b[2]['dual']).abs().max()) if cfg[2] else 0.0)
    return tuple(d)


# cfg -> (d_x, d_p, d_q) (tools/cp_study.py --sensitivity)
SENSITIVITY = {
    ('tiny', 'square', False, False): (6.11e-16, 6.72e-18, 0.00e+00),
    ('tiny', 'square', True, True): (1.67e-16, 5.42e-18, 4.34e-18),
    ('two_workgroups', 'square', True, True): (8.88e-16, 3.58e-18, 1.35e-18),
    ('tiny', 'abs', False, False): (1.78e-15, 1.14e-16, 0.00e+00),
    ('tiny', 'abs', True, True): (3.33e-16, 5.64e-18, 4.12e-18),
    ('two_workgroups', 'abs', True, True): (1.11e-15, 5.49e-17, 1.51e-18),
    ('tiny', 'huber', False, False): (2.22e-16, 2.17e-18, 0.00e+00),
    ('tiny', 'huber', True, True): (0.00e+00, 0.00e+00, 8.40e-19),
    ('two_workgroups', 'huber', True, True): (3.33e-16, 1.65e-18, 6.23e-19),
    ('tiny', 'poisson', False, False): (6.66e-16, 6.94e-18, 0.00e+00),
    ('tiny', 'poisson', True, True): (1.67e-16, 6.94e-18, 8.24e-18),
    ('two_workgroups', 'poisson', True, True): (5.55e-16, 5.20e-18, 1.44e-18),
}
FACTOR, FLOOR = 16.0, 1e-13        # gd_cases' rule: 16 x d, at least 1e-13 of the largest magnitude


def bounds(cfg, x, p, q):
    """The bounds the GPU tests hold for x, p and q against the CPU reference (x, p, q: the
    reference's tensors, q None without TV): FACTOR x the committed sensitivity, at least FLOOR x
    the reference's largest magnitude of that quantity."""
    d = SENSITIVITY[cfg]
    ref = (x, p, q)
    return tuple(max(FACTOR * dk, FLOOR * float(v.abs().max())) if v is not None else 0.0
                 for dk, v in zip(d, ref))
