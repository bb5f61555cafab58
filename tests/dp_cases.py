"""Cases and CPU restatements for the diagonally preconditioned Chambolle-Pock iteration
(retrieval.chambolle_pock(precondition='diagonal'); csrc/loss.hip: sphrt_dp_primal_f64,
sphrt_dp_ray_dual_f64, sphrt_dp_steps_f64, declared in include/sphrt_dp.h) — no tests here; numpy
and torch on the CPU (or on the tensors' device), no library call.  The edge rules, the exact fma
and the partial-sum order are pd_cases', cp_cases' and cg_cases'; the solver's problems, its
duality-gap recomputation and every bound are cp_cases' own, unchanged.

  kernels   SIZES (one element, around one workgroup, and 1024 * 256 + 257: past one element per
            thread) and VOLUMES (one voxel, the ring of two, one axis, small odd shapes with the
            ring open and closed) with every has_* mask; each entry restated op by op with
            per-element steps (`primal_ref`, `ray_dual_ref`, `steps_ref`; `degree` counts the
            edges at a voxel from pd_cases.neighbours, not from index arithmetic);
  lemma     `dense_k` stacks the oracle's dense A over pd_cases' dense D, `dense_steps` forms the
            steps in numpy: what the SVD and eigenvalue checks of test_dp_cpu.py run on;
  solver    cp_cases.solver_cases() at ITERATIONS iterations (chosen on the CPU: see below), held
            to cp_cases.GAP_LIMIT.
"""
import contextlib
import math

import numpy as np

import cg_cases as cc
import cp_cases as cp
import pd_cases as pc

# 1, around one workgroup, and one past 1024 workgroups x 256 threads plus a partial workgroup
SIZES = [1, 255, 256, 257, 1024 * 256 + 257]
# (shape, [wrap_a ...])
VOLUMES = [((1, 1, 1), [False]), ((1, 1, 2), [True]), ((2, 1, 1), [False]), ((3, 2, 2), [True]),
           ((5, 4, 7), [False, True])]
HAS = [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, 0)]
# volumes whose voxel counts are SIZES (the primal entry takes a volume, not a length)
SIZE_VOLUMES = {1: (1, 1, 1), 255: (5, 3, 17), 256: (4, 8, 8), 257: (1, 257, 1),
                1024 * 256 + 257: (3, 47, 1861)}
assert all(math.prod(v) == n for n, v in SIZE_VOLUMES.items()) and sorted(SIZE_VOLUMES) == SIZES


def volume_cases():
    return [(shape, w, h) for shape, wraps in VOLUMES for w in wraps for h in HAS]


def volume_id(case):
    shape, w, h = case
    return f'{"x".join(map(str, shape))}-{"ring" if w else "open"}-{"".join(map(str, h))}'


# ---- the steps -----------------------------------------------------------------------------------------
def degree(shape, wrap, has):
    """deg_j by brute force: the edges of pd_cases.neighbours that arrive at or leave voxel j."""
    lo, up = pc.neighbours(shape, wrap, has)
    return ((lo >= 0).sum(axis=0) + (up >= 0).sum(axis=0)).astype(np.float64)


def steps_ref(col, row, shape, wrap, has, rho, c, order=None):
    """sphrt_dp_steps_f64 -> (tau, sigma) in numpy; the fma rounded once through rationals on up
    to 600 voxels and wherever col is not an ordinary number, by cp_cases.fma_eft elsewhere."""
    import torch as tr
    col = np.asarray(col, dtype=np.float64)
    t_ = col + degree(shape, wrap, has)
    with np.errstate(all='ignore'):
        d = cp.fma_eft(tr.full((len(col),), float(rho), dtype=tr.float64), tr.from_numpy(t_),
                       tr.full((len(col),), float(c), dtype=tr.float64)).numpy()
        odd = ~np.isfinite(col) | (np.abs(col) < 1e-300)
        if len(col) <= 600:
            odd[:] = True
        for j in np.flatnonzero(odd):
            d[j] = cc.fma(rho, t_[j], c)
        tau = np.where(d > 0, 1.0 / d, 0.0)
        r = np.asarray(row)[order] if order is not None else np.asarray(row)
        sigma = np.where(r > 0, rho / r, 0.0)
    return tau, sigma


def steps_inputs(n_vox, n_ray, seed):
    """(col, row): positive sums over several decades, with zeros, a negative, -0.0, NaN, inf and
    a denormal planted where the lengths allow (the guards' cases)."""
    rng = np.random.default_rng(seed)
    col = 10.0 ** rng.uniform(-3, 2, n_vox)
    row = 10.0 ** rng.uniform(-3, 2, n_ray)
    plant = [0.0, -0.0, -1.5, np.nan, np.inf, 5e-324, -np.inf]
    for v, k in ((col, 3), (row, 5)):
        for j, val in enumerate(plant):
            i = (k + 7 * j) % len(v)
            if len(v) > len(plant):
                v[i] = val
    return col, row


# ---- the primal step -----------------------------------------------------------------------------------
def primal_ref(x, g, q, tau, shape, wrap, has, c_damp, lower, upper, fma=None):
    """sphrt_dp_primal_f64 on float64 torch tensors (x, g, tau: n; q: (3, n)), in the header's
    order -> (x_new, the terms of part_mm).  D^T q is pd_cases.adjoint_sum (numpy: the same IEEE
    adds in the same order); `fma` as cp_cases.ray_dual_ref takes it."""
    import torch as tr
    fma = fma or cp.fma_eft
    lo, up = pc.neighbours(shape, wrap, has)
    s = tr.from_numpy(pc.adjoint_sum(q.cpu().numpy(), lo, up)).to(x.device)
    gp = fma(tr.full_like(x, c_damp), x, g)
    u = fma(-tau, gp + s, x)
    lo_t, hi_t = tr.full_like(x, lower), tr.full_like(x, upper)
    xn = tr.where(u < lo_t, lo_t, tr.where(u > hi_t, hi_t, u))
    d = xn - x
    return xn, d * d


# ---- the ray dual --------------------------------------------------------------------------------------
def ray_dual_ref(kind, z_new, z_old, y, s, w, sigma, p, order=None, fma=None):
    """sphrt_dp_ray_dual_f64 restated in torch on the tensors' device: cp_cases.ray_dual_ref with
    sg = sigma[i] per ray, i = order[j] -> (p_new, p_adj or None, the terms of part_pp, the terms
    of part_fid), the terms per thread j."""
    import torch as tr
    fma = fma or cp.fma_eft
    par = cp.par_of(kind)
    idx = order.long() if order is not None else tr.arange(len(p), device=p.device)
    zn, zo, m, sv, wv, po, sg = (v[idx] for v in (z_new, z_old, y.to(tr.float64), s, w, p, sigma))
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


# ---- the lemma on dense systems --------------------------------------------------------------------------
LEMMA_SHAPE = (6, 4, 6)
LEMMA_RHO = [1.5 / 72, 1e-4, 30.0]       # rho cancels from the norm: several decades of it
LEMMA_DAMP = [0.0, 0.05]


def lemma_problem():
    """(CpuOperator, dense A) on a 6 x 4 x 6 grid: two small detectors whose fields of view leave
    voxels no ray crosses and rays that miss the grid."""
    import torch as tr
    from cpu_operator import CpuOperator
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    grid = SphericalGrid(shape=LEMMA_SHAPE)
    geom = ConeRectGeom((5, 5), pos=(5, 0.3, 1), fov=(35, 35)) + \
        ConeRectGeom((5, 5), pos=(-1, 4.5, -2), fov=(35, 35))
    op = CpuOperator(grid, geom)
    cols = []
    for i in range(math.prod(LEMMA_SHAPE)):
        e = tr.zeros(LEMMA_SHAPE, dtype=tr.float64)
        e.view(-1)[i] = 1.0
        cols.append(op(e).reshape(-1))
    return op, tr.stack(cols, dim=1).numpy()


def dense_k(A, shape, wrap, tv):
    """(K = [A; D], the number of rows of A): D pd_cases' dense forward difference (unweighted
    entries +-1) over the axes pd_cases.TV_WEIGHTS gives edges, or nothing without TV."""
    if not tv:
        return A, len(A)
    D, _, _ = pc.tv_matrix(shape, wrap, pc.TV_WEIGHTS)
    return np.vstack([A, D]), len(A)


def dense_steps(K, n_ray, rho, c):
    """(tau per column, sigma per row of K) from |K|'s sums in numpy: the issue's formulas."""
    row, col = np.abs(K).sum(axis=1), np.abs(K).sum(axis=0)
    with np.errstate(all='ignore'):
        sigma = np.where(row > 0, rho / row, 0.0)
        d = rho * col + c
        tau = np.where(d > 0, 1.0 / d, 0.0)
    return tau, sigma


# ---- the solver ------------------------------------------------------------------------------------------
# The iteration count of the solver tests, chosen on the CPU: at 3000 (cp_cases.ITERATIONS) every
# case of cp_cases.solver_cases() is under cp_cases.GAP_LIMIT, the closest being
# tiny-square-tv-unit-nodamp-box at 8.3e-12 of a limit of 1e-11; at 4000 that case is at 6.6e-15.
ITERATIONS = 4000


def solve_case(case, **kw):
    return cp.solve_case(case, iterations=kw.pop('iterations', ITERATIONS),
                         precondition='diagonal', **kw)


# precondition=None must stay bit for bit what the parent commit computed: x and the duals of
# these cases after GOLDEN_ITERATIONS iterations of the generic path, recorded from this
# repository's own run of that commit into tests/golden/dp_none_bits.npz (`golden_arrays` is what
# was run; no reference code is involved).
# A limitation, stated: recorded bits can be held across hosts only for operations whose result
# IEEE 754 fixes.  torch documents no correct rounding for its CPU sqrt and log kernels, and
# their float64 bits do vary with the host's CPU under one torch build, whereas +, -, *, / and
# the compares do not.  So the record is taken, and compared, with torch.sqrt standing on
# numpy's (the hardware instruction, correctly rounded) — `golden_arrays` asserts that the
# solver's square roots did go through it — and without the Poisson kind's 'fidelity' history,
# the one quantity torch.log feeds (it enters no iterate).  What the check shows is therefore
# "None runs the parent's sequence of operations, every IEEE one to the bit", not the bits of
# torch's own sqrt on the recording host.
GOLDEN_ITERATIONS = 200
GOLDEN_CASES = [c for c in cp.solver_cases() if c[0] == 'tiny' and c[3] and c[5] == cp.LOWER]
GOLDEN_FILE = 'dp_none_bits.npz'
GOLDEN_HISTORIES = ('primal_change', 'dual_change', 'ray_dual_change', 'fidelity')


@contextlib.contextmanager
def ieee_sqrt():
    """torch.sqrt replaced by numpy's on CPU tensors for the duration -> a one-element list
    counting its calls."""
    import torch as tr
    keep, calls = tr.sqrt, [0]

    def sqrt(v):
        calls[0] += 1
        with np.errstate(all='ignore'):
            return tr.from_numpy(np.sqrt(v.detach().numpy())).reshape(v.shape)
    tr.sqrt = sqrt
    try:
        yield calls
    finally:
        tr.sqrt = keep


def golden_arrays(**kw):
    """{case id + '/x' | '/p' | '/q' | '/hist': array} of chambolle_pock on GOLDEN_CASES (the
    generic path on the CPU under `ieee_sqrt`; kw: further keywords of the solve)."""
    out = {}
    for case in GOLDEN_CASES:
        with ieee_sqrt() as calls:
            x, _, info = cp.solve_case(case, iterations=GOLDEN_ITERATIONS, **kw)
        # (the scalar steps take one square root; the Poisson prox one per iteration)
        if kw.get('precondition') is None:
            assert calls[0] >= (GOLDEN_ITERATIONS if case[1] == 'poisson' else 1), calls
        key = cp.case_id(case)
        out[key + '/x'] = x.numpy()
        out[key + '/p'] = info['ray_dual'].numpy()
        if case[2]:
            out[key + '/q'] = info['dual'].numpy()
        keys = GOLDEN_HISTORIES[:3] if case[1] == 'poisson' else GOLDEN_HISTORIES
        out[key + '/hist'] = np.array([info[k] for k in keys])
    return out


# The generic paths the record above does not reach — `primal_dual` with either TV term,
# `chambolle_pock` with the iso term and with precondition='diagonal' — recorded the same way
# (this repository's own run, under `ieee_sqrt`, without the Poisson kind's fidelity history) from
# the commit before the TV term's plumbing was folded into one description, one pair of generic
# maps and one direct stage: tests/golden/tv_paths_bits.npz.  The inputs hold nothing a host's
# libraries decide: the problems are test_pd_cpu's and cp_cases' 'tiny' ones, the damping is the
# constant cp_cases.DAMP (not the eigenvalue-derived one of the certificate tests).
TV_GOLDEN_FILE = 'tv_paths_bits.npz'
TV_GOLDEN_CASES = [c for c in cp.solver_cases() if c[0] == 'tiny']
# (masked, the square smooth term's wrap_a) of pd_cases.VARIANTS: the smallest problem without a
# smooth term and the TV ring closed, and with one and the ring open
TV_GOLDEN_VARIANTS = [pc.VARIANTS[0], pc.VARIANTS[3]]


def tv_golden_arrays():
    """{path + case id + '/x' | '/q' | '/p' | '/hist' | '/steps' | '/tau' | '/sigma': array} of the
    generic paths on the CPU under `ieee_sqrt`, GOLDEN_ITERATIONS iterations each: 'pd-abs-' and
    'pd-iso-' (`primal_dual` on TV_GOLDEN_VARIANTS), 'cp-iso-' (`chambolle_pock` with the iso term
    on the TV cases of TV_GOLDEN_CASES) and 'cp-diag-' (precondition='diagonal' on all of them)."""
    import iso_cases as ic
    from sph_raytracer_amd.retrieval import primal_dual
    from test_pd_cpu import _operator, quadratic_terms, tv_term
    out = {}
    op, y, mask = _operator('tiny')
    for masked, wrap in TV_GOLDEN_VARIANTS:
        for name, tv in (('abs', tv_term(masked)), ('iso', ic.tv_term(pc.tv_wrap(masked)))):
            with ieee_sqrt() as calls:
                x, _, info = primal_dual(op, y, quadratic_terms(mask, masked, wrap) + [tv],
                                         damp=cp.DAMP, lower=pc.LOWER, upper=pc.UPPER,
                                         num_iterations=GOLDEN_ITERATIONS)
            # (the ball projection takes one square root per iteration, the clamp none)
            assert calls[0] >= GOLDEN_ITERATIONS if name == 'iso' else calls[0] == 0, calls
            key = f'pd-{name}-{"masked" if masked else "unit"}-{wrap}'
            out[key + '/x'], out[key + '/q'] = x.numpy(), info['dual'].numpy()
            out[key + '/hist'] = np.array([info[k] for k in GOLDEN_HISTORIES[:2]])
            out[key + '/steps'] = np.array([info[k] for k in ('lipschitz', 'tau', 'sigma')])
    for case in TV_GOLDEN_CASES:
        keys = GOLDEN_HISTORIES[:3] if case[1] == 'poisson' else GOLDEN_HISTORIES
        runs = [('cp-diag-', lambda: solve_case(case, iterations=GOLDEN_ITERATIONS))]
        if case[2]:
            runs.append(('cp-iso-', lambda: ic.cp_solve(case, iterations=GOLDEN_ITERATIONS)))
        for path, run in runs:
            with ieee_sqrt() as calls:
                x, _, info = run()
            if path == 'cp-iso-' or case[1] == 'poisson':
                assert calls[0] >= GOLDEN_ITERATIONS, calls
            key = path + cp.case_id(case)
            out[key + '/x'], out[key + '/p'] = x.numpy(), info['ray_dual'].numpy()
            if case[2]:
                out[key + '/q'] = info['dual'].numpy()
            out[key + '/hist'] = np.array([info[k] for k in keys])
            if path == 'cp-diag-':
                out[key + '/tau'], out[key + '/sigma'] = info['tau'].numpy(), info['sigma'].numpy()
                out[key + '/steps'] = np.array([info['sigma_tv']])
            else:
                out[key + '/steps'] = np.array([info[k] for k in ('norm', 'tau', 'sigma')])
    return out
