"""Host side of the bound-constrained solver (retrieval.fista; csrc/loss.hip's two pg entries):
the entries are declared, exported and bound, and their refusals fire on the host; fista_cases
holds what it claims, on the references alone; fista refuses what `cg` refuses and its own bad
arguments; and the generic (plain torch) path over the oracle-backed CpuOperator solves the tiny
problem of test_cg_cpu.py — grid 4 x 3 x 6, two views of 6 x 6 rays — under the bounds 0.35 / 0.65
against the bound-constrained minimiser of the dense system.  (No compute call of the library.)

The share condition (at least 15 % of the voxels on each bound and 15 % free at the minimiser) is
asserted on the two variants without a smooth term; the smooth term pulls the solution towards
its mean, so with it the upper bound holds one to three voxels of 72 whatever the seed: there
both bounds are only asserted to bind."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import fista_cases as fc
import loop_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = tr.float64
VP, I64, DBL = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
ENTRIES = {
    'sphrt_pg_step_f64': [VP, VP, VP, VP, I64, DBL, VP, DBL, DBL, VP, VP, VP],
    'sphrt_pg_momentum_f64': [VP, VP, VP, I64, VP, I64, VP, I64, VP, VP, VP],
}


# ---- the C entries -------------------------------------------------------------------------------------
def test_entries_declared_exported_and_bound():
    from sph_raytracer_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, 'include', 'sphrt.h')).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, argtypes in ENTRIES.items():
        m = re.search(r'int\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr)
        assert m, f'{name} is not declared in include/sphrt.h'
        args = [' '.join(a.split()) for a in m.group(1).split(',')]
        assert len(args) == len(argtypes) and args[-1] == 'void *stream'
        for a, ct in zip(args, argtypes):
            want = VP if '*' in a else I64 if a.startswith('int64_t') else DBL
            assert ct is want, (name, a)
        assert name in _lib.EXPORTED and hasattr(raw, name)
        fn = getattr(_lib.load(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes


def test_refusals_on_the_host():
    """Every refusal returns non-zero with its word in sphrt_last_error before any launch: the
    pointers (small fake addresses) are never dereferenced."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    a, b, c, d, e, f, g, h = (VP(1 << 20 | 4096 * k) for k in range(1, 9))
    nan, inf = float('nan'), float('inf')

    def step(z=a, g=b, xo=c, xn=d, n=300, st=e, lower=0.0, upper=1.0, gd=f, mm=g):
        return lib.sphrt_pg_step_f64(z, g, xo, xn, n, 0.5, st, lower, upper, gd, mm, None)

    def momentum(z=a, xn=b, xo=c, n=300, gd=d, n_part=2, om=e, n_omega=4, j_in=f, j_out=g):
        return lib.sphrt_pg_momentum_f64(z, xn, xo, n, gd, n_part, om, n_omega, j_in, j_out, None)

    cases = [(step, dict(n=0), b'empty'), (step, dict(n=-5), b'empty')]
    cases += [(step, {k: None}, b'null') for k in ('z', 'g', 'xo', 'xn', 'st', 'gd', 'mm')]
    cases += [(step, dict(xn=a), b'alias'), (step, dict(xn=b), b'alias'), (step, dict(xn=c), b'alias'),
              (step, dict(g=a), b'alias'), (step, dict(xo=a), b'alias'), (step, dict(xo=b), b'alias'),
              (step, dict(xn=VP(a.value + 8 * 299)), b'alias'), (step, dict(mm=f), b'alias'),
              (step, dict(gd=VP(d.value + 8)), b'alias'), (step, dict(st=VP(d.value + 16)), b'alias')]
    cases += [(step, dict(lower=nan), b'bound'), (step, dict(upper=nan), b'bound'),
              (step, dict(lower=nan, upper=nan), b'bound'), (step, dict(lower=1.0), b'bound'),
              (step, dict(lower=3.0), b'bound'), (step, dict(lower=inf, upper=inf), b'bound'),
              (step, dict(lower=-inf, upper=-inf), b'bound'), (step, dict(lower=0.0, upper=-0.0), b'bound')]
    cases += [(momentum, dict(n=0), b'empty'), (momentum, dict(n=-(2 ** 40)), b'empty')]
    cases += [(momentum, {k: None}, b'null') for k in ('z', 'xn', 'xo', 'gd', 'om', 'j_in', 'j_out')]
    cases += [(momentum, dict(n_part=k), b'n_part') for k in (0, 1, 3, -2, 1024)]
    cases += [(momentum, dict(n=n, n_part=k), b'n_part')
              for n, k in ((1, 2), (256, 2), (257, 1), (262144, 1023))]
    cases += [(momentum, dict(n_omega=k), b'n_omega') for k in (1, 0, -1)]
    cases += [(momentum, dict(z=b), b'alias'), (momentum, dict(z=c), b'alias'),
              (momentum, dict(xn=c), b'alias'), (momentum, dict(j_out=f), b'alias'),
              (momentum, dict(z=VP(b.value + 8 * 299)), b'alias')]
    for i, (fn, kw, word) in enumerate(cases):
        assert fn(**kw) != 0, (i, fn.__name__, kw)
        assert word in lib.sphrt_last_error(), (i, fn.__name__, kw, lib.sphrt_last_error())


# ---- fista_cases on its own references -------------------------------------------------------------------
def test_exact_cases_are_exact():
    """The integer references equal the float64 expressions (every operation is exact on this
    value set, fused or not); each clamp branch holds a tenth of every length >= 63; the partial
    sums are integers in their unit."""
    for n in lc.LENGTHS:
        z, g, x_old = fc.exact_vectors(n, seed=11 * n)
        assert all(len(v) == n and np.abs(v).max() <= 64 for v in (z, g, x_old))
        for case in fc.EXACT_STEPS:
            c, s, lo, hi = (a / b for a, b in case)
            xn, gd, mm, branch = fc.exact_step(z, g, x_old, *case)
            gp = c * z + g
            u = z - s * gp
            assert np.array_equal(xn, np.where(u < lo, lo, np.where(u > hi, hi, u)))
            assert np.array_equal(gd, cc.block_partials(gp * (xn - x_old)))
            assert np.array_equal(mm, cc.block_partials((z - xn) ** 2))
            unit = 8 * case[0][1] * case[1][1]
            assert np.array_equal(mm * unit ** 2, np.round(mm * unit ** 2))
            if n >= 63:
                for br in (-1, 0, 1):
                    assert (branch == br).sum() >= n / 10, (n, case, br)
        for sign in (1, -1, 0):
            part = fc.gd_partials(n, sign, seed=n + sign)
            assert len(part) == lc.grid_of(n) and np.array_equal(part, np.round(part))
            assert np.sign(cc.kernel_sum(part)) == sign == np.sign(part.sum())
            if len(part) > 1 and sign == 0:
                assert part.any() or n < 300
        for w in fc.EXACT_OMEGA:
            assert np.array_equal(fc.exact_momentum(z, x_old, w), z + w * (z - x_old))
    # a sample through the rational sequence too
    z, g, x_old = fc.exact_vectors(257, seed=1)
    case = fc.EXACT_STEPS[2]
    xn, _, _, _ = fc.exact_step(z, g, x_old, *case)
    for i in cc.sample(257, 0, cap=32):
        assert fc.step_ref(z[i], g[i], x_old[i], *(a / b for a, b in case))[0] == xn[i]
    n_omega = len(fc.EXACT_OMEGA)
    assert [fc.j_ref(1.0, j, n_omega) for j in fc.EXACT_J_IN] == [1, 1, 1, 1]
    assert [fc.j_ref(0.0, j, n_omega) for j in fc.EXACT_J_IN] == [1, 4, 7, 7]


def test_random_cases_tell_fma_from_multiply_add():
    differs = 0
    for n in (257, 262145):
        z, g, x_old = fc.random_vectors(n, seed=n)
        step, lower, upper = fc.random_scalars(n)
        inside = 0
        for i in cc.sample(n, seed=n):
            fused = fc.step_ref(z[i], g[i], x_old[i], 0.3, step, lower, upper)[0]
            plain = fc.step_unfused(z[i], g[i], x_old[i], 0.3, step, lower, upper)
            differs += fused != plain
            inside += lower < fused < upper
            assert abs(fused - plain) <= 4 * np.spacing(abs(z[i]) + abs(g[i]))
        assert 50 < inside < 220                       # (all three branches in the sample)
        for sign in (1, -1):
            part = fc.random_partials(n, seed=n, sign=sign)
            assert np.sign(cc.kernel_sum(part)) == sign and (part > 0).any() and (part < 0).any() \
                or len(part) < 3
    assert differs > 50, differs
    assert any(cc.kernel_sum(fc.random_partials(n, n, 1)) != float(np.sum(fc.random_partials(n, n, 1)))
               for n in lc.LENGTHS[-4:])


def test_special_cases_hold_what_they_claim():
    inf, nan = fc.INF, fc.NAN
    assert math.isnan(fc.clamp_ref(nan, 0.0, 1.0)) and fc.clamp_ref(-inf, 0.0, 1.0) == 0.0
    assert fc.clamp_ref(inf, 0.0, 1.0) == 1.0 and fc.clamp_ref(inf, -inf, inf) == inf
    assert math.copysign(1.0, fc.clamp_ref(-0.0, 0.0, 1.0)) == -1.0      # (-0 < 0 is false)
    for col in range(3):
        vals = [tup[col] for tup in fc.SPECIAL_ELEMENTS]
        assert any(math.isnan(v) for v in vals) and inf in vals and -inf in vals
        assert any(v == 0 and math.copysign(1, v) < 0 for v in vals) and any(0 < abs(v) < 1e-300 for v in vals)
    for (a, b), restart in fc.SPECIAL_GD:
        for part in ((a, b), (b, a)):
            assert (cc.kernel_sum(np.array(part)) > 0) == restart
            assert (fc.j_ref(cc.kernel_sum(np.array(part)), 3, 6) == 1) == restart
    assert any(math.isinf(lo) and math.isinf(hi) for lo, hi in fc.SPECIAL_BOUNDS)
    xn, gd, mm = fc.step_ref(1.0, nan, 1.0, 0.5, 0.25, 0.0, 1.0)
    assert math.isnan(xn) and math.isnan(gd) and math.isnan(mm)


def test_bounded_minimiser_and_fista_dense_on_a_known_problem():
    """A diagonal system's bounded minimiser is the clamped unconstrained one; a coupled one
    satisfies the KKT conditions by construction; without bounds it is N^-1 b; and a
    degenerate problem (a zero gradient on a bound) is refused."""
    d, b = np.array([1.0, 2.0, 4.0, 5.0]), np.array([0.2, 1.0, 8.0, 2.0])
    assert np.array_equal(fc.bounded_minimiser(np.diag(d), b, 0.35, 0.65), [0.35, 0.5, 0.65, 0.4])
    rng = np.random.default_rng(2)
    A = rng.standard_normal((30, 12))
    N, b = A.T @ A / 30 + 0.2 * np.eye(12), rng.standard_normal(12)
    assert np.allclose(fc.bounded_minimiser(N, b, -np.inf, np.inf), np.linalg.solve(N, b), rtol=1e-13)
    want = fc.bounded_minimiser(N, b, -0.3, 0.4)
    assert min(fc.shares(want, -0.3, 0.4)) > 0
    L = float(np.linalg.eigvalsh(N)[-1])
    xs, restarts, mm = fc.fista_dense(N, b, L, -0.3, 0.4, 400)
    assert len(xs) == 401 and len(mm) == 400 and cc.rel_err(xs[-1], want) < 1e-13
    assert all(np.all((x >= -0.3) & (x <= 0.4)) for x in xs) and restarts and min(restarts) >= 1
    with pytest.raises(AssertionError, match='complementarity'):
        fc.bounded_minimiser(np.diag(d), np.array([0.35, 1.0, 8.0, 2.0]), 0.35, 0.65,
                             max_iterations=2000)
    assert fc.first_stays_under([1, 1e-13, 1, 1e-13, 1e-14]) == 3
    assert fc.first_stays_under([1e-13]) == 0 and fc.first_stays_under([1e-13, 1]) is None
    from sph_raytracer_amd.retrieval import _fista_omega
    assert fc.omega_table(50) == _fista_omega(50) and fc.omega_table(3)[:2] == [0.0, 0.0]
    assert len(fc.omega_table(50)) == 51 and \
        abs(fc.omega_table(3)[2] - ((1 + 5 ** 0.5) / 2 - 1) / ((1 + (7 + 2 * 5 ** 0.5) ** 0.5) / 2)) < 1e-15


# ---- fista's refusals ------------------------------------------------------------------------------------
def test_fista_refuses_bad_terms_and_arguments():
    import sph_raytracer_amd as pkg
    from sph_raytracer_amd.loss import (AbsLoss, HuberLoss, NegRegularizer, PoissonLoss,
                                        SmoothRegularizer, SquareLoss)
    from sph_raytracer_amd.retrieval import fista
    assert 'fista' in pkg.__all__ and pkg.fista is fista
    y = tr.zeros(2, 6, 6, dtype=F64)
    ok = SquareLoss
    bad = [([], 'fista needs one SquareLoss'), ([ok(), ok()], 'two'),
           ([ok(), NegRegularizer()], 'NegRegularizer'), ([AbsLoss()], 'AbsLoss'),
           ([HuberLoss(delta=0.5)], 'HuberLoss'), ([PoissonLoss()], 'PoissonLoss'),
           ([ok(), SmoothRegularizer(kind='abs')], "'abs'"),
           ([ok(), SmoothRegularizer(kind='huber', delta=1.0)], "'huber'"),
           ([tr.tensor(2.0) * ok()], 'lam'), ([ok(use_grad=False)], 'use_grad'),
           ([ok(volume_mask=2)], 'volume_mask'), ([ok(projection_mask=2)], 'projection_mask')]
    for fns, word in bad:
        with pytest.raises(ValueError, match=word):
            fista(None, y, loss_fns=fns)          # (refused before the operator is touched)
    nan, inf = float('nan'), float('inf')
    for kw, word in ((dict(damp=-1.0), 'damp'), (dict(damp=nan), 'damp'),
                     (dict(num_iterations=-1), 'num_iterations'),
                     (dict(num_iterations=2.5), 'num_iterations'),
                     (dict(lower=nan), 'lower'), (dict(upper=nan), 'upper'),
                     (dict(lower='0'), 'lower'), (dict(upper=tr.tensor(1.0)), 'upper'),
                     (dict(lower=True), 'lower'),
                     (dict(lower=1.0, upper=1.0), 'lower < upper'),
                     (dict(lower=2.0, upper=1.0), 'lower < upper'),
                     (dict(lower=None, upper=-inf), 'lower < upper'),
                     (dict(lower=inf, upper=None), 'lower < upper'),
                     (dict(lipschitz=0.0), 'lipschitz'), (dict(lipschitz=-1.0), 'lipschitz'),
                     (dict(lipschitz=inf), 'lipschitz'), (dict(lipschitz=nan), 'lipschitz'),
                     (dict(lipschitz=tr.tensor(1.0)), 'lipschitz'),
                     (dict(power_iterations=0), 'power_iterations'),
                     (dict(power_iterations=1.5), 'power_iterations')):
        with pytest.raises(ValueError, match=word):
            fista(None, y, **kw)
    with pytest.raises(ValueError, match='fista needs measurements'):
        fista(None, None)


# ---- the generic path against dense algebra ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operator(name='tiny'):
    from cpu_operator import CpuOperator
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    if name == 'tiny':
        grid = SphericalGrid(shape=(4, 3, 6))
        geom = ConeRectGeom((6, 6), pos=(5, 0.3, 1), fov=(25, 25)) + \
            ConeRectGeom((6, 6), pos=(-1, 4.5, -2), fov=(25, 25))
    else:                                   # the 257-ray problem of test_gpu_cg.py
        grid = SphericalGrid(shape=(5, 6, 10))
        geom = ConeRectGeom((257, 1), pos=(4, 1, 0.5), fov=(50, 1))
    op = CpuOperator(grid, geom)
    g = tr.Generator().manual_seed(11)
    truth = tr.rand(tuple(grid.shape), dtype=F64, generator=g)      # uniform in [0, 1]
    y = op(truth).detach()
    y = y + 0.01 * tr.randn(y.shape, dtype=F64, generator=g)
    mask = tr.rand(y.shape, dtype=F64, generator=g) + 0.25
    mask.view(-1)[3] = 0.0                   # (a masked pixel)
    return op, y, mask


def _terms(name, masked, wrap):
    from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
    mask = _operator(name)[2]
    fns = [1.5 * SquareLoss(projection_mask=mask if masked else 1)]
    if wrap is not None:
        fns.append(0.3 * SmoothRegularizer(weights=(1, 0.5, 2), wrap_a=wrap))
    return fns


VARIANTS = [(False, None), (True, None), (False, True), (True, False)]
BOUNDS = [(fc.LOWER, fc.UPPER), (None, None)]


def _inf(lower, upper):
    return (-math.inf if lower is None else lower, math.inf if upper is None else upper)


@functools.lru_cache(maxsize=None)
def _system(name, masked, wrap):
    """(loss terms, damp, N, b) of a variant, damp from the undamped system."""
    op, y, _ = _operator(name)
    fns, shape = _terms(name, masked, wrap), tuple(op.grid.shape)
    N0, _, _ = cc.dense_system(op, y, fns, 0.0, shape)
    damp = cc.damp_for(N0, math.prod(shape))
    N, b, asym = cc.dense_system(op, y, fns, damp, shape)
    assert asym <= 1e-12 * np.abs(N).max()
    assert cc.condition(N) <= cc.KAPPA_MAX
    return fns, damp, N, b


@functools.lru_cache(maxsize=None)
def _minimiser(name, masked, wrap, lower, upper):
    _, _, N, b = _system(name, masked, wrap)
    return fc.bounded_minimiser(N, b, *_inf(lower, upper))


def test_the_reference_has_both_bounds_binding():
    """A condition on the inputs, on the reference alone."""
    for masked, wrap in VARIANTS:
        lo, hi, free = fc.shares(_minimiser('tiny', masked, wrap, fc.LOWER, fc.UPPER),
                                 fc.LOWER, fc.UPPER)
        if wrap is None:
            assert min(lo, hi, free) >= 0.15, (masked, wrap, lo, hi, free)
        else:
            assert lo > 0 and hi > 0 and free >= 0.15, (masked, wrap, lo, hi, free)


@pytest.mark.parametrize('name', ['tiny', 'two_workgroups'])
def test_recorded_iterations_and_limit(name):
    """fista_cases.ITERATIONS and LIMIT are what fista_dense measures, with L as `fista` itself
    estimates it: every system stays under 1e-12 from ITERATIONS on at the latest, and LIMIT is
    100 times the largest error there (1e-12 at least)."""
    from sph_raytracer_amd import retrieval
    p = retrieval._FISTA_POWER_ITERATIONS
    for masked, wrap in VARIANTS:
        _, _, N, b = _system(name, masked, wrap)
        v = np.ones(len(b))
        for _ in range(p):
            w = N @ v
            rho = (v @ w) / (v @ v)
            v = w / np.linalg.norm(w)
        L = rho * (1 + retrieval._FISTA_MARGIN)
        assert L >= np.linalg.eigvalsh(N)[-1]
        for lower, upper in BOUNDS:
            want = _minimiser(name, masked, wrap, lower, upper)
            xs, restarts, _ = fc.fista_dense(N, b, L, *_inf(lower, upper), fc.ITERATIONS + 300)
            errs = [cc.rel_err(x, want) for x in xs]
            k = fc.first_stays_under(errs)
            key = (name, masked, wrap, lower is not None)
            print(key, k, errs[fc.ITERATIONS])
            assert k is not None and k <= fc.ITERATIONS, key
            assert 100 * errs[fc.ITERATIONS] <= fc.LIMIT and fc.LIMIT >= 1e-12, key
            assert abs(fc.MEASURED[key][0] - k) <= 1, (key, k)     # (as recorded)
            assert restarts, key
    assert max(v[0] for v in fc.MEASURED.values()) == fc.ITERATIONS


@pytest.mark.parametrize('lower,upper', BOUNDS)
@pytest.mark.parametrize('masked,wrap', VARIANTS)
def test_generic_path_reaches_the_bounded_minimiser(masked, wrap, lower, upper):
    from sph_raytracer_amd.retrieval import fista
    op, y, _ = _operator()
    fns, damp, N, b = _system('tiny', masked, wrap)
    want = _minimiser('tiny', masked, wrap, lower, upper)
    x, y_hat, info = fista(op, y, loss_fns=fns, damp=damp, lower=lower, upper=upper,
                           num_iterations=fc.ITERATIONS)
    assert x.shape == tuple(op.grid.shape) and x.dtype == F64 and not x.requires_grad
    assert tr.equal(y_hat, op(x)) and y_hat.shape == y.shape
    err = cc.rel_err(x.numpy(), want)
    print(f'fista tiny masked={masked} wrap={wrap} bounds={lower, upper}: {err:.3g}')
    assert err <= fc.LIMIT
    if lower is None:
        assert cc.rel_err(x.numpy(), np.linalg.solve(N, b)) <= fc.LIMIT
    else:
        xn = x.numpy().reshape(-1)
        assert np.all((xn >= lower) & (xn <= upper))
        assert np.array_equal(xn <= lower, want <= lower) and np.array_equal(xn >= upper, want >= upper)
    res = info['residual']
    assert len(res) == fc.ITERATIONS and res[0] == 1.0 and res[-1] < 1e-10
    assert all(math.isfinite(v) and v >= 0 for v in res)
    assert info['lipschitz'] >= np.linalg.eigvalsh(N)[-1]
    assert info['restarts'] and all(1 <= k < fc.ITERATIONS for k in info['restarts'])
    # a given L is used as it is, and the iterates are those of the dense restatement
    L = 1.25 * float(np.linalg.eigvalsh(N)[-1])
    x12, _, i12 = fista(op, y, loss_fns=fns, damp=damp, lower=lower, upper=upper,
                        num_iterations=12, lipschitz=L)
    xs, restarts, mm = fc.fista_dense(N, b, L, *_inf(lower, upper), 12)
    assert i12['lipschitz'] == L and cc.rel_err(x12.numpy(), xs[-1]) <= 1e-12
    assert i12['restarts'] == restarts
    assert np.allclose(i12['residual'], np.sqrt(np.array(mm) / mm[0]), rtol=1e-9)


def test_every_iterate_is_inside_the_bounds_with_the_bounds_bits():
    from sph_raytracer_amd.retrieval import fista
    op, y, _ = _operator()
    fns, damp, _, _ = _system('tiny', True, True)
    lo_bits, hi_bits = (np.float64(v).view(np.int64) for v in (fc.LOWER, fc.UPPER))
    x0 = tr.linspace(-1, 2, 72, dtype=F64).reshape(4, 3, 6)
    hit = [0, 0]
    for k in range(0, 9):
        x, _, info = fista(op, y, loss_fns=fns, damp=damp, lower=fc.LOWER, upper=fc.UPPER,
                           num_iterations=k, x0=x0)
        xn = x.numpy().reshape(-1)
        assert np.all((xn >= fc.LOWER) & (xn <= fc.UPPER)), k
        bits = xn.view(np.int64)
        assert np.all(bits[xn == fc.LOWER] == lo_bits) and np.all(bits[xn == fc.UPPER] == hi_bits)
        hit[0] += int((xn == fc.LOWER).sum())
        hit[1] += int((xn == fc.UPPER).sum())
        assert len(info['residual']) == k and info['restarts'] == [r for r in info['restarts'] if r < k]
    assert min(hit) > 0 and tr.equal(x0, tr.linspace(-1, 2, 72, dtype=F64).reshape(4, 3, 6))
    # one-sided bounds: the default is x >= 0
    x, _, _ = fista(op, y - 1.0, loss_fns=fns, damp=damp, num_iterations=30)
    assert float(x.min()) == 0.0 and bool((x == 0).any())
    x, _, _ = fista(op, y, loss_fns=fns, damp=damp, lower=None, upper=0.4, num_iterations=30)
    assert float(x.max()) == 0.4


def test_zero_measurements_and_other_starts():
    """b = 0 with 0 inside the bounds: nothing moves, the history is zeros (MM_0 = 0); a float32
    start runs in its dtype; a non-contiguous start solves."""
    from sph_raytracer_amd.retrieval import fista
    op, y, _ = _operator()
    fns, damp, N, b = _system('tiny', False, None)
    x, y_hat, info = fista(op, tr.zeros_like(y), loss_fns=fns, damp=damp, lower=-1.0, upper=1.0,
                           num_iterations=5)
    assert not x.any() and not y_hat.any() and info['residual'] == [0.0] * 5
    want = _minimiser('tiny', False, None, fc.LOWER, fc.UPPER)
    x32, _, _ = fista(op, y, loss_fns=fns, damp=damp, lower=fc.LOWER, upper=fc.UPPER,
                      num_iterations=fc.ITERATIONS, x0=tr.zeros(4, 3, 6, dtype=tr.float32))
    # (float32 rounding 6e-8 at a condition number of at most 100: 6e-6, with a decade to spare)
    assert x32.dtype == tr.float32 and cc.rel_err(x32.double().numpy(), want) <= 1e-4
    x0 = tr.zeros(6, 3, 4, dtype=F64).permute(2, 1, 0)
    xs, _, _ = fista(op, y, loss_fns=fns, damp=damp, lower=fc.LOWER, upper=fc.UPPER,
                     num_iterations=fc.ITERATIONS, x0=x0)
    assert cc.rel_err(xs.numpy(), want) <= fc.LIMIT
