"""Host side of the conjugate-gradient solver (retrieval.cg; csrc/loss.hip's three cg entries):
the entries are declared, exported and bound, and their refusals fire on the host; cg_cases holds
what it claims, on the references alone; cg refuses every total that is not known to be
quadratic; and the generic (plain torch) path over the oracle-backed CpuOperator solves a tiny
static problem — grid 4 x 3 x 6, two views of 6 x 6 rays — against dense algebra: the solution,
the gradient of the loss classes' own total, the third iterate against the Krylov minimiser, a
zero right-hand side and the freeze.  (No compute call of the library.)"""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import loop_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = tr.float64
VP, I64, DBL = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
ENTRIES = {
    'sphrt_cg_curvature_f64': [VP, VP, I64, DBL, VP, VP],
    'sphrt_cg_update_f64': [VP, VP, VP, VP, I64, VP, VP, I64, VP, VP, VP],
    'sphrt_cg_direction_f64': [VP, VP, I64, VP, VP, I64, VP, VP],
}


# ---- the C entries -------------------------------------------------------------------------------
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
        for a, ct in zip(args, argtypes):     # pointers, int64_t and double where bound so
            want = VP if '*' in a else I64 if a.startswith('int64_t') else DBL
            assert ct is want, (name, a)
        assert name in _lib.EXPORTED and hasattr(raw, name)
        fn = getattr(_lib.load(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes
    m = re.search(r'sphrt_cg_update_f64\s*\(([^;]*)\)', hdr).group(1)
    assert re.search(r'double \*x, double \*r, const double \*p, const double \*h, int64_t n,\s*'
                     r'const double \*part_rr, const double \*part_php, int64_t n_part,\s*'
                     r'const double \*rr_stop, double \*part_rr_new', m)


def test_refusals_on_the_host():
    """Every refusal returns non-zero with its word in sphrt_last_error before any launch: the
    pointers (small fake addresses) are never dereferenced."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    a, b, c, d, e, f, g = (VP(4096 * k) for k in range(1, 8))

    def curvature(p=a, h=b, n=300, c_damp=0.5, part=c):
        return lib.sphrt_cg_curvature_f64(p, h, n, c_damp, part, None)

    def update(x=a, r=b, p=c, h=d, n=300, rr=e, php=f, n_part=2, stop=None, out=g):
        return lib.sphrt_cg_update_f64(x, r, p, h, n, rr, php, n_part, stop, out, None)

    def direction(p=a, r=b, n=300, new=c, old=d, n_part=2, stop=None):
        return lib.sphrt_cg_direction_f64(p, r, n, new, old, n_part, stop, None)

    cases = [(curvature, dict(n=0), b'empty'), (curvature, dict(n=-5), b'empty')]
    cases += [(curvature, {k: None}, b'null') for k in ('p', 'h', 'part')]
    cases += [(update, dict(n=0), b'empty'), (update, dict(n=-1), b'empty')]
    cases += [(update, {k: None}, b'null') for k in ('x', 'r', 'p', 'h', 'rr', 'php', 'out')]
    cases += [(direction, dict(n=0), b'empty'), (direction, dict(n=-(2 ** 40)), b'empty')]
    cases += [(direction, {k: None}, b'null') for k in ('p', 'r', 'new', 'old')]
    for fn in (update, direction):
        # n_part must be the partial count of a launch over n elements (300 -> 2)
        cases += [(fn, dict(n_part=k), b'n_part') for k in (0, 1, 3, -2, 1024)]
        cases += [(fn, dict(n=n, n_part=k), b'n_part')
                  for n, k in ((1, 2), (256, 2), (257, 1), (262144, 1023), (2 ** 40, 1025))]
        for stop in (None, a):                # (with and without a freeze threshold)
            cases += [(fn, dict(n_part=3, stop=stop), b'n_part'), (fn, dict(n=0, stop=stop), b'empty')]
    for i, (fn, kw, word) in enumerate(cases):
        assert fn(**kw) != 0, (i, fn.__name__, kw)
        assert word in lib.sphrt_last_error(), (i, fn.__name__, kw, lib.sphrt_last_error())


# ---- cg_cases on its own references ----------------------------------------------------------------
def test_summation_orders():
    """kernel_sum and block_partials are sums (exactly, where every order is exact), take every
    element once, and are the documented order rather than another."""
    rng = np.random.default_rng(3)
    for n_part in (1, 2, 63, 64, 65, 255, 256, 257, 511, 1023, 1024):
        ints = rng.integers(-1000, 1000, size=n_part).astype(np.float64)
        assert cc.kernel_sum(ints) == ints.sum()
        one = np.zeros(n_part)
        for j in {0, n_part // 2, n_part - 1}:
            one[:] = 0
            one[j] = 1.0
            assert cc.kernel_sum(one) == 1.0
    # the order matters on values that do not sum exactly, and it is this one: by hand for the
    # slice of thread 0 (elements 0, 256, 512, 768), then lanes 0 and 32, then the waves
    part = np.zeros(1024)
    part[[0, 256, 512, 768]] = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53]
    assert cc.kernel_sum(part) == 1.0                       # ((1 + e) + e) + e: each add rounds down
    part[[0, 256, 512, 768]] = [2.0 ** -53, 2.0 ** -53, 1.0, 0.0]
    assert cc.kernel_sum(part) == 1.0 + 2.0 ** -52          # (e + e) + 1
    part[:] = 0
    part[[0, 32, 64]] = [2.0 ** -53, 2.0 ** -53, 1.0]       # lanes 0 + 32 pair first; wave 1 after
    assert cc.kernel_sum(part) == 1.0 + 2.0 ** -52
    part[[0, 32, 64]] = [1.0, 2.0 ** -53, 2.0 ** -53]       # (1 + e) first, then + e of wave 1
    assert cc.kernel_sum(part) == 1.0
    for n in lc.LENGTHS:
        k = rng.integers(-100, 100, size=n)
        got = cc.block_partials(k.astype(np.float64))
        assert got.shape == (lc.grid_of(n),)
        assert np.array_equal(got, lc._per_workgroup(k, n).astype(np.float64))


def test_exact_cases_are_exact():
    """alpha and beta are the dyadic rationals claimed, in the documented order and in plain
    summation alike; the integer references equal the float64 expressions (every operation is
    exact on this value set, fused or not), and the partial sums are integers in their unit."""
    for n in lc.LENGTHS:
        x, r, p, h = cc.exact_vectors(n, seed=7 * n)
        assert all(len(v) == n and np.abs(v).max() <= 64 for v in (x, r, p, h))
        for num, den in cc.DYADIC:
            top, bot = cc.dyadic_partials(n, num, den, seed=n + num)
            assert len(top) == lc.grid_of(n)
            assert cc.alpha_ref(cc.kernel_sum(top), cc.kernel_sum(bot), None) == num / den
            assert cc.beta_ref(cc.kernel_sum(top), cc.kernel_sum(bot), None) == num / den
            assert top.sum() / bot.sum() == num / den
            a = num / den
            xn, rn, part = cc.exact_update(x, r, p, h, num, den)
            assert np.array_equal(xn, x + a * p) and np.array_equal(rn, r - a * h)
            assert np.array_equal(part, cc.block_partials(rn * rn))
            assert np.array_equal(part * (8 * den) ** 2, np.round(part * (8 * den) ** 2))
            hn, php = cc.exact_curvature(p, h, num, den)
            assert np.array_equal(hn, a * p + h)
            assert np.array_equal(php, cc.block_partials(p * hn))
            assert np.array_equal(cc.exact_direction(p, r, num, den), a * p + r)
    # a sample through the rational fma too
    x, r, p, h = cc.exact_vectors(257, seed=1)
    xn, rn, _ = cc.exact_update(x, r, p, h, 3, 8)
    for i in cc.sample(257, 0, cap=32):
        assert cc.update_ref(x[i], r[i], p[i], h[i], 0.375) == (xn[i], rn[i])


def test_random_cases_tell_fma_from_multiply_add():
    differs = 0
    for n in (257, 262145):
        x, r, p, h = cc.random_vectors(n, seed=n)
        rr, php = cc.random_partials(n, seed=n)
        assert cc.kernel_sum(rr) > 0 and cc.kernel_sum(php) > 0
        alpha = cc.alpha_ref(cc.kernel_sum(rr), cc.kernel_sum(php), None)
        assert alpha == cc.kernel_sum(rr) / cc.kernel_sum(php)
        for i in cc.sample(n, seed=n):
            fused = cc.update_ref(x[i], r[i], p[i], h[i], alpha)
            plain = cc.update_unfused(x[i], r[i], p[i], h[i], alpha)
            differs += fused != plain
            # the two differ by the product's rounding (half an ulp of it) and one more rounding
            for got, two, prod in zip(fused, plain, (alpha * p[i], alpha * h[i])):
                assert abs(got - two) <= np.spacing(abs(prod)) + np.spacing(abs(got))
    assert differs > 50, differs       # (about a quarter of 2 x 514 elements)
    # the order of summation is visible in these partials: the documented order is not numpy's
    assert any(cc.kernel_sum(cc.random_partials(n, seed=n)[0]) !=
               float(np.sum(cc.random_partials(n, seed=n)[0])) for n in lc.LENGTHS[-4:])


def test_guards_of_alpha_and_beta():
    inf, nan = cc.INF, cc.NAN
    assert cc.alpha_ref(2.0, 8.0, None) == 0.25 and cc.alpha_ref(2.0, 8.0, 1.0) == 0.25
    assert cc.alpha_ref(2.0, 8.0, 2.0) == 0.0 and cc.alpha_ref(2.0, 8.0, 3.0) == 0.0   # frozen
    for php in (0.0, -0.0, -1.0, nan, -inf):
        assert cc.alpha_ref(2.0, php, None) == 0.0
    assert cc.alpha_ref(0.0, 0.0, None) == 0.0 and cc.alpha_ref(nan, 1.0, None) == 0.0
    assert cc.alpha_ref(inf, 1.0, None) == 0.0 and cc.alpha_ref(1e308, 1e-308, None) == 0.0
    assert cc.alpha_ref(0.0, 1.0, None) == 0.0 and cc.alpha_ref(1.0, inf, None) == 0.0
    assert cc.alpha_ref(2.0, 8.0, nan) == 0.25          # (a NaN threshold fails the compare)
    assert cc.beta_ref(1.0, 4.0, None) == 0.25 and cc.beta_ref(1.0, 4.0, 4.0) == 0.0
    for old in (0.0, -0.0, -1.0, nan):
        assert cc.beta_ref(1.0, old, None) == 0.0
    assert cc.beta_ref(inf, 1.0, None) == inf and math.isnan(cc.beta_ref(nan, 1.0, None))


# ---- cg's refusals -----------------------------------------------------------------------------------
def test_cg_refuses_what_is_not_quadratic():
    import sph_raytracer_amd as pkg
    from sph_raytracer_amd.loss import (AbsLoss, HuberLoss, NegRegularizer, SmoothRegularizer,
                                        SquareLoss, SquareRelLoss)
    from sph_raytracer_amd.retrieval import cg
    assert 'cg' in pkg.__all__ and pkg.cg is cg

    class Sub(SquareLoss):
        pass

    class SubSmooth(SmoothRegularizer):
        pass

    y = tr.zeros(2, 6, 6, dtype=F64)
    ok = SquareLoss
    bad = [
        ([], 'one SquareLoss'), ([SmoothRegularizer()], 'one SquareLoss'),
        ([ok(), ok()], 'two'), ([ok(), SmoothRegularizer(), SmoothRegularizer()], 'two'),
        ([ok(), NegRegularizer()], 'NegRegularizer'), ([AbsLoss()], 'AbsLoss'),
        ([HuberLoss(delta=0.5)], 'HuberLoss'), ([SquareRelLoss()], 'SquareRelLoss'),
        ([Sub()], 'Sub'), ([ok(), SubSmooth()], 'SubSmooth'),
        ([ok(), SmoothRegularizer(kind='abs')], "'abs'"),
        ([ok(), SmoothRegularizer(kind='huber', delta=1.0)], "'huber'"),
        ([tr.tensor(2.0) * ok()], 'lam'), ([ok(), tr.tensor(0.5) * SmoothRegularizer()], 'lam'),
        ([float('nan') * ok()], 'lam'), ([True * ok()], 'lam'),
        ([ok(use_grad=False)], 'use_grad'), ([ok(), SmoothRegularizer(use_grad=False)], 'use_grad'),
        ([ok(volume_mask=2)], 'volume_mask'), ([ok(volume_mask=tr.ones(4, 3, 6))], 'volume_mask'),
        ([ok(), SmoothRegularizer(volume_mask=0.5)], 'volume_mask'),
        ([ok(projection_mask=2)], 'projection_mask'),
        ([ok(projection_mask=tr.ones(5, 6, dtype=F64))], 'projection_mask'),        # no broadcast
        ([ok(projection_mask=tr.ones(6, 6, dtype=tr.int64))], 'projection_mask'),   # dtype
        ([ok(projection_mask=tr.ones(6, 6, requires_grad=True))], 'projection_mask'),
        ([ok(), SmoothRegularizer(projection_mask=tr.ones(6, 6))], 'projection_mask'),
    ]
    for fns, word in bad:
        with pytest.raises(ValueError, match=word):
            cg(None, y, loss_fns=fns)         # (refused before the operator is touched)
    for kw, word in ((dict(damp=-1.0), 'damp'), (dict(damp=float('inf')), 'damp'),
                     (dict(damp=float('nan')), 'damp'), (dict(damp=tr.tensor(1.0)), 'damp'),
                     (dict(tol=-1e-3), 'tol'), (dict(tol=float('nan')), 'tol'),
                     (dict(num_iterations=-1), 'num_iterations'),
                     (dict(num_iterations=2.5), 'num_iterations')):
        with pytest.raises(ValueError, match=word):
            cg(None, y, **kw)
    with pytest.raises(ValueError, match='tensor'):
        cg(None, None)


# ---- the generic path against dense algebra ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operator():
    from cpu_operator import CpuOperator
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    grid = SphericalGrid(shape=(4, 3, 6))
    geom = ConeRectGeom((6, 6), pos=(5, 0.3, 1), fov=(25, 25)) + \
        ConeRectGeom((6, 6), pos=(-1, 4.5, -2), fov=(25, 25))
    op = CpuOperator(grid, geom)
    g = tr.Generator().manual_seed(11)
    truth = tr.rand(tuple(grid.shape), dtype=F64, generator=g)
    y = op(truth).detach() + 0.01 * tr.randn(2, 6, 6, dtype=F64, generator=g)
    mask = (tr.rand(2, 6, 6, dtype=F64, generator=g) + 0.25)
    mask[0, 2, 3] = 0.0                      # (a masked pixel)
    return op, y, mask


def _terms(masked, smooth):
    from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
    mask = _operator()[2]
    fns = [1.5 * SquareLoss(projection_mask=mask if masked else 1)]
    if smooth:
        fns.append(0.3 * SmoothRegularizer(weights=(1, 0.5, 2)))
    return fns


VARIANTS = [(False, False), (True, False), (False, True), (True, True)]


@functools.lru_cache(maxsize=None)
def _system(masked, smooth):
    """(loss terms, damp, N, b, N^-1 b) of a variant, damp from the undamped system."""
    op, y, _ = _operator()
    fns, shape = _terms(masked, smooth), tuple(op.grid.shape)
    N0, _, _ = cc.dense_system(op, y, fns, 0.0, shape)
    damp = cc.damp_for(N0, math.prod(shape))
    N, b, asym = cc.dense_system(op, y, fns, damp, shape)
    assert asym <= 1e-12 * np.abs(N).max()
    return fns, damp, N, b, np.linalg.solve(N, b)


@pytest.mark.parametrize('masked,smooth', VARIANTS)
def test_generic_path_solves_the_dense_system(masked, smooth):
    from sph_raytracer_amd.retrieval import cg
    op, y, _ = _operator()
    fns, damp, N, b, want = _system(masked, smooth)
    assert cc.condition(N) <= cc.KAPPA_MAX        # the condition the bounds below are derived under
    x, y_hat, info = cg(op, y, loss_fns=fns, damp=damp, num_iterations=cc.ITERATIONS)
    assert x.shape == tuple(op.grid.shape) and x.dtype == F64 and not x.requires_grad
    assert tr.equal(y_hat, op(x)) and y_hat.shape == y.shape
    assert cc.rel_err(x.numpy(), want) <= cc.SOLVE_TOL
    # the gradient of the loss classes' own total (pins every lam / N factor against them)
    g0 = cc.grad_total(op, y, fns, damp, tr.zeros_like(x))
    assert float(cc.grad_total(op, y, fns, damp, x).norm()) <= cc.SOLVE_TOL * float(g0.norm())
    # info: one entry per iterate, from 1 down
    res = info['residual']
    assert len(res) == cc.ITERATIONS + 1 and res[0] == 1.0 and info['converged_at'] is None
    assert all(math.isfinite(v) and v >= 0 for v in res) and res[-1] < 1e-12
    # the third iterate is the Krylov minimiser (a method that merely converges is not)
    x3, _, info3 = cg(op, y, loss_fns=fns, damp=damp, num_iterations=3)
    assert cc.rel_err(x3.numpy(), cc.krylov_minimiser(N, b, 3)) <= cc.KRYLOV_TOL
    assert info3['residual'] == res[:4]
    # from another start: the same solution
    x0 = tr.full(tuple(op.grid.shape), 0.5, dtype=F64)
    xs, _, _ = cg(op, y, loss_fns=fns, damp=damp, num_iterations=cc.ITERATIONS, x0=x0)
    assert cc.rel_err(xs.numpy(), want) <= cc.SOLVE_TOL
    assert tr.equal(x0, tr.full_like(x0, 0.5))                 # (x0 is not written)


@pytest.mark.parametrize('masked,smooth', VARIANTS)
def test_zero_measurements_give_exact_zeros(masked, smooth):
    """b = 0: p = 0 and p N p = 0 from the first iteration (the PHP guard), nothing divides."""
    from sph_raytracer_amd.retrieval import cg
    op, y, _ = _operator()
    fns, damp, *_ = _system(masked, smooth)
    for tol in (0.0, 1e-6):
        x, y_hat, info = cg(op, tr.zeros_like(y), loss_fns=fns, damp=damp, num_iterations=5, tol=tol)
        assert not x.any() and not y_hat.any()
        assert info['residual'] == [0.0] * 6
        assert info['converged_at'] == (0 if tol else None)


@pytest.mark.parametrize('masked,smooth', VARIANTS)
def test_freeze_at_tol(masked, smooth):
    from sph_raytracer_amd.retrieval import cg
    op, y, _ = _operator()
    fns, damp, *_ = _system(masked, smooth)
    tol = 1e-6
    _, _, info = cg(op, y, loss_fns=fns, damp=damp, num_iterations=cc.ITERATIONS, tol=tol)
    k, res = info['converged_at'], info['residual']
    # (|r_k| / |r_0| <= 2 sqrt(kappa) ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^k: under 1e-6 by k = 84)
    assert k is not None and 0 < k <= 84
    assert res[k] <= tol < min(res[:k]) and res[k:] == [res[k]] * (len(res) - k)
    xa, _, ia = cg(op, y, loss_fns=fns, damp=damp, num_iterations=k + 1, tol=tol)
    xb, _, ib = cg(op, y, loss_fns=fns, damp=damp, num_iterations=k + 20, tol=tol)
    assert tr.equal(xa, xb) and ia['converged_at'] == ib['converged_at'] == k
    assert np.array_equal(xa.numpy().view(np.int64), xb.numpy().view(np.int64))
    # and it is the iterate of an unfrozen solve of k iterations
    xk, _, _ = cg(op, y, loss_fns=fns, damp=damp, num_iterations=k)
    assert tr.equal(xa, xk)


def test_generic_path_takes_other_inputs():
    """A float32 start (the solve runs in its dtype), a non-contiguous start and a bool mask."""
    from sph_raytracer_amd.loss import SquareLoss
    from sph_raytracer_amd.retrieval import cg
    op, y, mask = _operator()
    fns, damp, N, b, want = _system(False, False)
    x32, _, _ = cg(op, y, loss_fns=fns, damp=damp, num_iterations=30,
                   x0=tr.zeros(tuple(op.grid.shape), dtype=tr.float32))
    assert x32.dtype == tr.float32 and cc.rel_err(x32.double().numpy(), want) <= 1e-4
    x0 = tr.zeros(6, 3, 4, dtype=F64).permute(2, 1, 0)
    xs, _, _ = cg(op, y, loss_fns=fns, damp=damp, num_iterations=cc.ITERATIONS, x0=x0)
    assert cc.rel_err(xs.numpy(), want) <= cc.SOLVE_TOL
    keep = mask > 0.5
    xb, _, _ = cg(op, y, loss_fns=[SquareLoss(projection_mask=keep)], damp=damp,
                  num_iterations=cc.ITERATIONS)
    xf, _, _ = cg(op, y, loss_fns=[SquareLoss(projection_mask=keep.double())], damp=damp,
                  num_iterations=cc.ITERATIONS)
    assert tr.equal(xb, xf) and xb.dtype == F64
