"""retrieval.fista on the GPU, against the bound-constrained minimiser of tests/fista_cases.py on
the dense system taken from the loss classes (cg_cases.dense_system through the stored Operator):
the two problems of test_gpu_cg.py — 72 rays over 72 voxels, and 257 rays over 300 voxels (two
workgroups, two partial sums) — in its four variants of mask and smooth term, through the direct
path over the stored Operator and over a MatrixFreeOperator (float64 atomics, and the
deterministic fixed-point trace), and through the generic path on the same tensors.  The bounds
are 0.35 / 0.65 (the truth is uniform in [0, 1]: both bind); fista_cases.ITERATIONS iterations,
the solution within fista_cases.LIMIT (both measured on the CPU: test_fista_cpu.py); bitwise
equality where the adjoint is deterministic."""
import functools
import math

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import fista_cases as fc

pytestmark = pytest.mark.gpu
F64 = tr.float64
PROBLEMS = ['tiny', 'two_workgroups']
VARIANTS = [(False, None), (True, None), (False, True), (True, False)]
OPERATORS = ['stored', 'matrix_free', 'matrix_free_deterministic']
LO, HI = fc.LOWER, fc.UPPER


@functools.lru_cache(maxsize=None)
def _problem(name, gpu):
    """(grid, geom, the stored Operator, y, mask) — built once, never written."""
    from sph_raytracer_amd import ConeRectGeom, Operator, SphericalGrid
    if name == 'tiny':
        grid = SphericalGrid(shape=(4, 3, 6))
        geom = ConeRectGeom((6, 6), pos=(5, 0.3, 1), fov=(25, 25)) + \
            ConeRectGeom((6, 6), pos=(-1, 4.5, -2), fov=(25, 25))
    else:
        grid = SphericalGrid(shape=(5, 6, 10))
        geom = ConeRectGeom((257, 1), pos=(4, 1, 0.5), fov=(50, 1))
    op = Operator(grid, geom, device=gpu)
    g = tr.Generator().manual_seed(11)
    truth = tr.rand(tuple(grid.shape), dtype=F64, generator=g).to(gpu)
    y = op(truth).detach()
    y = y + 0.01 * tr.randn(y.shape, dtype=F64, generator=g).to(gpu)
    mask = (tr.rand(y.shape, dtype=F64, generator=g) + 0.25).to(gpu)
    mask.view(-1)[3] = 0.0
    assert y.numel() == (72 if name == 'tiny' else 257)
    return grid, geom, op, y, mask


@functools.lru_cache(maxsize=None)
def _operator(name, kind, gpu):
    from sph_raytracer_amd import MatrixFreeOperator
    grid, geom, op, _, _ = _problem(name, gpu)
    if kind == 'stored':
        return op
    return MatrixFreeOperator(grid, geom, device=gpu,
                              deterministic=kind == 'matrix_free_deterministic')


def _terms(name, gpu, masked, wrap):
    from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
    mask = _problem(name, gpu)[4]
    fns = [1.5 * SquareLoss(projection_mask=mask if masked else 1)]
    if wrap is not None:
        fns.append(0.3 * SmoothRegularizer(weights=(1, 0.5, 2), wrap_a=wrap))
    return fns


@functools.lru_cache(maxsize=None)
def _system(name, gpu, masked, wrap, y32=False):
    """(damp, N, b, the minimiser inside the bounds, lambda_max) of a variant."""
    grid, _, op, y, _ = _problem(name, gpu)
    y = y.float().double() if y32 else y
    fns, shape = _terms(name, gpu, masked, wrap), tuple(grid.shape)
    N0, _, _ = cc.dense_system(op, y, fns, 0.0, shape)
    damp = cc.damp_for(N0, math.prod(shape))
    N, b, asym = cc.dense_system(op, y, fns, damp, shape)
    assert asym <= 1e-12 * np.abs(N).max()
    assert cc.condition(N) <= cc.KAPPA_MAX
    return damp, N, b, fc.bounded_minimiser(N, b, LO, HI), float(np.linalg.eigvalsh(N)[-1])


def _spy(monkeypatch):
    """Counts of the two paths' runs."""
    from sph_raytracer_amd import retrieval
    seen = {'direct': 0, 'generic': 0}
    for key in seen:
        fn = getattr(retrieval, f'_fista_{key}')

        def wrapped(*a, _fn=fn, _key=key, **k):
            seen[_key] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(retrieval, f'_fista_{key}', wrapped)
    return seen


def _bits(x):
    return x.detach().cpu().numpy().view(np.int64)


def _inside(x):
    return bool(((x >= LO) & (x <= HI)).all())


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('masked,wrap', VARIANTS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_direct_path_reaches_the_bounded_minimiser(name, masked, wrap, kind, gpu, monkeypatch):
    from sph_raytracer_amd.retrieval import cg, fista
    grid, _, _, y, _ = _problem(name, gpu)
    op = _operator(name, kind, gpu)
    damp, N, b, want, lmax = _system(name, gpu, masked, wrap)
    seen = _spy(monkeypatch)

    def solve(**kw):
        return fista(op, y, loss_fns=_terms(name, gpu, masked, wrap), damp=damp,
                     num_iterations=fc.ITERATIONS, **kw)

    x, y_hat, info = solve(lower=LO, upper=HI)
    assert seen == {'direct': 1, 'generic': 0}
    assert x.shape == tuple(grid.shape) and x.dtype == F64 and x.device == y.device
    assert y_hat.shape == y.shape and tr.equal(y_hat, op(x))
    e_x = cc.rel_err(x.cpu().numpy(), want)
    print(f'fista {name} {kind} masked={masked} wrap={wrap}: solution {e_x:.3g}, L / lambda_max '
          f'{info["lipschitz"] / lmax:.4f}, restarts {len(info["restarts"])}')
    assert e_x <= fc.LIMIT
    assert _inside(x)
    xn = x.cpu().numpy().reshape(-1)
    assert np.array_equal(xn == LO, want <= LO) and np.array_equal(xn == HI, want >= HI)
    assert info['lipschitz'] >= lmax
    res = info['residual']
    assert len(res) == fc.ITERATIONS and res[0] == 1.0
    assert all(math.isfinite(v) and v >= 0 for v in res) and res[-1] < 1e-10
    assert info['restarts'] and all(1 <= k < fc.ITERATIONS for k in info['restarts'])
    # without bounds: N^-1 b, which is cg's solution
    xu, _, _ = solve(lower=None, upper=None)
    xc, _, _ = cg(op, y, loss_fns=_terms(name, gpu, masked, wrap), damp=damp,
                  num_iterations=cc.ITERATIONS)
    assert seen == {'direct': 2, 'generic': 0}
    assert cc.rel_err(xu.cpu().numpy(), np.linalg.solve(N, b)) <= fc.LIMIT
    assert cc.rel_err(xu.cpu().numpy(), xc.cpu().numpy().reshape(-1)) <= fc.LIMIT
    # from a start of its own, outside the bounds (not written), with L given
    x0 = tr.full(tuple(grid.shape), 0.9, dtype=F64, device=gpu)
    xs, _, infos = solve(lower=LO, upper=HI, x0=x0, lipschitz=1.3 * lmax)
    assert seen == {'direct': 3, 'generic': 0} and infos['lipschitz'] == 1.3 * lmax
    assert cc.rel_err(xs.cpu().numpy(), want) <= fc.LIMIT and bool((x0 == 0.9).all())


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_short_runs_stay_inside_and_match_the_dense_restatement(name, kind, gpu):
    """Every iterate of a short run lies inside the bounds, bound voxels with the bound's bits,
    and is the iterate of fista_dense for the same L."""
    from sph_raytracer_amd.retrieval import fista
    op, y = _operator(name, kind, gpu), _problem(name, gpu)[3]
    damp, N, b, _, lmax = _system(name, gpu, True, True)
    L = 1.25 * lmax
    shape = tuple(_problem(name, gpu)[0].shape)
    x0 = tr.linspace(-1, 2, len(b), dtype=F64).reshape(shape).to(gpu)     # (outside on both sides)
    xs, restarts, mm = fc.fista_dense(N, b, L, LO, HI, 40, x0=x0.cpu().numpy().reshape(-1))
    lo_bits, hi_bits = (np.float64(v).view(np.int64) for v in (LO, HI))
    hit = [0, 0]
    for k in (0, 1, 2, 5, 40):
        x, _, info = fista(op, y, loss_fns=_terms(name, gpu, True, True), damp=damp, lower=LO,
                           upper=HI, num_iterations=k, lipschitz=L, x0=x0)
        assert _inside(x) and len(info['residual']) == k
        xn = x.cpu().numpy().reshape(-1)
        assert np.all(xn.view(np.int64)[xn == LO] == lo_bits)
        assert np.all(xn.view(np.int64)[xn == HI] == hi_bits)
        hit[0] += int((xn == LO).sum())
        hit[1] += int((xn == HI).sum())
        assert cc.rel_err(xn, xs[k]) <= 1e-12
    assert min(hit) > 0
    assert info['restarts'] == restarts and restarts
    assert np.allclose(info['residual'], np.sqrt(np.array(mm) / mm[0]), rtol=1e-9)


@pytest.mark.parametrize('masked,wrap', VARIANTS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_generic_path_on_the_gpu_agrees(name, masked, wrap, gpu, monkeypatch):
    """The same tensors through the plain-torch path (forced)."""
    from sph_raytracer_amd import retrieval
    _, _, op, y, _ = _problem(name, gpu)
    damp, _, _, want, lmax = _system(name, gpu, masked, wrap)
    seen = _spy(monkeypatch)
    monkeypatch.setattr(retrieval, '_cg_is_direct', lambda *a: False)
    x, _, info = retrieval.fista(op, y, loss_fns=_terms(name, gpu, masked, wrap), damp=damp,
                                 lower=LO, upper=HI, num_iterations=fc.ITERATIONS)
    assert seen == {'direct': 0, 'generic': 1}
    assert cc.rel_err(x.cpu().numpy(), want) <= fc.LIMIT and _inside(x)
    assert len(info['residual']) == fc.ITERATIONS and info['residual'][0] == 1.0
    assert info['lipschitz'] >= lmax and info['restarts']


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_reproducible_where_the_adjoint_is(name, kind, gpu):
    """Two solves over the stored Operator, and over a deterministic MatrixFreeOperator, are
    bitwise equal (x, f(x) and info, the estimated L included); float64 atomics are held to the
    limit only."""
    from sph_raytracer_amd.retrieval import fista
    op, y = _operator(name, kind, gpu), _problem(name, gpu)[3]
    damp, _, _, want, _ = _system(name, gpu, True, True)
    runs = [fista(op, y, loss_fns=_terms(name, gpu, True, True), damp=damp, lower=LO, upper=HI,
                  num_iterations=fc.ITERATIONS) for _ in range(2)]
    for x, _, _ in runs:
        assert cc.rel_err(x.cpu().numpy(), want) <= fc.LIMIT
    if kind != 'matrix_free':
        (xa, ya, ia), (xb, yb, ib) = runs
        assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(ya), _bits(yb))
        assert ia == ib


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_float32_measurements(name, kind, gpu, monkeypatch):
    """A float32 y stays on the direct path, promoted exactly where it is read."""
    from sph_raytracer_amd.retrieval import fista
    op, y = _operator(name, kind, gpu), _problem(name, gpu)[3]
    damp, _, _, want, _ = _system(name, gpu, True, None, y32=True)
    seen = _spy(monkeypatch)
    x, y_hat, _ = fista(op, y.float(), loss_fns=_terms(name, gpu, True, None), damp=damp,
                        lower=LO, upper=HI, num_iterations=fc.ITERATIONS)
    assert seen == {'direct': 1, 'generic': 0} and x.dtype == F64 and y_hat.dtype == F64
    assert cc.rel_err(x.cpu().numpy(), want) <= fc.LIMIT


def test_inputs_that_take_the_generic_path_still_solve(gpu, monkeypatch):
    """A non-contiguous x0, a float32 x0, and a dynamic operator (view i <-> time slice i)."""
    from sph_raytracer_amd import Operator, SphericalGrid
    from sph_raytracer_amd.loss import SquareLoss
    from sph_raytracer_amd.retrieval import fista
    grid, geom, op, y, _ = _problem('tiny', gpu)
    damp, _, _, want, _ = _system('tiny', gpu, True, True)
    seen = _spy(monkeypatch)
    kw = dict(loss_fns=_terms('tiny', gpu, True, True), damp=damp, lower=LO, upper=HI,
              num_iterations=fc.ITERATIONS)
    x0 = tr.zeros(6, 3, 4, dtype=F64, device=gpu).permute(2, 1, 0)
    x, _, _ = fista(op, y, x0=x0, **kw)
    assert seen == {'direct': 0, 'generic': 1}
    assert cc.rel_err(x.cpu().numpy(), want) <= fc.LIMIT and _inside(x)
    x32, _, _ = fista(op, y, x0=tr.zeros(tuple(grid.shape), dtype=tr.float32, device=gpu), **kw)
    assert seen == {'direct': 0, 'generic': 2} and x32.dtype == tr.float32
    # (float32 rounding 6e-8 at a condition number of at most 100: 6e-6, with a decade to spare)
    assert cc.rel_err(x32.double().cpu().numpy(), want) <= 1e-4
    # a dynamic grid: two time slices, one per view
    dgrid = SphericalGrid(shape=(2, 4, 3, 6))
    dop = Operator(dgrid, geom, dynamic=True, device=gpu)
    g = tr.Generator().manual_seed(3)
    yd = dop(tr.rand(tuple(dgrid.shape), dtype=F64, generator=g).to(gpu)).detach()
    fns = [2.0 * SquareLoss()]
    N0, _, _ = cc.dense_system(dop, yd, fns, 0.0, tuple(dgrid.shape))
    ddamp = cc.damp_for(N0, math.prod(dgrid.shape))
    N, b, _ = cc.dense_system(dop, yd, fns, ddamp, tuple(dgrid.shape))
    assert cc.condition(N) <= cc.KAPPA_MAX
    dwant = fc.bounded_minimiser(N, b, LO, HI)
    # (a system outside the measured set: 600 iterations, 2 sqrt(k) (1 - 1 / sqrt(k))^600 < 1e-26)
    xd, yh, info = fista(dop, yd, loss_fns=fns, damp=ddamp, lower=LO, upper=HI, num_iterations=600)
    assert seen == {'direct': 0, 'generic': 3}
    assert xd.shape == tuple(dgrid.shape) and yh.shape == yd.shape and _inside(xd)
    assert cc.rel_err(xd.cpu().numpy(), dwant) <= fc.LIMIT
