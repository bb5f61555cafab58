"""retrieval.primal_dual on the GPU, against the minimiser certified by tests/pd_cases.py on the
dense system taken from the loss classes (cg_cases.dense_system through the stored Operator; D
from pd_cases.tv_matrix): the two problems of test_gpu_fista.py — 72 rays over 72 voxels, and 257
rays over 300 voxels (two workgroups, two partial sums) — in the four variants of mask and square
smooth term, with the bounds 0.35 / 0.65 and without, through the direct path over the stored
Operator and over a MatrixFreeOperator (float64 atomics, and the deterministic fixed-point
trace), and through the generic path on the same tensors.  pd_cases.ITERATIONS iterations, the
solution within pd_cases.LIMIT (both measured on the CPU: test_pd_cpu.py); bitwise equality where
the adjoint is deterministic."""
import functools
import math

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import pd_cases as pc
from test_gpu_fista import _bits, _operator, _problem
from test_pd_cpu import _inf, dense_problem, tv_term

pytestmark = pytest.mark.gpu
F64 = tr.float64
PROBLEMS = ['tiny', 'two_workgroups']
OPERATORS = ['stored', 'matrix_free', 'matrix_free_deterministic']
BOUNDS = [(pc.LOWER, pc.UPPER), (None, None)]


@functools.lru_cache(maxsize=None)
def _system(name, gpu, masked, wrap):
    """(quadratic terms, damp, N, b, D, c, B, L) of a variant, through the stored Operator."""
    _, _, op, y, mask = _problem(name, gpu)
    return dense_problem(op, y, mask, masked, wrap)


@functools.lru_cache(maxsize=None)
def _certified(name, gpu, masked, wrap, lower, upper):
    _, _, N, b, D, c, B, L = _system(name, gpu, masked, wrap)
    return pc.certify(N, b, D, c, *_inf(lower, upper), L, B)


def _terms(name, gpu, masked, wrap):
    return list(_system(name, gpu, masked, wrap)[0]) + [tv_term(masked)]


def _spy(monkeypatch):
    """Counts of the two paths' runs and of the two entries' calls."""
    from sph_raytracer_amd import _lib, retrieval
    seen = {'direct': 0, 'generic': 0, 'sphrt_pd_primal_f64': 0, 'sphrt_pd_dual_f64': 0}
    for key in ('direct', 'generic'):
        fn = getattr(retrieval, f'_primal_dual_{key}')

        def wrapped(*a, _fn=fn, _key=key, **k):
            seen[_key] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(retrieval, f'_primal_dual_{key}', wrapped)
    lib = _lib.load()
    for name in _lib.PD_EXPORTED:
        fn = getattr(lib, name)

        def counted(*a, _fn=fn, _name=name):
            seen[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counted)
    return seen


def _steps_are(info, ratio, B):
    """tau and sigma are those of the L reported, to two roundings (the steps are formed on the
    device, where torch divides a tensor by a constant through the constant's reciprocal)."""
    return all(math.isclose(info[k], v, rel_tol=4 * 2.0 ** -53, abs_tol=0.0) for k, v in
               zip(('tau', 'sigma'), pc.pd_steps(info['lipschitz'], ratio, B)))


def _flat_dual(q, up):
    qn = q.cpu().numpy().reshape(3, -1)
    return np.concatenate([qn[ax][up[ax] >= 0] for ax in range(3)])


def _check_solution(name, gpu, masked, wrap, lower, upper, x, info):
    """x within the limit of the certified minimiser, inside the bounds, |q| <= c exactly, +0.0
    where there is no edge, and (x, q) a certificate of its own that agrees with the reference's."""
    _, _, N, b, D, c, B, L = _system(name, gpu, masked, wrap)
    want, _, radius = _certified(name, gpu, masked, wrap, lower, upper)
    lo, hi = _inf(lower, upper)
    xn = x.cpu().numpy().reshape(-1).astype(np.float64)
    err = cc.rel_err(xn, want)
    assert err <= pc.LIMIT, err
    assert np.all((xn >= lo) & (xn <= hi))
    shape = tuple(x.shape[-3:])
    _, up = pc.neighbours(shape, pc.tv_wrap(masked), (1, 1, 1))
    q = info['dual']
    assert q.shape == (3,) + tuple(x.shape) and q.device == x.device
    qn = q.cpu().numpy().reshape(3, -1)
    cax = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS) / xn.size
    assert all(np.abs(qn[ax]).max() <= cax[ax] for ax in range(3))
    assert not qn[up < 0].any() and not np.signbit(qn[up < 0]).any()
    if x.dtype == F64:
        own = pc.radius_of(N, b, D, c, xn, _flat_dual(q, up), lo, hi)
        print(f'  error {err:.3g}, own radius {own / np.linalg.norm(want):.3g}')
        assert np.linalg.norm(xn - want) <= own + radius      # (both balls hold the minimiser)
    return err


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('masked,wrap', pc.VARIANTS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_direct_path_reaches_the_certified_minimiser(name, masked, wrap, kind, gpu, monkeypatch):
    from sph_raytracer_amd.retrieval import primal_dual
    grid, _, _, y, _ = _problem(name, gpu)
    op = _operator(name, kind, gpu)
    _, damp, N, b, D, c, B, L = _system(name, gpu, masked, wrap)
    lmax = float(np.linalg.eigvalsh(N)[-1])
    seen = _spy(monkeypatch)
    for run, (lower, upper) in enumerate(BOUNDS, 1):
        x, y_hat, info = primal_dual(op, y, _terms(name, gpu, masked, wrap), damp=damp,
                                     lower=lower, upper=upper, num_iterations=pc.ITERATIONS)
        assert seen == {'direct': run, 'generic': 0, 'sphrt_pd_primal_f64': run * pc.ITERATIONS,
                        'sphrt_pd_dual_f64': run * pc.ITERATIONS}
        assert x.shape == tuple(grid.shape) and x.dtype == F64 and x.device == y.device
        assert y_hat.shape == y.shape and tr.equal(y_hat, op(x))
        print(f'primal_dual {name} {kind} masked={masked} wrap={wrap} bounds={lower, upper}:')
        _check_solution(name, gpu, masked, wrap, lower, upper, x, info)
        assert info['lipschitz'] >= lmax and abs(info['lipschitz'] - L) <= 1e-9 * L
        assert _steps_are(info, 1.0, B)
        pcg, dcg = info['primal_change'], info['dual_change']
        assert len(pcg) == len(dcg) == pc.ITERATIONS and pcg[0] == 1.0
        assert all(math.isfinite(v) and v >= 0 for v in pcg + dcg) and pcg[-1] < 1e-6
    if wrap is None:                      # (without the square smooth term both bounds bind)
        want = _certified(name, gpu, masked, wrap, pc.LOWER, pc.UPPER)[0]
        assert (want == pc.LOWER).any() and (want == pc.UPPER).any()


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_short_runs_stay_inside_and_match_the_dense_restatement(name, kind, gpu):
    """Every iterate of a short run lies inside the bounds, bound voxels with the bound's bits,
    every |q| <= c, and x, q and the two histories are those of pd_dense for the same L and
    ratio: the info fields recomputed."""
    from sph_raytracer_amd.retrieval import primal_dual
    op, y = _operator(name, kind, gpu), _problem(name, gpu)[3]
    _, damp, N, b, D, c, B, _ = _system(name, gpu, True, False)
    L = 1.25 * float(np.linalg.eigvalsh(N)[-1])
    shape = tuple(_problem(name, gpu)[0].shape)
    _, up = pc.neighbours(shape, pc.tv_wrap(True), (1, 1, 1))
    x0 = tr.linspace(-1, 2, len(b), dtype=F64).reshape(shape).to(gpu)     # (outside on both sides)
    xs, qk, mm, qq = pc.pd_dense(N, b, D, c, pc.LOWER, pc.UPPER, L, 0.5, 40, B,
                                 x0=x0.cpu().numpy().reshape(-1))
    lo_bits, hi_bits = (np.float64(v).view(np.int64) for v in (pc.LOWER, pc.UPPER))
    cax = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS) / len(b)
    hit = [0, 0]
    for k in (0, 1, 2, 5, 40):
        x, _, info = primal_dual(op, y, _terms(name, gpu, True, False), damp=damp, lower=pc.LOWER,
                                 upper=pc.UPPER, num_iterations=k, lipschitz=L, dual_ratio=0.5,
                                 x0=x0)
        xn = x.cpu().numpy().reshape(-1)
        assert np.all((xn >= pc.LOWER) & (xn <= pc.UPPER)) and len(info['primal_change']) == k
        assert np.all(xn.view(np.int64)[xn == pc.LOWER] == lo_bits)
        assert np.all(xn.view(np.int64)[xn == pc.UPPER] == hi_bits)
        hit[0] += int((xn == pc.LOWER).sum())
        hit[1] += int((xn == pc.UPPER).sum())
        assert cc.rel_err(xn, xs[k]) <= 1e-12
        qn = info['dual'].cpu().numpy().reshape(3, -1)
        assert all(np.abs(qn[ax]).max() <= cax[ax] for ax in range(3))
    assert min(hit) > 0 and bool((x0 == tr.linspace(-1, 2, len(b), dtype=F64).reshape(shape).to(gpu)).all())
    assert info['lipschitz'] == L and _steps_are(info, 0.5, B)
    assert np.allclose(_flat_dual(info['dual'], up), qk, rtol=0, atol=1e-12 * c.max())
    assert (np.abs(qk) == c).any() and (np.abs(qk) < c).any()
    assert np.allclose(info['primal_change'], np.sqrt(np.array(mm) / mm[0]), rtol=1e-9)
    assert np.allclose(info['dual_change'], np.sqrt(qq), rtol=1e-9, atol=1e-18)


@pytest.mark.parametrize('masked,wrap', pc.VARIANTS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_generic_path_on_the_gpu_agrees(name, masked, wrap, gpu, monkeypatch):
    """The same tensors through the plain-torch path (forced)."""
    from sph_raytracer_amd import retrieval
    _, _, op, y, _ = _problem(name, gpu)
    damp = _system(name, gpu, masked, wrap)[1]
    seen = _spy(monkeypatch)
    monkeypatch.setattr(retrieval, '_cg_is_direct', lambda *a: False)
    x, _, info = retrieval.primal_dual(op, y, _terms(name, gpu, masked, wrap), damp=damp,
                                       lower=pc.LOWER, upper=pc.UPPER,
                                       num_iterations=pc.ITERATIONS)
    assert seen == {'direct': 0, 'generic': 1, 'sphrt_pd_primal_f64': 0, 'sphrt_pd_dual_f64': 0}
    _check_solution(name, gpu, masked, wrap, pc.LOWER, pc.UPPER, x, info)
    assert len(info['primal_change']) == pc.ITERATIONS and info['primal_change'][0] == 1.0


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_reproducible_where_the_adjoint_is(name, kind, gpu):
    """Two solves over the stored Operator, and over a deterministic MatrixFreeOperator, are
    bitwise equal (x, f(x), q and the histories, the estimated L included); float64 atomics are
    held to the limit only."""
    from sph_raytracer_amd.retrieval import primal_dual
    op, y = _operator(name, kind, gpu), _problem(name, gpu)[3]
    damp = _system(name, gpu, True, False)[1]
    runs = [primal_dual(op, y, _terms(name, gpu, True, False), damp=damp, lower=pc.LOWER,
                        upper=pc.UPPER, num_iterations=pc.ITERATIONS) for _ in range(2)]
    for x, _, info in runs:
        _check_solution(name, gpu, True, False, pc.LOWER, pc.UPPER, x, info)
    if kind != 'matrix_free':
        (xa, ya, ia), (xb, yb, ib) = runs
        assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(ya), _bits(yb))
        assert np.array_equal(_bits(ia.pop('dual')), _bits(ib.pop('dual'))) and ia == ib


def test_inputs_that_take_the_generic_path_still_solve(gpu, monkeypatch):
    """A float32 x0, a float32 y with it, a two-channel volume (each channel the single-channel
    problem of its measurements: every term's mean halves, the minimiser stays) and a dynamic
    operator (view i <-> time slice i; the TV term over each slice's r, e, a)."""
    from sph_raytracer_amd import Operator, SphericalGrid
    from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
    from sph_raytracer_amd.retrieval import primal_dual
    grid, geom, op, y, _ = _problem('tiny', gpu)
    damp = _system('tiny', gpu, False, True)[1]
    want = _certified('tiny', gpu, False, True, pc.LOWER, pc.UPPER)[0]
    seen = _spy(monkeypatch)
    kw = dict(damp=damp, lower=pc.LOWER, upper=pc.UPPER, num_iterations=pc.ITERATIONS)
    fns = _terms('tiny', gpu, False, True)
    x32, _, i32 = primal_dual(op, y, fns, x0=tr.zeros(tuple(grid.shape), dtype=tr.float32, device=gpu),
                              **kw)
    assert seen['generic'] == 1 and seen['direct'] == 0 and x32.dtype == tr.float32
    # (float32 rounding 6e-8 at a condition number of at most 100: 6e-6, with a decade to spare)
    assert cc.rel_err(x32.double().cpu().numpy(), want) <= 1e-4
    assert i32['dual'].dtype == tr.float32
    # the direct path's solution of the same problem
    xd, _, _ = primal_dual(op, y, fns, **kw)
    assert seen['direct'] == 1 and cc.rel_err(xd.cpu().numpy(), want) <= pc.LIMIT
    # two channels: the second one's measurements are the first one's
    y2 = tr.stack([y, y])
    x2, yh2, i2 = primal_dual(op, y2, fns, x0=tr.zeros((2,) + tuple(grid.shape), dtype=F64, device=gpu),
                              **kw)
    assert seen['generic'] == 2 and seen['direct'] == 1
    assert x2.shape == (2,) + tuple(grid.shape) and yh2.shape == y2.shape
    assert i2['dual'].shape == (3, 2) + tuple(grid.shape)
    for ch in range(2):
        assert cc.rel_err(x2[ch].cpu().numpy(), want) <= pc.LIMIT
        assert cc.rel_err(x2[ch].cpu().numpy(), xd.cpu().numpy().reshape(-1)) <= pc.LIMIT
    # a dynamic grid: two time slices, one per view
    dgrid = SphericalGrid(shape=(2, 4, 3, 6))
    dop = Operator(dgrid, geom, dynamic=True, device=gpu)
    g = tr.Generator().manual_seed(3)
    yd = dop(tr.rand(tuple(dgrid.shape), dtype=F64, generator=g).to(gpu)).detach()
    quad = [2.0 * SquareLoss()]
    N0, _, _ = cc.dense_system(dop, yd, quad, 0.0, tuple(dgrid.shape))
    ddamp = cc.damp_for(N0, math.prod(dgrid.shape))
    N, b, _ = cc.dense_system(dop, yd, quad, ddamp, tuple(dgrid.shape))
    assert cc.condition(N) <= cc.KAPPA_MAX
    D1, axis1, B = pc.tv_matrix((4, 3, 6), True, pc.TV_WEIGHTS)
    D, axis = np.kron(np.eye(2), D1), np.tile(axis1, 2)
    c = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS)[axis] / 144
    L = 1.05 * float(np.linalg.eigvalsh(N)[-1])
    tv = pc.LAM_TV * SmoothRegularizer(weights=pc.TV_WEIGHTS, kind='abs', wrap_a=True)
    # (a system outside the measured set: held to the dense restatement's iterates, and both to
    # the bounds and the clamps)
    xs, qk, mm, qq = pc.pd_dense(N, b, D, c, pc.LOWER, pc.UPPER, L, 1.0, 40, B)
    xt, yh, info = primal_dual(dop, yd, quad + [tv], damp=ddamp, lower=pc.LOWER, upper=pc.UPPER,
                               num_iterations=40, lipschitz=L)
    assert seen['generic'] == 3 and seen['direct'] == 1
    assert xt.shape == tuple(dgrid.shape) and yh.shape == yd.shape
    assert info['dual'].shape == (3,) + tuple(dgrid.shape)
    assert bool(((xt >= pc.LOWER) & (xt <= pc.UPPER)).all())
    assert cc.rel_err(xt.cpu().numpy(), xs[-1]) <= 1e-12
    _, up = pc.neighbours((4, 3, 6), True, (1, 1, 1))
    qt = info['dual'].cpu().numpy().reshape(3, 2, -1)
    flat = np.concatenate([qt[ax, s][up[ax] >= 0] for s in range(2) for ax in range(3)])
    assert np.allclose(flat, qk, rtol=0, atol=1e-12 * c.max()) and (np.abs(qk) == c).any()
    assert np.allclose(info['primal_change'], np.sqrt(np.array(mm) / mm[0]), rtol=1e-9)
