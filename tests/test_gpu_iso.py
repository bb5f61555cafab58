"""retrieval.primal_dual and retrieval.chambolle_pock with an IsoTVRegularizer on the GPU, against
the minimiser certified by tests/iso_cases.py on the dense system taken from the loss classes
through the stored Operator: the two problems of test_gpu_pd.py, masked and not, without the
square smooth term (the total chambolle_pock solves too: a SquareLoss, damping, the iso term),
with the bounds 0.35 / 0.65 and without, through the direct path over the stored Operator and
over a MatrixFreeOperator (float64 atomics, and the deterministic fixed-point trace).
iso_cases.ITERATIONS iterations, the solution within iso_cases.LIMIT (both measured on the CPU:
test_iso_cpu.py, which also measures chambolle_pock under the limit there); the bounds exactly,
the ball within 12 u in Fractions; bitwise equality where the adjoint is deterministic; the route
spied; a float32 start and a dynamic operator on the generic path."""
import functools
import math

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import iso_cases as ic
import pd_cases as pc
from test_gpu_fista import _bits, _operator, _problem
from test_pd_cpu import _inf, dense_problem

pytestmark = pytest.mark.gpu
F64 = tr.float64
PROBLEMS = ['tiny', 'two_workgroups']
OPERATORS = ['stored', 'matrix_free', 'matrix_free_deterministic']
SOLVERS = ['primal_dual', 'chambolle_pock']
BOUNDS = [(pc.LOWER, pc.UPPER), (None, None)]
WATCHED = ['sphrt_iso_primal_f64', 'sphrt_iso_dual_f64', 'sphrt_pd_primal_f64', 'sphrt_pd_dual_f64']


@functools.lru_cache(maxsize=None)
def _system(name, gpu, masked):
    """(damp, N, b, Dw, voxel, B, L, r) of a variant without the square smooth term."""
    _, _, op, y, mask = _problem(name, gpu)
    _, damp, N, b, _, _, _, L = dense_problem(op, y, mask, masked, None)
    Dw, voxel, B = ic.iso_matrix(tuple(op.grid.shape), pc.tv_wrap(masked), ic.TV_WEIGHTS)
    return damp, N, b, Dw, voxel, B, L, ic.LAM_TV / len(b)


@functools.lru_cache(maxsize=None)
def _certified(name, gpu, masked, lower, upper):
    _, N, b, Dw, voxel, B, L, r = _system(name, gpu, masked)
    return ic.certify(N, b, Dw, voxel, r, *_inf(lower, upper), L, B)


def _solve(solver, op, y, mask, masked, damp, lower, upper, iterations, **kw):
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.loss import SquareLoss
    fns = [1.5 * SquareLoss(projection_mask=mask if masked else 1), ic.tv_term(pc.tv_wrap(masked))]
    return getattr(retrieval, solver)(op, y, fns, damp=damp, lower=lower, upper=upper,
                                      num_iterations=iterations, **kw)


def _spy(monkeypatch):
    from sph_raytracer_amd import _lib, retrieval
    seen = {'direct': 0, 'generic': 0, **{k: 0 for k in WATCHED}}
    for solver in ('primal_dual', 'chambolle_pock'):
        for key in ('direct', 'generic'):
            fn = getattr(retrieval, f'_{solver}_{key}')

            def wrapped(*a, _fn=fn, _key=key, **k):
                seen[_key] += 1
                return _fn(*a, **k)
            monkeypatch.setattr(retrieval, f'_{solver}_{key}', wrapped)
    lib = _lib.load()
    for name in WATCHED:
        fn = getattr(lib, name)

        def counted(*a, _fn=fn, _name=name):
            seen[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counted)
    return seen


def _check_solution(name, gpu, masked, lower, upper, x, info):
    _, N, b, Dw, voxel, B, L, r = _system(name, gpu, masked)
    want, _, radius = _certified(name, gpu, masked, lower, upper)
    lo, hi = _inf(lower, upper)
    xn = x.cpu().numpy().reshape(-1).astype(np.float64)
    err = cc.rel_err(xn, want)
    assert err <= ic.LIMIT, err
    assert np.all((xn >= lo) & (xn <= hi))
    _, up = pc.neighbours(tuple(x.shape), pc.tv_wrap(masked), (1, 1, 1))
    q = info['dual']
    assert q.shape == (3,) + tuple(x.shape) and q.device == x.device
    qn = q.cpu().numpy().reshape(3, -1)
    excess = ic.ball_excess(qn, up, r)
    assert excess <= ic.BALL, float((excess - 1) * 2 ** 53)
    assert not qn[up < 0].any() and not np.signbit(qn[up < 0]).any()
    own = ic.radius_of(N, b, Dw, voxel, r, xn, ic.flat_dual(q, up), lo, hi)
    print(f'  error {err:.3g}, own radius {own / np.linalg.norm(want):.3g}, ball excess '
          f'{float((excess - 1) * 2 ** 53):.3g} u')
    assert np.linalg.norm(xn - want) <= own + radius          # (both balls hold the minimiser)
    return err


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('name', PROBLEMS)
@pytest.mark.parametrize('solver', SOLVERS)
def test_direct_path_reaches_the_certified_minimiser(solver, name, masked, kind, gpu, monkeypatch):
    grid, _, _, y, mask = _problem(name, gpu)
    op = _operator(name, kind, gpu)
    damp, N, b, Dw, voxel, B, L, r = _system(name, gpu, masked)
    seen = _spy(monkeypatch)
    K = ic.ITERATIONS
    for run, (lower, upper) in enumerate(BOUNDS, 1):
        x, y_hat, info = _solve(solver, op, y, mask, masked, damp, lower, upper, K)
        assert seen == {'direct': run, 'generic': 0, 'sphrt_iso_primal_f64': run * K,
                        'sphrt_iso_dual_f64': run * K, 'sphrt_pd_primal_f64': 0,
                        'sphrt_pd_dual_f64': 0}
        assert x.shape == tuple(grid.shape) and x.dtype == F64 and x.device == y.device
        assert y_hat.shape == y.shape and tr.equal(y_hat, op(x))
        print(f'{solver} {name} {kind} masked={masked} bounds={lower, upper}:')
        _check_solution(name, gpu, masked, lower, upper, x, info)
        pcg, dcg = info['primal_change'], info['dual_change']
        assert len(pcg) == len(dcg) == K and all(math.isfinite(v) and v >= 0 for v in pcg + dcg)
        if solver == 'primal_dual':
            assert abs(info['lipschitz'] - L) <= 1e-9 * L
            assert all(math.isclose(info[k], v, rel_tol=4 * 2.0 ** -53, abs_tol=0.0) for k, v in
                       zip(('tau', 'sigma'), pc.pd_steps(info['lipschitz'], 1.0, B)))
        else:
            kn2 = info['norm'] + B
            sigma = 1.5 / y.numel() / math.sqrt(kn2)
            assert math.isclose(info['sigma'], sigma, rel_tol=1e-14)
            assert math.isclose(info['tau'], 1 / (sigma * kn2 + 2 * damp / len(b)), rel_tol=1e-14)


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('solver', SOLVERS)
def test_short_runs_match_the_dense_restatement_and_reproduce(solver, kind, gpu):
    """40 iterations from a start outside the bounds: bound voxels carry the bound's bits, every
    triple lies in the ball, primal_dual's iterate is iso_dense's; two runs agree bitwise on the
    stored and the deterministic operator."""
    name = 'two_workgroups'
    op, (grid, _, _, y, mask) = _operator(name, kind, gpu), _problem(name, gpu)
    damp, N, b, Dw, voxel, B, _, r = _system(name, gpu, True)
    shape = tuple(grid.shape)
    _, up = pc.neighbours(shape, pc.tv_wrap(True), (1, 1, 1))
    x0 = tr.linspace(-1, 2, len(b), dtype=F64).reshape(shape).to(gpu)
    kw = dict(x0=x0)
    if solver == 'primal_dual':
        kw.update(lipschitz=1.25 * float(np.linalg.eigvalsh(N)[-1]), dual_ratio=0.5)
    runs = [_solve(solver, op, y, mask, True, damp, pc.LOWER, pc.UPPER, 40, **kw) for _ in range(2)]
    lo_bits, hi_bits = (np.float64(v).view(np.int64) for v in (pc.LOWER, pc.UPPER))
    for x, _, info in runs:
        xn = x.cpu().numpy().reshape(-1)
        assert np.all((xn >= pc.LOWER) & (xn <= pc.UPPER))
        assert np.all(xn.view(np.int64)[xn == pc.LOWER] == lo_bits) and (xn == pc.LOWER).any()
        assert np.all(xn.view(np.int64)[xn == pc.UPPER] == hi_bits) and (xn == pc.UPPER).any()
        qn = info['dual'].cpu().numpy().reshape(3, -1)
        assert ic.ball_excess(qn, up, r) <= ic.BALL
        assert (ic.norms(ic.flat_dual(info['dual'], up), voxel, len(b)) >= r * (1 - 1e-9)).any()
    if solver == 'primal_dual':
        xs, qk, mm, qq = ic.iso_dense(N, b, Dw, voxel, r, pc.LOWER, pc.UPPER, kw['lipschitz'], 0.5,
                                      40, B, x0=x0.cpu().numpy().reshape(-1))
        x, _, info = runs[0]
        assert cc.rel_err(x.cpu().numpy(), xs[-1]) <= 1e-12
        assert np.allclose(ic.flat_dual(info['dual'], up), qk, rtol=0, atol=1e-12 * r)
        assert np.allclose(info['primal_change'], np.sqrt(np.array(mm) / mm[0]), rtol=1e-9)
        assert np.allclose(info['dual_change'], np.sqrt(qq), rtol=1e-9, atol=1e-18)
    if kind != 'matrix_free':
        (xa, ya, ia), (xb, yb, ib) = runs
        assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(ya), _bits(yb))
        assert np.array_equal(_bits(ia.pop('dual')), _bits(ib.pop('dual')))
        if solver == 'chambolle_pock':
            assert np.array_equal(_bits(ia.pop('ray_dual')), _bits(ib.pop('ray_dual')))
        assert ia == ib


@pytest.mark.parametrize('solver', SOLVERS)
def test_inputs_that_take_the_generic_path_still_solve(solver, gpu, monkeypatch):
    """A float32 x0 runs the plain-torch path in its dtype and still reaches the minimiser; a
    dynamic operator runs it over each slice's r, e, a (primal_dual: iso_dense's iterates on the
    block system; chambolle_pock: inside the bounds and the ball)."""
    from sph_raytracer_amd import Operator, SphericalGrid, retrieval
    from sph_raytracer_amd.loss import SquareLoss
    grid, geom, op, y, mask = _problem('tiny', gpu)
    damp = _system('tiny', gpu, True)[0]
    want = _certified('tiny', gpu, True, pc.LOWER, pc.UPPER)[0]
    seen = _spy(monkeypatch)
    x32, _, i32 = _solve(solver, op, y, mask, True, damp, pc.LOWER, pc.UPPER, ic.ITERATIONS,
                         x0=tr.zeros(tuple(grid.shape), dtype=tr.float32, device=gpu))
    assert seen['generic'] == 1 and seen['direct'] == 0 and not any(seen[k] for k in WATCHED)
    assert x32.dtype == tr.float32 and i32['dual'].dtype == tr.float32
    # (float32 rounding 6e-8 at a condition number of at most 100: test_gpu_pd.py's bound)
    assert cc.rel_err(x32.double().cpu().numpy(), want) <= 1e-4
    dgrid = SphericalGrid(shape=(2, 4, 3, 6))
    dop = Operator(dgrid, geom, dynamic=True, device=gpu)
    g = tr.Generator().manual_seed(3)
    yd = dop(tr.rand(tuple(dgrid.shape), dtype=F64, generator=g).to(gpu)).detach()
    quad = [2.0 * SquareLoss()]
    N0, _, _ = cc.dense_system(dop, yd, quad, 0.0, tuple(dgrid.shape))
    ddamp = cc.damp_for(N0, 144)
    N, b, _ = cc.dense_system(dop, yd, quad, ddamp, tuple(dgrid.shape))
    D1, v1, B = ic.iso_matrix((4, 3, 6), True, ic.TV_WEIGHTS)
    D, voxel = np.kron(np.eye(2), D1), np.concatenate([v1, v1 + 72])
    L = 1.05 * float(np.linalg.eigvalsh(N)[-1])
    kw = dict(lipschitz=L) if solver == 'primal_dual' else {}
    xt, yh, info = getattr(retrieval, solver)(dop, yd, quad + [ic.tv_term(True)], damp=ddamp,
                                              lower=pc.LOWER, upper=pc.UPPER, num_iterations=40,
                                              **kw)
    assert seen['generic'] == 2 and seen['direct'] == 0 and not any(seen[k] for k in WATCHED)
    assert xt.shape == tuple(dgrid.shape) and yh.shape == yd.shape
    assert info['dual'].shape == (3,) + tuple(dgrid.shape)
    assert bool(((xt >= pc.LOWER) & (xt <= pc.UPPER)).all())
    _, up = pc.neighbours((4, 3, 6), True, (1, 1, 1))
    qt = info['dual'].cpu().numpy().reshape(3, 2, -1)
    for s in range(2):
        assert ic.ball_excess(qt[:, s], up, ic.LAM_TV / 144) <= ic.BALL
    if solver == 'primal_dual':
        xs, qk, mm, _ = ic.iso_dense(N, b, D, voxel, ic.LAM_TV / 144, pc.LOWER, pc.UPPER, L, 1.0, 40, B)
        assert cc.rel_err(xt.cpu().numpy(), xs[-1]) <= 1e-12
        flat = np.concatenate([qt[ax, s][up[ax] >= 0] for s in range(2) for ax in range(3)])
        assert np.allclose(flat, qk, rtol=0, atol=1e-12 * ic.LAM_TV / 144)
