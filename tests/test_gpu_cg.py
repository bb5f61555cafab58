"""retrieval.cg on the GPU, against the dense algebra of tests/cg_cases.py (the system taken from
the loss classes by autograd through the stored Operator, its condition number asserted): the
tiny problem of test_cg_cpu.py — grid 4 x 3 x 6, two views of 6 x 6 rays — and one of 257 rays
over 300 voxels (two workgroups, two partial sums per dot product), each through the direct path
over the stored Operator and over a MatrixFreeOperator (float64 atomics, and the deterministic
fixed-point trace), and through the generic path on the same tensors.  Limits as on the CPU:
1e-10 relative on the solution and on the gradient of the loss classes' own total after 200
iterations at a condition number of at most 100, 1e-9 on the third iterate against the Krylov
minimiser; bitwise equality where the adjoint is deterministic."""
import functools
import math

import numpy as np
import pytest
import torch as tr

import cg_cases as cc

pytestmark = pytest.mark.gpu
F64 = tr.float64
PROBLEMS = ['tiny', 'two_workgroups']
# (masked, smooth term: None, or the azimuth ring closed / open)
VARIANTS = [(False, None), (True, None), (False, True), (True, False)]
OPERATORS = ['stored', 'matrix_free', 'matrix_free_deterministic']


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
    """(damp, N, b, N^-1 b) of a variant: damp from the undamped system's largest eigenvalue."""
    grid, _, op, y, _ = _problem(name, gpu)
    y = y.float().double() if y32 else y
    fns, shape = _terms(name, gpu, masked, wrap), tuple(grid.shape)
    N0, _, _ = cc.dense_system(op, y, fns, 0.0, shape)
    damp = cc.damp_for(N0, math.prod(shape))
    N, b, asym = cc.dense_system(op, y, fns, damp, shape)
    assert asym <= 1e-12 * np.abs(N).max()
    assert cc.condition(N) <= cc.KAPPA_MAX            # the condition the limits are derived under
    return damp, N, b, np.linalg.solve(N, b)


def _spy(monkeypatch):
    """Counts of the two paths' runs."""
    from sph_raytracer_amd import retrieval
    seen = {'direct': 0, 'generic': 0}
    for key in seen:
        fn = getattr(retrieval, f'_cg_{key}')

        def wrapped(*a, _fn=fn, _key=key, **k):
            seen[_key] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(retrieval, f'_cg_{key}', wrapped)
    return seen


def _bits(x):
    return x.detach().cpu().numpy().view(np.int64)


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('masked,wrap', VARIANTS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_direct_path_solves_the_dense_system(name, masked, wrap, kind, gpu, monkeypatch):
    from sph_raytracer_amd.retrieval import cg
    grid, _, stored, y, _ = _problem(name, gpu)
    op = _operator(name, kind, gpu)
    damp, N, b, want = _system(name, gpu, masked, wrap)
    seen = _spy(monkeypatch)

    def solve(**kw):
        return cg(op, y, loss_fns=_terms(name, gpu, masked, wrap), damp=damp, **kw)

    x, y_hat, info = solve(num_iterations=cc.ITERATIONS)
    assert seen == {'direct': 1, 'generic': 0}
    assert x.shape == tuple(grid.shape) and x.dtype == F64 and x.device == y.device
    assert y_hat.shape == y.shape and tr.equal(y_hat, op(x))
    e_x = cc.rel_err(x.cpu().numpy(), want)
    fns = _terms(name, gpu, masked, wrap)
    g0 = float(cc.grad_total(stored, y, fns, damp, tr.zeros_like(x)).norm())
    e_g = float(cc.grad_total(stored, y, fns, damp, x).norm()) / g0
    x3, _, info3 = solve(num_iterations=3)
    e_3 = cc.rel_err(x3.cpu().numpy(), cc.krylov_minimiser(N, b, 3))
    print(f'cg {name} {kind} masked={masked} wrap={wrap}: solution {e_x:.3g}, gradient {e_g:.3g}, '
          f'x3 {e_3:.3g}, kappa {cc.condition(N):.3g}')
    assert e_x <= cc.SOLVE_TOL and e_g <= cc.SOLVE_TOL and e_3 <= cc.KRYLOV_TOL
    res = info['residual']
    assert len(res) == cc.ITERATIONS + 1 and res[0] == 1.0 and info['converged_at'] is None
    assert all(math.isfinite(v) and v >= 0 for v in res) and res[-1] < 1e-12
    assert np.allclose(info3['residual'], res[:4], rtol=1e-9, atol=0)
    # from a start of its own (a contiguous float64 x0 stays on the direct path; it is not written)
    x0 = tr.full(tuple(grid.shape), 0.5, dtype=F64, device=gpu)
    xs, _, _ = solve(num_iterations=cc.ITERATIONS, x0=x0)
    assert seen == {'direct': 3, 'generic': 0}
    assert cc.rel_err(xs.cpu().numpy(), want) <= cc.SOLVE_TOL and bool((x0 == 0.5).all())


@pytest.mark.parametrize('masked,wrap', VARIANTS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_generic_path_on_the_gpu_agrees(name, masked, wrap, gpu, monkeypatch):
    """The same tensors through the plain-torch path (forced): within the dense-solve limit of
    the same N^-1 b as the direct path."""
    from sph_raytracer_amd import retrieval
    _, _, op, y, _ = _problem(name, gpu)
    damp, N, b, want = _system(name, gpu, masked, wrap)
    seen = _spy(monkeypatch)
    monkeypatch.setattr(retrieval, '_cg_is_direct', lambda *a: False)
    x, _, info = retrieval.cg(op, y, loss_fns=_terms(name, gpu, masked, wrap), damp=damp,
                              num_iterations=cc.ITERATIONS)
    assert seen == {'direct': 0, 'generic': 1}
    assert cc.rel_err(x.cpu().numpy(), want) <= cc.SOLVE_TOL
    assert len(info['residual']) == cc.ITERATIONS + 1 and info['residual'][0] == 1.0


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_reproducible_where_the_adjoint_is(name, kind, gpu):
    """Two solves over the stored Operator, and over a deterministic MatrixFreeOperator, are
    bitwise equal (x, f(x) and the history); float64 atomics are held to the tolerance only."""
    from sph_raytracer_amd.retrieval import cg
    op, y = _operator(name, kind, gpu), _problem(name, gpu)[3]
    damp, _, _, want = _system(name, gpu, True, True)
    tol = 1e-7         # (frozen by iteration 96 at kappa <= 100; |e| / |x| <= kappa |r| / |b|)
    runs = [cg(op, y, loss_fns=_terms(name, gpu, True, True), damp=damp, num_iterations=120,
               tol=tol) for _ in range(2)]
    for x, _, info in runs:
        assert info['converged_at'] is not None
        assert cc.rel_err(x.cpu().numpy(), want) <= cc.KAPPA_MAX * tol
    if kind != 'matrix_free':
        (xa, ya, ia), (xb, yb, ib) = runs
        assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(ya), _bits(yb))
        assert ia == ib


@pytest.mark.parametrize('kind', ['stored', 'matrix_free_deterministic'])
@pytest.mark.parametrize('name', PROBLEMS)
def test_freeze_and_zero_measurements(name, kind, gpu, monkeypatch):
    from sph_raytracer_amd.retrieval import cg
    op, y = _operator(name, kind, gpu), _problem(name, gpu)[3]
    damp = _system(name, gpu, True, True)[0]
    seen = _spy(monkeypatch)

    def solve(y, **kw):
        return cg(op, y, loss_fns=_terms(name, gpu, True, True), damp=damp, **kw)

    tol = 1e-6
    _, _, info = solve(y, num_iterations=cc.ITERATIONS, tol=tol)
    k, res = info['converged_at'], info['residual']
    # (|r_k| / |r_0| <= 2 sqrt(kappa) ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^k: under 1e-6 by k = 84)
    assert k is not None and 0 < k <= 84
    assert res[k] <= tol < min(res[:k]) and res[k:] == [res[k]] * (len(res) - k)
    xa, _, ia = solve(y, num_iterations=k + 1, tol=tol)
    xb, _, ib = solve(y, num_iterations=k + 20, tol=tol)
    xk, _, _ = solve(y, num_iterations=k)
    assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(xa), _bits(xk))
    assert ia['converged_at'] == ib['converged_at'] == k
    for t in (0.0, tol):          # b = 0: the PHP guard, nothing divides
        x, y_hat, info = solve(tr.zeros_like(y), num_iterations=5, tol=t)
        assert not bool(x.any()) and not bool(y_hat.any())
        assert info['residual'] == [0.0] * 6 and info['converged_at'] == (0 if t else None)
    assert seen == {'direct': 6, 'generic': 0}


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_float32_measurements(name, kind, gpu, monkeypatch):
    """A float32 y stays on the direct path, promoted exactly where it is read."""
    from sph_raytracer_amd.retrieval import cg
    op, y = _operator(name, kind, gpu), _problem(name, gpu)[3]
    damp, _, _, want = _system(name, gpu, True, None, y32=True)
    seen = _spy(monkeypatch)
    x, y_hat, _ = cg(op, y.float(), loss_fns=_terms(name, gpu, True, None), damp=damp,
                     num_iterations=cc.ITERATIONS)
    assert seen == {'direct': 1, 'generic': 0} and x.dtype == F64 and y_hat.dtype == F64
    assert cc.rel_err(x.cpu().numpy(), want) <= cc.SOLVE_TOL


@pytest.mark.parametrize('y32', [False, True])
@pytest.mark.parametrize('masked', [False, True])
def test_direct_gradient_is_autograd_s_bitwise(masked, y32, gpu):
    """Over the stored Operator, `_normal_direct`'s application against y — the loop's forward,
    the fidelity stage's residual launch, the adjoint: what cg, fista, primal_dual and
    chambolle_pock's power method start from — has the bits of autograd's gradient of
    lam * mean(w * (y - f(x))^2) through the loss class, at an x with entries of both signs: the
    equality `_gd_direct` documents, for a unit and a tensor mask, a float64 and a float32 y."""
    from sph_raytracer_amd import retrieval
    grid, _, op, y, _ = _problem('tiny', gpu)
    y = y.float() if y32 else y
    sq, = _terms('tiny', gpu, masked, None)
    g = tr.Generator().manual_seed(5)
    x = (tr.rand(tuple(grid.shape), dtype=F64, generator=g) - 0.25).to(gpu)
    want = cc.grad_total(op, y, [sq], 0.0, x)
    with tr.no_grad(), tr.cuda.device(gpu):
        got = retrieval._normal_direct(op, y, sq, None, x)[0](x, against_y=True)
    assert bool(want.any()) and np.array_equal(_bits(got), _bits(want))


def test_inputs_that_take_the_generic_path_still_solve(gpu, monkeypatch):
    """A non-contiguous x0, a float32 x0, and a dynamic operator (view i <-> time slice i)."""
    from sph_raytracer_amd import Operator, SphericalGrid
    from sph_raytracer_amd.loss import SquareLoss
    from sph_raytracer_amd.retrieval import cg
    grid, geom, op, y, _ = _problem('tiny', gpu)
    damp, _, _, want = _system('tiny', gpu, True, True)
    seen = _spy(monkeypatch)
    x0 = tr.zeros(6, 3, 4, dtype=F64, device=gpu).permute(2, 1, 0)
    x, _, _ = cg(op, y, loss_fns=_terms('tiny', gpu, True, True), damp=damp,
                 num_iterations=cc.ITERATIONS, x0=x0)
    assert seen == {'direct': 0, 'generic': 1}
    assert cc.rel_err(x.cpu().numpy(), want) <= cc.SOLVE_TOL
    x32, _, _ = cg(op, y, loss_fns=_terms('tiny', gpu, True, True), damp=damp, num_iterations=30,
                   x0=tr.zeros(tuple(grid.shape), dtype=tr.float32, device=gpu))
    assert seen == {'direct': 0, 'generic': 2} and x32.dtype == tr.float32
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
    xd, yh, info = cg(dop, yd, loss_fns=fns, damp=ddamp, num_iterations=cc.ITERATIONS)
    assert seen == {'direct': 0, 'generic': 3}
    assert xd.shape == tuple(dgrid.shape) and yh.shape == yd.shape
    assert cc.rel_err(xd.cpu().numpy(), np.linalg.solve(N, b)) <= cc.SOLVE_TOL
