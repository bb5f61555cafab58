"""The fused residual back-projection on the GPU: MatrixFreeOperator.residual_gradient (the
trace's normal mode, sphrt_trace_normal_f64) — yhat = A x and grad = A^T(scale (A x - m)) from one
trace — through every path a ray can take to its emit code, and gd()'s loop over it.

Reference: the C oracle's own trace with IEEE square roots (test_gpu_adjoint_paths._Ref:
oracle.trace_segments, oracle.forward and oracle.adjoint over it), never the code under test.

Tolerances (the project's own): float64 within 1e-10 x max|reference|, float32 within 1e-5 x;
against the two separate calls op.T(scale (op(x) - m)) rtol 1e-12 and atol 1e-12 x max (the same
products, the atomics in another order).  yhat is bitwise the float64 forward.  Atomic sums are
not bitwise reproducible: no two gradients are compared for bit equality — except where every
term is zero (a zero residual, rays that all miss).

Which path a case is on is asserted as in test_gpu_matrix_free.py §3: from the oracle (segment
counts), the plan (K against the limits of csrc/trace.hip) and the trace's deferred-ray counter
(gpu_helpers.exact_stats)."""
import gc as _gc
import math

import numpy as np
import pytest
import torch as tr

import golden_cases as gc
from gpu_helpers import exact_stats
from test_gpu_adjoint_paths import (DGRID, F32, F64, SGRID, T_DYN, TOL, _assert_close,
                                    _check_coverage, _orbit, _rand, _Ref, _static_geom)

pytestmark = pytest.mark.gpu

SCALE = 0.37            # not a power of two: the residual's product rounds
_EXACT_LDS = 64 * 1024  # csrc/trace.hip exact_wave_lds, as test_gpu_matrix_free.py


def _exact_waves(K):
    for w in (4, 1):
        if K * 36 + w * 780 <= _EXACT_LDS:
            return w
    return 0


def _assert_separate_agree(got, ref):
    assert tr.allclose(got, ref, rtol=1e-12, atol=1e-12 * float(ref.abs().max()))


def _ref_forward(ref, x, n_chan):
    """The oracle's A x of every channel -> (n_chan, n) float64."""
    xc = x.reshape((n_chan,) + tuple(x.shape[-3:]))
    return np.stack([ref.forward(xc[c]) for c in range(n_chan)])


def _ref_gradient(ref, fwd, m, scale, **kw):
    """The oracle's A^T(scale (fwd - m)) from its own forward `fwd`."""
    r = scale * (fwd.reshape(-1) - m.detach().cpu().double().numpy().reshape(-1))
    return ref.adjoint(tr.from_numpy(r), **kw)


def _assert_zero_residual(op, x, yhat):
    """m = op(x), bitwise yhat: every scattered term is (yhat - yhat) * scale * len = 0, so the
    gradient is exactly zero only if the scatter uses the sum the same kernel integrated."""
    m0 = op(x)
    assert tr.equal(m0, yhat)
    y0, g0 = op.residual_gradient(x, m0, SCALE)
    assert tr.equal(y0, m0) and g0.shape == x.shape and not g0.any()


# ---- 1. static grids, channels -------------------------------------------------------------------
@pytest.fixture(scope='module')
def static_cases():
    """name -> (grid, geom, reference, MatrixFreeOperator): built once per geometry, read-only."""
    cache = {}

    def get(name, gpu):
        if name not in cache:
            from sph_raytracer_amd import MatrixFreeOperator, SphericalGrid
            grid, geom = SphericalGrid(shape=SGRID), _static_geom(name)
            ref = _Ref(grid, geom)
            _check_coverage(ref)
            cache[name] = (grid, geom, ref, MatrixFreeOperator(grid, geom, device=gpu))
        return cache[name]

    return get


@pytest.mark.parametrize('lead', [(), (3,), (2, 2)], ids=['1ch', '3ch', '2x2ch'])
@pytest.mark.parametrize('name', ['S1', 'S2', 'S3', 'S4'])
def test_static_residual_gradient(name, lead, gpu, static_cases):
    """x of 1, 3 and (2, 2) channels: yhat bitwise the forward; grad against the oracle's adjoint
    of the oracle's residual and against the two separate calls; float32 in, float32 out."""
    grid, geom, ref, op = static_cases(name, gpu)
    n_chan = math.prod(lead)
    x = _rand(lead + SGRID, F64, 41, gpu)
    m = _rand(lead + tuple(geom.shape), F64, 42, gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE)
    assert yhat.shape == m.shape and yhat.dtype == F64 and yhat.device == gpu
    assert grad.shape == x.shape and grad.dtype == F64 and grad.device == gpu
    ax = op(x)
    assert tr.equal(yhat, ax)
    fwd = _ref_forward(ref, x, n_chan)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_gradient(ref, fwd, m, SCALE, n_chan=n_chan), TOL[F64])
    _assert_separate_agree(grad, op.T(SCALE * (ax - m)))
    x32, m32 = x.float(), m.float()
    y32, g32 = op.residual_gradient(x32, m32, SCALE)
    assert y32.dtype == F32 and g32.dtype == F32 and y32.shape == m.shape and g32.shape == x.shape
    fwd32 = _ref_forward(ref, x32, n_chan)
    _assert_close(y32, fwd32, TOL[F32])
    _assert_close(g32, _ref_gradient(ref, fwd32, m32, SCALE, n_chan=n_chan), TOL[F32])


def test_default_scale_and_host_input(gpu, static_cases):
    """scale defaults to 1; CPU tensors give CPU results."""
    grid, geom, ref, op = static_cases('S1', gpu)
    x, m = _rand(SGRID, F64, 43, 'cpu'), _rand(geom.shape, F64, 44, 'cpu')
    yhat, grad = op.residual_gradient(x, m)
    assert yhat.device.type == 'cpu' and grad.device.type == 'cpu'
    fwd = _ref_forward(ref, x, 1)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_gradient(ref, fwd, m, 1.0), TOL[F64])


# ---- 2. zero residual ----------------------------------------------------------------------------
@pytest.mark.parametrize('lead', [(), (3,)], ids=['1ch', '3ch'])
def test_zero_residual_gives_exactly_zero(lead, gpu, static_cases):
    grid, geom, ref, op = static_cases('S3', gpu)
    x = _rand(lead + SGRID, F64, 45, gpu)
    yhat, _ = op.residual_gradient(x, _rand(lead + tuple(geom.shape), F64, 46, gpu), SCALE)
    _assert_zero_residual(op, x, yhat)


# ---- 3. every emit path --------------------------------------------------------------------------
def _path_check(grid, geom, gpu, seed, ref=None):
    """yhat against the oracle's forward, grad against the oracle's adjoint of the oracle's
    residual, and the zero-residual check -> the reference."""
    from sph_raytracer_amd import MatrixFreeOperator
    ref = ref or _Ref(grid, geom)
    op = MatrixFreeOperator(grid, geom, device=gpu)
    x = _rand(grid.shape, F64, seed, gpu)
    m = _rand(geom.shape, F64, seed + 100, gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE)
    assert yhat.shape == tuple(geom.shape) and grad.shape == tuple(grid.shape)
    fwd = _ref_forward(ref, x, 1)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_gradient(ref, fwd, m, SCALE), TOL[F64])
    _assert_zero_residual(op, x, yhat)
    return ref


def test_head_segments(gpu):
    """Starts inside a voxel (the inside_starts fixture's): trace_one's head segment, -tneg, is
    integrated and scattered on lane 0."""
    case = gc.load('inside_starts')
    grid, geom = gc.make_grid(case), gc.FixtureGeom(case)
    st, shape = case['starts'], case['shape']
    inside = np.all((st >= 0) & (st < shape[:, None]), axis=0)
    assert inside.mean() >= 0.5
    ref = _path_check(grid, geom, gpu, 47)
    first = ref.vox[ref.ptr[:-1][inside]]
    svox = (st[0] * shape[1] + st[1]) * shape[2] + st[2]
    assert np.mean(first == svox[inside]) >= 0.9


@pytest.mark.parametrize('name', gc.LATTICE_CASES)
def test_lattice_tie_rays(name, gpu):
    """The four tie lattices: the rays the wave path defers go through exact_walk_wave (4 waves
    per ray at this K)."""
    from sph_raytracer_amd.raytracer import _Plan
    case = gc.load(name)
    grid = gc.make_grid(case)
    geom = gc.FixtureGeom(dict(case, xs=case['xs'].copy(), rays=case['rays'].copy()))
    assert len(case['xs']) == 8918
    assert _exact_waves(int(_Plan(grid, gpu).K)) == 4
    deferred = exact_stats(grid, geom, gpu)[0]
    ref = _Ref(grid, geom)
    hit = int((np.diff(ref.ptr) > 0).sum())
    assert 0 < deferred < hit, (deferred, hit)
    _path_check(grid, geom, gpu, 48, ref=ref)


def test_lds_list_path(gpu):
    """Lists of more than 512 entries are sorted and walked in LDS (pair_fmt)."""
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    grid = SphericalGrid(shape=(300, 2, 2))
    geom = ConeRectGeom((4, 5), pos=(3, 0.01, 0.02), fov=(2, 2))
    ref = _Ref(grid, geom)
    assert int((np.diff(ref.ptr) > 512).sum()) >= 8        # F >= segments > 512
    assert np.unique(ref.vox).size >= 0.5 * ref.vol
    _path_check(grid, geom, gpu, 49, ref=ref)


@pytest.mark.parametrize('nr,waves', [(880, 1), (1000, 0)], ids=['one_wave', 'serial'])
def test_exact_path_large_lists(nr, waves, gpu):
    """Tie rays on grids whose list no longer fits four waves' LDS (one wave per deferred ray,
    K = 1773) or any wave's (K = 2013 > 1815: the serial exact_walk, which walks twice —
    integrate, then scatter the residual of what it wrote)."""
    from sph_raytracer_amd import SphericalGrid
    from sph_raytracer_amd.raytracer import _Plan
    case = gc.load('lattice_full')
    grid = SphericalGrid(shape=(nr, 4, 4), size_r=(0, 2))
    K = int(_Plan(grid, gpu).K)
    assert K == 2 * (nr + 1) + 2 * 5 + 5 + 1 and _exact_waves(K) == waves
    assert waves == 1 or K > 1815
    xs, rays = case['xs'][::7].copy(), case['rays'][::7].copy()
    through = np.linalg.norm(np.cross(xs, rays), axis=1) == 0
    assert through.sum() >= 8                                # lines through the origin
    geom = gc.FixtureGeom(dict(xs=xs, rays=rays, ray_shape=np.array([len(xs)])))
    deferred = exact_stats(grid, geom, gpu)[0]
    ref = _Ref(grid, geom)
    assert 0 < deferred <= int((np.diff(ref.ptr) > 0).sum())
    _path_check(grid, geom, gpu, 50, ref=ref)


def test_large_k_route(gpu):
    """K = 14 017 > 13 653: no wave list at all, every hit ray goes through defer_hits_kernel to
    the serial exact path."""
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    from sph_raytracer_amd.raytracer import _Plan
    grid = SphericalGrid(shape=(7000, 3, 5))
    geom = ConeRectGeom((6, 8), pos=(3, 0, 0.5), fov=(40, 40))
    K = int(_Plan(grid, gpu).K)
    assert K == 14017 and K > 13653 and _exact_waves(K) == 0
    ref = _Ref(grid, geom)
    hit = int((np.diff(ref.ptr) > 0).sum())
    assert ref.n == 48 and hit >= 24
    assert exact_stats(grid, geom, gpu)[0] == hit            # every hit ray is deferred
    _path_check(grid, geom, gpu, 51, ref=ref)


def test_serial_walk_with_channels(gpu):
    """The serial exact_walk with three channels: one integrating walk per channel, then one
    scattering walk that reads every channel's residual."""
    from sph_raytracer_amd import MatrixFreeOperator, SphericalGrid
    case = gc.load('lattice_full')
    grid = SphericalGrid(shape=(1000, 4, 4), size_r=(0, 2))
    xs, rays = case['xs'][::7].copy(), case['rays'][::7].copy()
    geom = gc.FixtureGeom(dict(xs=xs, rays=rays, ray_shape=np.array([len(xs)])))
    assert exact_stats(grid, geom, gpu)[0] > 0
    ref = _Ref(grid, geom)
    op = MatrixFreeOperator(grid, geom, device=gpu)
    x = _rand((3,) + tuple(grid.shape), F64, 52, gpu)
    m = _rand((3,) + tuple(geom.shape), F64, 53, gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE)
    assert tr.equal(yhat, op(x))
    fwd = _ref_forward(ref, x, 3)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_gradient(ref, fwd, m, SCALE, n_chan=3), TOL[F64])
    _assert_zero_residual(op, x, yhat)


# ---- 4. all rays miss ----------------------------------------------------------------------------
def test_all_rays_miss(gpu):
    """A detector looking away from the grid: the screen writes yhat = 0 and nothing is
    scattered."""
    from sph_raytracer_amd import ConeRectGeom, MatrixFreeOperator, SphericalGrid
    grid = SphericalGrid(shape=SGRID)
    geom = ConeRectGeom((9, 7), pos=(5, 0, 0), lookdir=(1, 0, 0), fov=(20, 20))
    assert _Ref(grid, geom).ptr[-1] == 0
    op = MatrixFreeOperator(grid, geom, device=gpu)
    for lead in ((), (3,)):
        x = _rand(lead + SGRID, F64, 54, gpu)
        m = _rand(lead + tuple(geom.shape), F64, 55, gpu)
        yhat, grad = op.residual_gradient(x, m, SCALE)
        assert yhat.shape == m.shape and grad.shape == x.shape
        assert not yhat.any() and not grad.any()


# ---- 5. dynamic grids ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dyn():
    """5 views <-> 5 time slices, and the first of the views at every time step."""
    from sph_raytracer_amd import ConeCircGeom, SphericalGrid
    grid = SphericalGrid(shape=DGRID)
    geoms = [ConeCircGeom((24, 16), pos=p, fov=(0, 12)) for p in _orbit(T_DYN)]
    geom = sum(geoms)
    ref, ref1 = _Ref(grid, geom), _Ref(grid, geoms[0])
    assert ref.n == 1920 and ref1.n == 384
    _check_coverage(ref, div=ref.n // T_DYN, n_t=T_DYN)
    _check_coverage(ref1)
    return grid, geom, geoms[0], ref, ref1


def _autograd_gradient(op, x, m, scale):
    xg = x.clone().requires_grad_()
    grad, = tr.autograd.grad(0.5 * scale * ((op(xg) - m) ** 2).sum(), xg)
    return grad


def test_dynamic_view_time_pairing(dyn, gpu):
    """The 5-view collection: view i reads and updates time slice i (ray_chan_div > 0)."""
    from sph_raytracer_amd import MatrixFreeOperator
    grid, geom, _, ref, _ = dyn
    div = ref.n // T_DYN
    op = MatrixFreeOperator(grid, geom, dynamic=True, device=gpu)
    assert op._layout(DGRID) == (1, div, tuple(geom.shape))
    x, m = _rand(DGRID, F64, 56, gpu), _rand(geom.shape, F64, 57, gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE)
    assert yhat.shape == tuple(geom.shape) and grad.shape == DGRID
    assert tr.equal(yhat, op(x))
    fwd = ref.forward(x, div=div)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_gradient(ref, fwd, m, SCALE, div=div, n_t=T_DYN), TOL[F64])
    _assert_separate_agree(grad, _autograd_gradient(op, x, m, SCALE))
    _assert_zero_residual(op, x, yhat)


def test_dynamic_single_detector(dyn, gpu):
    """One detector seen by the 5 time steps (n_chan = T)."""
    from sph_raytracer_amd import MatrixFreeOperator
    grid, _, single, _, ref1 = dyn
    op = MatrixFreeOperator(grid, single, device=gpu)
    yshape = (T_DYN,) + tuple(single.shape)
    assert op._layout(DGRID) == (T_DYN, 0, yshape)
    x, m = _rand(DGRID, F64, 58, gpu), _rand(yshape, F64, 59, gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE)
    assert yhat.shape == yshape and grad.shape == DGRID
    assert tr.equal(yhat, op(x))
    fwd = _ref_forward(ref1, x, T_DYN)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_gradient(ref1, fwd, m, SCALE, n_chan=T_DYN), TOL[F64])
    _assert_separate_agree(grad, _autograd_gradient(op, x, m, SCALE))
    _assert_zero_residual(op, x, yhat)


# ---- 6. retrieval --------------------------------------------------------------------------------
def _gd_circ16(gpu):
    from sph_raytracer_amd import ConeCircGeom, MatrixFreeOperator, SphericalGrid
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    case = gc.load('gd_circ16')
    grid = SphericalGrid(shape=(16, 16, 16))
    geom = sum(ConeCircGeom(shape=(20, 16), pos=(5 * tr.cos(t), 5 * tr.sin(t), 1), fov=(0, 45))
               for t in tr.linspace(0, 2 * tr.pi, 12))
    assert tr.equal(geom.rays, tr.from_numpy(case['rays']))
    op = MatrixFreeOperator(grid, geom, device=gpu)
    meas = tr.from_numpy(case['meas']).to(gpu)
    return case, op, meas, FullyDenseModel(grid), SquareLoss(), NegRegularizer()


def _assert_gd_pins(case, coeffs, y_res, losses, sq, neg, what):
    l_sq, l_neg = np.array(losses[sq]), np.array(losses[neg])
    assert len(l_sq) == len(case['loss_sq']) == int(case['iterations'])
    e_sq = float((np.abs(l_sq - case['loss_sq']) / case['loss_sq']).max())
    e_neg = float(np.abs(l_neg - case['loss_neg']).max())
    e_c = float(np.abs(coeffs.detach().cpu().numpy() - case['coeffs']).max())
    e_y = gc.rel_close(y_res.detach().cpu().numpy(), case['y_result'], 1e-9)
    print(f'gd_circ16 matrix-free, {what}: loss_sq rel {e_sq:.3g}, loss_neg abs {e_neg:.3g}, '
          f'coeffs abs {e_c:.3g}, y_result rel {e_y:.3g}')
    assert e_sq <= 1e-9 and e_neg <= 1e-12 and e_c <= 1e-9 and e_y <= 1e-9
    assert l_sq[-1] < 0.05 * l_sq[0]


def test_gd_takes_the_fused_loop(gpu, monkeypatch):
    """gd() over a MatrixFreeOperator: _direct_plan declines, _fused_plan accepts; the loop never
    calls the operator's forward or adjoint (one forward after it, for the returned y) and meets
    the gd_circ16 fixture's pins."""
    from sph_raytracer_amd import retrieval
    case, op, meas, model, sq, neg = _gd_circ16(gpu)
    coeffs0 = tr.ones(model.coeffs_shape, dtype=F64, device=gpu)
    args = (op, meas, model, coeffs0, [sq, neg], [coeffs0])
    assert retrieval._direct_plan(*args) is None
    assert retrieval._fused_plan(*args) == (sq, neg)
    calls = {'forward': [], 'adjoint': 0, 'normal': 0}
    fwd, adj, normal = op._apply_forward, op._apply_adjoint, op._normal_into

    def forward(density):
        calls['forward'].append(fwd(density))
        return calls['forward'][-1]

    def adjoint(*a, **k):
        calls['adjoint'] += 1
        return adj(*a, **k)

    def normal_into(*a):
        calls['normal'] += 1
        return normal(*a)

    monkeypatch.setattr(op, '_apply_forward', forward)
    monkeypatch.setattr(op, '_apply_adjoint', adjoint)
    monkeypatch.setattr(op, '_normal_into', normal_into)
    coeffs, y_res, losses = retrieval.gd(op, meas, model, lr=0.1,
                                         num_iterations=int(case['iterations']),
                                         loss_fns=[sq, neg], progress_bar=False)
    assert len(calls['forward']) == 1 and calls['adjoint'] == 0
    assert calls['normal'] == int(case['iterations'])
    assert tr.equal(y_res.detach(), calls['forward'][0].detach())
    _assert_gd_pins(case, coeffs, y_res, losses, sq, neg, 'fused loop')


def test_gd_autograd_loop_still_meets_the_pins(gpu, monkeypatch):
    """The same run with the fused plan declined: the autograd loop, the same pins.  (No bit
    equality between the two loops: both sum with atomics.)"""
    from sph_raytracer_amd import retrieval
    case, op, meas, model, sq, neg = _gd_circ16(gpu)
    monkeypatch.setattr(retrieval, '_fused_plan', lambda *a, **k: None)
    calls = {'adjoint': 0}
    adj = op._apply_adjoint

    def adjoint(*a, **k):
        calls['adjoint'] += 1
        return adj(*a, **k)

    monkeypatch.setattr(op, '_apply_adjoint', adjoint)
    coeffs, y_res, losses = retrieval.gd(op, meas, model, lr=0.1,
                                         num_iterations=int(case['iterations']),
                                         loss_fns=[sq, neg], progress_bar=False)
    assert calls['adjoint'] == int(case['iterations'])
    _assert_gd_pins(case, coeffs, y_res, losses, sq, neg, 'autograd loop')


def test_fused_plan_conditions(gpu):
    """_fused_plan has _direct_plan's conditions: a dynamic grid, another model of the
    coefficients, measurements of another shape or a stored Operator take other loops."""
    from sph_raytracer_amd import MatrixFreeOperator, Operator, SphericalGrid, retrieval
    from sph_raytracer_amd.loss import SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom = SphericalGrid(shape=SGRID), _static_geom('S1')
    op = MatrixFreeOperator(grid, geom, device=gpu)
    model, sq = FullyDenseModel(grid), SquareLoss()
    c = tr.ones(SGRID, dtype=F64, device=gpu)
    y = _rand(geom.shape, F64, 60, gpu)
    assert retrieval._fused_plan(op, y, model, c, [sq], [c]) == (sq, None)
    assert retrieval._fused_plan(op, y[:-1], model, c, [sq], [c]) is None
    assert retrieval._fused_plan(op, y, model, c.float(), [sq], [c.float()]) is None
    assert retrieval._fused_plan(op, y, model, c, [sq], [c, y]) is None
    assert retrieval._fused_plan(op, None, model, c, [sq], [c]) is None
    assert retrieval._fused_plan(Operator(grid, geom, device=gpu), y, model, c, [sq], [c]) is None
    dgrid = SphericalGrid(shape=DGRID)
    dop = MatrixFreeOperator(dgrid, geom, device=gpu)
    dc = tr.ones(DGRID, dtype=F64, device=gpu)
    assert retrieval._fused_plan(dop, y, FullyDenseModel(dgrid), dc, [sq], [dc]) is None


# ---- 7. memory -----------------------------------------------------------------------------------
def test_call_holds_nothing_per_segment(gpu, static_cases):
    """residual_gradient keeps nothing: with its results freed the operator holds what it held
    before (bounded as in test_operator_holds_nothing_per_segment), and the call's peak exceeds
    that by no more than float64 copies of the inputs (none are made of float64 inputs), yhat and
    the accumulator, each rounded up to the caching allocator's 512-byte blocks — far below one
    entry per segment."""
    from sph_raytracer_amd import MatrixFreeOperator, _lib
    grid, geom, ref, _ = static_cases('S3', gpu)
    lib = _lib.load()
    x, m = _rand(SGRID, F64, 61, gpu), _rand(geom.shape, F64, 62, gpu)
    _gc.collect()
    tr.cuda.synchronize(gpu)
    base = tr.cuda.memory_allocated(gpu)
    op = MatrixFreeOperator(grid, geom, device=gpu)
    op.residual_gradient(x, m, SCALE)     # (results dropped: what a first call sets up is `held`)
    _gc.collect()
    tr.cuda.synchronize(gpu)
    held = tr.cuda.memory_allocated(gpu) - base
    plan, batch, ws = op._parts
    ws_bytes = lib.sphrt_trace_workspace_bytes(plan.handle, batch.n)
    assert 0 < held <= 48 * batch.n + ws_bytes + lib.sphrt_plan_table_bytes(plan._desc)
    tr.cuda.reset_peak_memory_stats(gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE)
    tr.cuda.synchronize(gpu)
    peak = tr.cuda.max_memory_allocated(gpu) - base - held
    allowed = 2 * (8 * x.numel() + 512) + 2 * (8 * m.numel() + 512)
    print(f'residual_gradient peak {peak} B over the operator, allowed {allowed} B, '
          f'{len(ref.seg)} segments ({12 * len(ref.seg)} B as a CSR)')
    assert 12 * len(ref.seg) > allowed        # (a per-segment buffer would not fit the bound)
    assert 0 < peak <= allowed
    del yhat, grad
    _gc.collect()
    tr.cuda.synchronize(gpu)
    assert tr.cuda.memory_allocated(gpu) - base == held
