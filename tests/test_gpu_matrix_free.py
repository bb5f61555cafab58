"""The matrix-free pair on the GPU: back_project (the fused trace's scatter mode,
sphrt_trace_backproject_f64) and MatrixFreeOperator (forward = line_integrals, adjoint =
back_project, differentiable), through every path a ray can take to its emit code.

Reference: the C oracle's own trace with IEEE square roots (oracle.trace_segments, never
op.segments()) and oracle.adjoint / oracle.forward over it, as test_gpu_adjoint_paths._Ref.

Tolerances (the project's own): float64 within 1e-10 x max|reference|, float32 within 1e-5 x;
against Operator.T with adjoint_mode='atomic' in float64 rtol 1e-12 and atol 1e-12 x max (the same
sums in another order); <A x, y> = <x, A^T y> within 1e-12 relative.  Atomic sums are not
bitwise reproducible: nothing here asserts bit equality of two back-projections — except the
all-miss case, which is exactly zero.

Which path a case is on is asserted from the oracle (segment counts), the plan (K against the
limits of csrc/trace.hip) and the trace's own deferred-ray counter (gpu_helpers.exact_stats)."""
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

# csrc/trace.hip: a deferred ray's list lives in LDS while K * 36 B + 780 B per wave fit 64 KiB
# (exact_wave_lds; 4 waves per ray, else 1, else the serial kernel over a workspace list), and a
# wave's own list while K <= 13 653 (one wave per workgroup, 12 B per entry of 160 KiB)
_EXACT_LDS = 64 * 1024


def _exact_waves(K):
    for w in (4, 1):
        if K * 36 + w * 780 <= _EXACT_LDS:
            return w
    return 0


def _assert_atomic_agree(got, ref, dt):
    """Against Operator's float64-atomic adjoint: the same products in another order."""
    if dt == F64:
        assert tr.allclose(got, ref, rtol=1e-12, atol=1e-12 * float(ref.abs().max()))
    else:
        _assert_close(got, ref.double().cpu().numpy(), TOL[dt])


# ---- 1. static grids, channels -------------------------------------------------------------------
@pytest.fixture(scope='module')
def static_cases():
    """name -> (grid, geom, reference, Operator): built once per geometry, read-only."""
    cache = {}

    def get(name, gpu):
        if name not in cache:
            from sph_raytracer_amd import Operator, SphericalGrid
            grid, geom = SphericalGrid(shape=SGRID), _static_geom(name)
            ref = _Ref(grid, geom)
            _check_coverage(ref)
            cache[name] = (grid, geom, ref, Operator(grid, geom, device=gpu))
        return cache[name]

    return get


@pytest.mark.parametrize('lead', [(), (3,), (2, 2)], ids=['1ch', '3ch', '2x2ch'])
@pytest.mark.parametrize('name', ['S1', 'S2', 'S3', 'S4'])
def test_static_back_project(name, lead, gpu, static_cases):
    """y of 1, 3 and (2, 2) channels, float64 and float32: against the oracle, against
    Operator.T with float64 atomics and against the transposed (deterministic) Operator.T."""
    from sph_raytracer_amd import back_project
    grid, geom, ref, op = static_cases(name, gpu)
    n_chan = math.prod(lead)
    for dt in (F64, F32):
        y = _rand(lead + tuple(geom.shape), dt, 21, gpu)
        got = back_project(grid, geom, y)
        assert got.shape == lead + SGRID and got.dtype == dt and got.device == gpu
        want = ref.adjoint(y, n_chan=n_chan)
        _assert_close(got, want, TOL[dt])
        yc, gc_ = y.reshape((n_chan,) + tuple(geom.shape)), got.reshape((n_chan,) + SGRID)
        try:
            for c in range(n_chan):
                op.adjoint_mode = 'atomic'
                _assert_atomic_agree(gc_[c], op.T(yc[c]), dt)
                op.adjoint_mode = 'transpose'
                _assert_close(gc_[c], op.T(yc[c]).double().cpu().numpy(), TOL[dt])
        finally:
            op.adjoint_mode = 'transpose'


def test_back_project_host_input_and_other_dtypes(gpu, static_cases):
    """A CPU y gives a CPU result; a float16 y computes from float32 and comes back float16."""
    from sph_raytracer_amd import back_project
    grid, geom, ref, _ = static_cases('S1', gpu)
    y = _rand(geom.shape, F64, 22, 'cpu')
    got = back_project(grid, geom, y)
    assert got.device.type == 'cpu' and got.dtype == F64
    _assert_close(got, ref.adjoint(y), TOL[F64])
    yh = y.to(gpu).half()
    got = back_project(grid, geom, yh)
    assert got.dtype == tr.float16 and got.device == gpu
    _assert_close(got, ref.adjoint(yh), 2e-3)        # (float16's own rounding of the result)


# ---- 2. dynamic grids ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dyn():
    """5 views <-> 5 time slices, and the first of the views at every time step."""
    from sph_raytracer_amd import ConeCircGeom, SphericalGrid
    grid = SphericalGrid(shape=DGRID)
    geoms = [ConeCircGeom((24, 16), pos=p, fov=(0, 12)) for p in _orbit(T_DYN)]
    geom = sum(geoms)
    ref, ref1 = _Ref(grid, geom), _Ref(grid, geoms[0])
    assert ref.n == 1920 and ref1.n == 384
    _check_coverage(ref)
    _check_coverage(ref, div=ref.n // T_DYN, n_t=T_DYN)
    _check_coverage(ref1)
    return grid, geom, geoms[0], ref, ref1


@pytest.mark.parametrize('dt', [F64, F32])
def test_dynamic_view_time_pairing(dyn, dt, gpu):
    """The 5-view collection: view i into time slice i (ray_chan_div > 0), against the oracle's
    time-paired accumulate and Operator.T(time_slices=True) with atomics; without
    time_slices=True the operator's T raises."""
    from sph_raytracer_amd import MatrixFreeOperator, Operator, back_project
    grid, geom, _, ref, _ = dyn
    div = ref.n // T_DYN
    y = _rand(geom.shape, dt, 23, gpu)
    want = ref.adjoint(y, div=div, n_t=T_DYN)
    got = back_project(grid, geom, y)
    assert got.shape == DGRID and got.dtype == dt and got.device == gpu
    _assert_close(got, want, TOL[dt])
    mf = MatrixFreeOperator(grid, geom, dynamic=True, device=gpu)
    assert mf._layout(DGRID) == (1, div, tuple(geom.shape))
    with pytest.raises(NotImplementedError):
        mf.T(y)
    with pytest.raises(NotImplementedError):
        back_project(grid, geom, y, time_slices=False)
    t = mf.T(y, time_slices=True)
    assert t.shape == DGRID and t.dtype == dt and t.device == gpu
    _assert_close(t, want, TOL[dt])
    op = Operator(grid, geom, dynamic=True, device=gpu)
    op.adjoint_mode = 'atomic'
    _assert_atomic_agree(t, op.T(y, time_slices=True), dt)


@pytest.mark.parametrize('dt', [F64, F32])
def test_dynamic_single_detector(dyn, dt, gpu):
    """One detector seen by the 5 time steps (n_chan = T): every time step's image into its
    slice."""
    from sph_raytracer_amd import MatrixFreeOperator, back_project
    grid, _, single, _, ref1 = dyn
    y = _rand((T_DYN,) + tuple(single.shape), dt, 24, gpu)
    want = ref1.adjoint(y, n_chan=T_DYN)
    got = back_project(grid, single, y)
    assert got.shape == DGRID and got.dtype == dt
    _assert_close(got, want, TOL[dt])
    mf = MatrixFreeOperator(grid, single, device=gpu)
    assert mf._layout(DGRID) == (T_DYN, 0, (T_DYN,) + tuple(single.shape))
    with pytest.raises(NotImplementedError):
        mf.T(y)
    _assert_close(mf.T(y, time_slices=True), want, TOL[dt])


# ---- 3. every emit path --------------------------------------------------------------------------
def _path_check(grid, geom, gpu, seed, ref=None, dts=(F64, F32)):
    """back_project of a random y against the oracle's adjoint -> the reference."""
    from sph_raytracer_amd import back_project
    ref = ref or _Ref(grid, geom)
    for dt in dts:
        y = _rand(geom.shape, dt, seed, gpu)
        got = back_project(grid, geom, y)
        assert got.shape == tuple(grid.shape) and got.dtype == dt
        _assert_close(got, ref.adjoint(y), TOL[dt])
    return ref


def test_head_segments(gpu):
    """Starts inside a voxel (the inside_starts fixture's): the distance behind the start goes
    into the start voxel (trace_one's head segment, -tneg)."""
    case = gc.load('inside_starts')
    grid, geom = gc.make_grid(case), gc.FixtureGeom(case)
    st, shape = case['starts'], case['shape']
    inside = np.all((st >= 0) & (st < shape[:, None]), axis=0)
    assert inside.mean() >= 0.5
    ref = _path_check(grid, geom, gpu, 25)
    # the oracle's first segment of such a ray lies in its start voxel
    first = ref.vox[ref.ptr[:-1][inside]]
    svox = (st[0] * shape[1] + st[1]) * shape[2] + st[2]
    assert np.mean(first == svox[inside]) >= 0.9
    from sph_raytracer_amd import back_project
    got = back_project(grid, geom, tr.from_numpy(case['y0']).to(gpu))
    want = np.asarray(ref.oracle.adjoint(ref.ptr, ref.vox, ref.seg, case['y0'], ref.vol))
    _assert_close(got, want, TOL[F64])


@pytest.mark.parametrize('name', gc.LATTICE_CASES)
def test_lattice_tie_rays(name, gpu):
    """The four tie lattices (8918 rays each): the rays the wave path defers go through
    exact_walk_wave (4 waves per ray at this K); every ray's segments, weighted by its own y,
    against the IEEE oracle."""
    from sph_raytracer_amd import back_project
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
    got = back_project(grid, geom, tr.from_numpy(case['y0']).to(gpu))
    want = np.asarray(ref.oracle.adjoint(ref.ptr, ref.vox, ref.seg, case['y0'], ref.vol))
    _assert_close(got, want, TOL[F64])
    got = back_project(grid, geom, tr.from_numpy(case['y0']).to(gpu).float())
    _assert_close(got, want, TOL[F32])


def test_lds_list_path(gpu):
    """Lists of more than 512 entries are sorted and walked in LDS (pair_fmt): rays within 0.1
    of the centre of 300 shells."""
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    grid = SphericalGrid(shape=(300, 2, 2))
    geom = ConeRectGeom((4, 5), pos=(3, 0.01, 0.02), fov=(2, 2))
    ref = _Ref(grid, geom)
    assert int((np.diff(ref.ptr) > 512).sum()) >= 8        # F >= segments > 512
    assert np.unique(ref.vox).size >= 0.5 * ref.vol
    _path_check(grid, geom, gpu, 26, ref=ref)


@pytest.mark.parametrize('nr,waves', [(880, 1), (1000, 0)], ids=['one_wave', 'serial'])
def test_exact_path_large_lists(nr, waves, gpu):
    """Tie rays on grids whose K-entry list no longer fits four waves' LDS (one wave per deferred
    ray, K = 1773) or any wave's (K = 2013 > 1815: lane 0 sorts and walks the list in the
    workspace, exact_walk): lattice rays, the lines through the origin among them."""
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
    _path_check(grid, geom, gpu, 27, ref=ref)


def test_large_k_route(gpu):
    """K = 14 017 > 13 653: no wave list at all, every hit ray goes through defer_hits_kernel to
    the serial exact path (the grid of test_large_k_trace_vs_oracle, 48 rays)."""
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
    _path_check(grid, geom, gpu, 28, ref=ref, dts=(F64,))


def test_all_rays_miss(gpu):
    """A detector looking away from the grid: the screen rejects every ray, nothing is written,
    the result is exactly zero."""
    from sph_raytracer_amd import ConeRectGeom, MatrixFreeOperator, SphericalGrid, back_project
    grid = SphericalGrid(shape=SGRID)
    geom = ConeRectGeom((9, 7), pos=(5, 0, 0), lookdir=(1, 0, 0), fov=(20, 20))
    ref = _Ref(grid, geom)
    assert ref.ptr[-1] == 0
    for dt in (F64, F32):
        y = _rand(geom.shape, dt, 29, gpu)
        got = back_project(grid, geom, y)
        assert got.shape == SGRID and got.dtype == dt and not got.any()
        assert not MatrixFreeOperator(grid, geom, device=gpu).T(y).any()


# ---- 4. operator properties ----------------------------------------------------------------------
def _prop_cases(dyn, gpu, static_cases):
    grid, geom, ref, _ = static_cases('S3', gpu)
    dgrid, dgeom, single, dref, ref1 = dyn
    return [(grid, geom, False, SGRID, tuple(geom.shape), ref, 0),
            (dgrid, dgeom, True, DGRID, tuple(dgeom.shape), dref, dref.n // T_DYN),
            (dgrid, single, False, DGRID, (T_DYN,) + tuple(single.shape), ref1, 0)]


def test_operator_forward_adjoint_gradient(dyn, gpu, static_cases):
    """MatrixFreeOperator on SGRID and DGRID: the forward equals line_integrals and the oracle;
    <A x, y> = <x, A^T y> within 1e-12 relative; autograd's gradient of (w * op(x)).sum() equals
    op.T(w)."""
    from sph_raytracer_amd import MatrixFreeOperator
    from sph_raytracer_amd.raytracer import line_integrals
    for grid, geom, dynamic, xshape, yshape, ref, div in _prop_cases(dyn, gpu, static_cases):
        op = MatrixFreeOperator(grid, geom, dynamic=dynamic, device=gpu)
        assert (op.grid, op.geom, op.dynamic, op.device) == (grid, geom, dynamic, gpu)
        ts = dict(time_slices=True) if grid.dynamic else {}
        for dt in (F64, F32):
            x, w = _rand(xshape, dt, 30, gpu), _rand(yshape, dt, 31, gpu)
            ax = op(x)
            assert ax.shape == yshape and ax.dtype == dt and not ax.requires_grad
            assert tr.equal(ax, line_integrals(grid, geom, x))
            if grid.dynamic and not div:
                want = np.stack([ref.forward(x[t]) for t in range(T_DYN)])
            else:
                want = ref.forward(x, div=div)
            _assert_close(ax, want, TOL[dt])
            atw = op.T(w, **ts)
            assert atw.shape == xshape and atw.dtype == dt
            xg = x.clone().requires_grad_()
            out = op(xg)
            assert out.requires_grad and tr.equal(out.detach(), ax)
            grad, = tr.autograd.grad((w * out).sum(), xg)
            assert grad.shape == xshape and grad.dtype == dt
            if dt == F64:
                lhs, rhs = float((ax * w).sum()), float((x * atw).sum())
                assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
                assert tr.allclose(grad, atw, rtol=1e-12, atol=1e-12 * float(atw.abs().max()))
            else:
                _assert_close(grad, atw.double().cpu().numpy(), TOL[dt])


def test_multichannel_gradient_equals_per_channel(gpu, static_cases):
    from sph_raytracer_amd import MatrixFreeOperator
    grid, geom, ref, _ = static_cases('S3', gpu)
    op = MatrixFreeOperator(grid, geom, device=gpu)
    x = _rand((3,) + SGRID, F64, 32, gpu).requires_grad_()
    w = _rand((3,) + tuple(geom.shape), F64, 33, gpu)
    out = op(x)
    assert out.shape == w.shape
    grad, = tr.autograd.grad((w * out).sum(), x)
    want = ref.adjoint(w, n_chan=3)
    for c in range(3):
        xc = x[c].detach().clone().requires_grad_()
        gc_, = tr.autograd.grad((w[c] * op(xc)).sum(), xc)
        assert tr.allclose(grad[c], gc_, rtol=1e-12, atol=1e-12 * float(gc_.abs().max()))
        _assert_close(grad[c], want[c], TOL[F64])
    assert tr.allclose(op.T(w), grad, rtol=1e-12, atol=1e-12 * float(grad.abs().max()))


# ---- 5. retrieval --------------------------------------------------------------------------------
def test_gd_with_matrix_free_operator(gpu):
    """gd() over a MatrixFreeOperator (the autograd loop: _direct_plan declines it) on the
    gd_circ16 problem meets that fixture's pin: coefficients within 1e-9, SquareLoss history
    within 1e-9 relative, NegRegularizer within 1e-12 (test_gpu_pins.test_gd_vs_reference)."""
    from sph_raytracer_amd import ConeCircGeom, MatrixFreeOperator, SphericalGrid, retrieval
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    case = gc.load('gd_circ16')
    grid = SphericalGrid(shape=(16, 16, 16))
    geom = sum(ConeCircGeom(shape=(20, 16), pos=(5 * tr.cos(t), 5 * tr.sin(t), 1), fov=(0, 45))
               for t in tr.linspace(0, 2 * tr.pi, 12))
    assert tr.equal(geom.rays, tr.from_numpy(case['rays']))
    op = MatrixFreeOperator(grid, geom, device=gpu)
    meas = tr.from_numpy(case['meas']).to(gpu)
    model = FullyDenseModel(grid)
    sq, neg = SquareLoss(), NegRegularizer()
    coeffs0 = tr.ones(model.coeffs_shape, dtype=F64, device=gpu)
    assert retrieval._direct_plan(op, meas, model, coeffs0, [sq, neg], [coeffs0]) is None
    coeffs, y_res, losses = retrieval.gd(op, meas, model, lr=0.1,
                                         num_iterations=int(case['iterations']),
                                         loss_fns=[sq, neg], progress_bar=False)
    l_sq, l_neg = np.array(losses[sq]), np.array(losses[neg])
    assert len(l_sq) == len(case['loss_sq']) == int(case['iterations'])
    e_sq = float((np.abs(l_sq - case['loss_sq']) / case['loss_sq']).max())
    e_neg = float(np.abs(l_neg - case['loss_neg']).max())
    e_c = float(np.abs(coeffs.detach().cpu().numpy() - case['coeffs']).max())
    e_y = gc.rel_close(y_res.detach().cpu().numpy(), case['y_result'], 1e-9)
    print(f'gd_circ16 matrix-free: loss_sq rel {e_sq:.3g}, loss_neg abs {e_neg:.3g}, '
          f'coeffs abs {e_c:.3g}, y_result rel {e_y:.3g}')
    assert e_sq <= 1e-9 and e_neg <= 1e-12 and e_c <= 1e-9 and e_y <= 1e-9
    assert l_sq[-1] < 0.05 * l_sq[0]


# ---- 6. memory -----------------------------------------------------------------------------------
def test_operator_holds_nothing_per_segment(gpu, static_cases):
    """Constructing the operator, one forward and one T, results freed: the device memory held
    grows by no more than the ray batch (at most 48 B per ray: starts and directions), the trace
    workspace (sphrt_trace_workspace_bytes) and the plan tables — the project's own sizes, no
    term per segment."""
    from sph_raytracer_amd import MatrixFreeOperator, _lib
    grid, geom, ref, _ = static_cases('S3', gpu)
    lib = _lib.load()
    x, w = _rand(SGRID, F64, 34, gpu), _rand(geom.shape, F64, 35, gpu)
    _gc.collect()
    tr.cuda.synchronize(gpu)
    base = tr.cuda.memory_allocated(gpu)
    op = MatrixFreeOperator(grid, geom, device=gpu)
    y = op(x)
    v = op.T(w)
    del y, v
    _gc.collect()
    tr.cuda.synchronize(gpu)
    grown = tr.cuda.memory_allocated(gpu) - base
    plan, batch, ws = op._parts
    assert batch.n == ref.n
    ws_bytes = lib.sphrt_trace_workspace_bytes(plan.handle, batch.n)
    assert ws.numel() == ws_bytes
    bound = 48 * batch.n + ws_bytes + lib.sphrt_plan_table_bytes(plan._desc)
    print(f'matrix-free operator holds {grown} B, bound {bound} B, '
          f'{len(ref.seg)} segments ({12 * len(ref.seg)} B as a CSR)')
    assert 0 < grown <= bound
