"""The trace-order layer against the C oracle, in geometry order.

Every case of tests/order_cases.py (one per decision of raytracer._view_tiles, _trace_order and
SPHRT_RAY_ORDER: view tiles of every kind, wedges with and without a remainder, orbits where both
compete, dynamic orbits, a mixed collection, forced and refused tiles) runs the whole stack on
the GPU and every result is compared, in geometry order, with the oracle's reference for the
case — never with another run of the library (the one exception: gd's direct loop against its
autograd loop, bitwise by the project's contract).  tests/test_order_cases_cpu.py shows on the
references alone that any two adjacent views, rows or columns swapped, or a view paired with a
neighbouring time slice, move some output by 100 x the loosest tolerance below: a wrong row <->
ray map cannot pass.

Tolerances are the project's: segments by gc.compare_segments as in test_gpu_fuzz.py (voxel
sequences exact, lengths 1e-12); forwards gc.F64_RTOL / gc.F32_RTOL by gc.rel_close; adjoints and
gradients 1e-10 x the reference's maximum.
"""
import numpy as np
import pytest
import torch as tr

import golden_cases as gc
import order_cases as oc

pytestmark = pytest.mark.gpu

ADJ_RTOL = 1e-10


def _env(case, monkeypatch):
    monkeypatch.delenv('SPHRT_RAY_ORDER', raising=False)
    for k, v in oc.build(case)[2].items():
        monkeypatch.setenv(k, v)


def _operator(name, gpu, monkeypatch, cls=None, **kw):
    from sph_raytracer_amd import Operator
    case = oc.BY_NAME[name]
    _env(case, monkeypatch)
    grid, geom, _ = oc.build(case)
    return case, grid, geom, (cls or Operator)(grid, geom, device=gpu, **kw)


def _dev(a, gpu, dtype=tr.float64):
    return tr.tensor(a, dtype=dtype, device=gpu)


def _adj_close(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape, f'{what}: shape {got.shape} != {want.shape}'
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max()) / scale
    assert err <= ADJ_RTOL, f'{what}: {err:.3g} of the maximum'


def _fwd_close(got, want, rtol, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape, f'{what}: shape {got.shape} != {want.shape}'
    err = gc.rel_close(got, want, rtol)
    assert err <= rtol, f'{what}: rel err {err:.3g}'


def _transpose(op, y, case):
    return op.T(y, time_slices=True) if case.dynamic else op.T(y)


@pytest.mark.parametrize('name', oc.NAMES)
def test_trace(name, gpu, monkeypatch):
    """segments() gives the oracle's segments ray by ray in geometry order; a reported ray_id map
    is a permutation of the rays, and is reported exactly when the layer chose a tile or a wedge
    (the case then really runs in another order)."""
    case, grid, geom, op = _operator(name, gpu, monkeypatch)
    ref = oc.reference(name)
    got = tuple(t.cpu().numpy() for t in op.segments())
    msg = gc.compare_segments(ref.segs, got, oc.SCALE, name)
    assert msg is None, msg
    n = int(np.prod(case.shape))
    assert len(got[0]) == n + 1
    rid = op._csr['ray_id']
    tiles, wedge = oc.decisions(case)
    assert (rid is not None) == (tiles is not None or wedge is not None)
    if rid is not None:
        assert np.array_equal(np.sort(rid.cpu().numpy()), np.arange(n))


@pytest.mark.parametrize('name', oc.NAMES)
def test_forward(name, gpu, monkeypatch):
    """op(x) in geometry order, float64 and float32, one channel and (static grids: a dynamic
    grid takes (T, nr, ne, na) only) three channels of different densities; a dynamic case pairs
    view v with time slice v."""
    case, grid, geom, op = _operator(name, gpu, monkeypatch)
    ref = oc.reference(name)
    sets = [(ref.x, ref.y)] + ([(ref.x3, ref.y3)] if not case.dynamic else [])
    for x, want in sets:
        got = op(_dev(x, gpu))
        assert got.dtype == tr.float64 and tuple(got.shape[-len(case.shape):]) == case.shape
        _fwd_close(got, want, gc.F64_RTOL, f'{name} f64 {x.shape}')
        got32 = op(_dev(x, gpu, tr.float32))
        assert got32.dtype == tr.float32
        _fwd_close(got32, want, gc.F32_RTOL, f'{name} f32 {x.shape}')


@pytest.mark.parametrize('name', oc.NAMES)
def test_adjoint(name, gpu, monkeypatch):
    """op.T(y) for y in geometry order, three calls (launches alternate their block order from
    call to call).  Dynamic: the result has the grid's shape and slice t holds view t's
    back-projection alone — all of it, and nothing of another view."""
    case, grid, geom, op = _operator(name, gpu, monkeypatch)
    ref = oc.reference(name)
    y = _dev(ref.yt, gpu)
    for call in range(3):
        got = _transpose(op, y, case)
        assert tuple(got.shape) == tuple(grid.shape)
        _adj_close(got, ref.xt, f'{name} call {call}')
    if case.dynamic:
        t = 2
        only = tr.zeros_like(y)
        only[t] = y[t]
        got = _transpose(op, only, case)
        want = np.zeros_like(ref.xt)
        want[t] = ref.xt[t]
        _adj_close(got, want, f'{name} view {t} alone')
        rest = got.clone()
        rest[t] = 0
        assert not bool(rest.any()), f'{name}: view {t} reached another time slice'


@pytest.mark.parametrize('name', oc.NAMES)
def test_autograd(name, gpu, monkeypatch):
    """(op(xg) * y).sum().backward() leaves the oracle's adjoint of y in xg.grad."""
    case, grid, geom, op = _operator(name, gpu, monkeypatch)
    ref = oc.reference(name)
    xg = _dev(ref.x, gpu).requires_grad_()
    (op(xg) * _dev(ref.yt, gpu)).sum().backward()
    _adj_close(xg.grad, ref.xt, name)


@pytest.mark.parametrize('deterministic', [False, True])
@pytest.mark.parametrize('name', oc.STATIC)
def test_matrix_free(name, deterministic, gpu, monkeypatch):
    """MatrixFreeOperator's forward, T and residual_gradient against the oracle: A x, A^T y, and
    for the last A x with A^T(scale (A x - m))."""
    from oracle import oracle as ora
    from sph_raytracer_amd import MatrixFreeOperator
    case, grid, geom, op = _operator(name, gpu, monkeypatch, cls=MatrixFreeOperator,
                                     deterministic=deterministic)
    ref = oc.reference(name)
    x, m = _dev(ref.x, gpu), _dev(ref.yt, gpu)
    _fwd_close(op(x), ref.y, gc.F64_RTOL, f'{name} f64')
    _fwd_close(op(_dev(ref.x3, gpu)), ref.y3, gc.F64_RTOL, f'{name} f64 x3')
    _fwd_close(op(x.float()), ref.y, gc.F32_RTOL, f'{name} f32')
    _adj_close(op.T(m), ref.xt, f'{name} T')
    scale = 0.37
    yhat, grad = op.residual_gradient(x, m, scale)
    _fwd_close(yhat, ref.y, gc.F64_RTOL, f'{name} residual_gradient forward')
    want = np.asarray(ora.adjoint(*ref.segs, scale * (ref.y - ref.yt), ref.n_vox))
    _adj_close(grad, want.reshape(ref.x.shape), f'{name} residual_gradient gradient')


@pytest.mark.parametrize('name', oc.STATIC_ORBITS)
def test_gd(name, gpu, monkeypatch):
    """retrieval.gd, 3 iterations of SquareLoss + NegRegularizer on the oracle's forward as the
    measurement: the direct loop (trace-position rows, measurements permuted once, the adjoint in
    trace order) and the autograd loop give the same bits, and the returned forward is the
    oracle's forward of the returned coefficients."""
    from oracle import oracle as ora
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    case, grid, geom, op = _operator(name, gpu, monkeypatch)
    ref = oc.reference(name)
    meas = _dev(ref.y, gpu)
    calls = []
    direct = retrieval._gd_direct
    monkeypatch.setattr(retrieval, '_gd_direct',
                        lambda *a, **k: calls.append(1) or direct(*a, **k))
    runs = []
    for use_direct in (True, False):
        if not use_direct:
            monkeypatch.setattr(retrieval, '_direct_plan', lambda *a: None)
        c, yh, _ = retrieval.gd(op, meas.clone(), FullyDenseModel(grid), lr=1e-1,
                                num_iterations=3, loss_fns=[SquareLoss(), NegRegularizer()],
                                progress_bar=False)
        runs.append((c.detach().clone(), yh.detach().clone()))
    assert len(calls) == 1
    (ca, ya), (cb, yb) = runs
    assert tr.equal(ca, cb) and tr.equal(ya, yb)
    assert tuple(ya.shape) == case.shape
    want = np.asarray(ora.forward(*ref.segs, ca.cpu().numpy(), ref.n_vox)).reshape(case.shape)
    _fwd_close(ya, want, gc.F64_RTOL, f'{name} returned forward')
    assert not tr.equal(ca, tr.ones_like(ca))
