"""Host side of the robust fidelity terms (sphrt_trace_normal_robust_f64 / _fixed_f64,
sphrt_robust_residual_f64, MatrixFreeOperator.residual_gradient(loss=..., delta=...),
loss.HuberLoss): the entries are declared, exported and bound; their refusals fire on the host;
HuberLoss over the oracle-backed CpuOperator equals a hand-written piecewise formula, value and
gradient; bad loss / delta / weights arguments are refused before any device is looked for.  (No
compute call of the library: no GPU here.  retrieval._loop_terms asks for coefficients on a GPU
before it looks at a loss term, so its conditions are in tests/test_gpu_robust_gradient.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch as tr

from test_matrix_free_gradient_cpu import _host_plan, _operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'sphrt_trace_normal_robust_f64': 16, 'sphrt_trace_normal_robust_fixed_f64': 17,
           'sphrt_robust_residual_f64': 12}
ABS, HUBER = 1, 2
BAD_DELTAS = (0.0, -1.0, float('inf'), -float('inf'), float('nan'))


def test_entries_declared_exported_and_bound():
    from sph_raytracer_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, 'include', 'sphrt.h')).read()
    assert re.search(r'#define\s+SPHRT_RESID_ABS\s+1\b', hdr)
    assert re.search(r'#define\s+SPHRT_RESID_HUBER\s+2\b', hdr)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for entry, n_args in ENTRIES.items():
        m = re.search(r'int\s+' + entry + r'\s*\(([^;]*)\)\s*;', hdr)
        assert m, f'{entry} is not declared in include/sphrt.h'
        assert len(m.group(1).split(',')) == n_args
        assert 'const double *ray_scale' in m.group(1)
        assert re.search(r'int kind,\s*double delta', m.group(1))
        assert entry in _lib.EXPORTED and hasattr(raw, entry)
        fn = getattr(_lib.load(), entry)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
        # one int and one double by value, next to each other: kind, delta
        k = fn.argtypes.index(ctypes.c_double)
        assert fn.argtypes[k - 1] is ctypes.c_int and fn.argtypes.count(ctypes.c_double) == 1
    # the weighted and unweighted entries keep their signatures
    lib = _lib.load()
    assert len(lib.sphrt_trace_normal_weighted_f64.argtypes) == 14
    assert len(lib.sphrt_trace_normal_weighted_fixed_f64.argtypes) == 15
    assert len(lib.sphrt_wsq_residual_f64.argtypes) == 10
    assert len(lib.sphrt_trace_normal_f64.argtypes) == 14
    # the header states the fixed-point bound of the robust entry and its caveat
    fixed = hdr[hdr.index('Replaces sphrt_trace_normal_robust_f64'):
                hdr.index('int sphrt_trace_normal_robust_fixed_f64')]
    assert 'a = ray_scale' in fixed and 'fa = L for ABS' in fixed and 'delta * L' in fixed
    assert '2^32 times the bound' in fixed


def _trace_call(lib):
    from sph_raytracer_amd import SphericalGrid, _lib
    grid = SphericalGrid(shape=(4, 5, 6))
    plan, keep = _host_plan(grid)
    vol, n = 4 * 5 * 6, 10
    rays = _lib.RayBatch()
    rays.ndim = 1
    rays.shape[0] = n
    rays.xs_stride[0] = rays.rays_stride[0] = 3
    p = ctypes.c_void_p(16)      # never dereferenced: every call below fails its checks first
    rays.xs = rays.rays = rays.start = 16
    need = lib.sphrt_trace_workspace_bytes(plan.handle, n)
    h = plan.handle

    def call(fixed, kind=ABS, delta=0.0, plan=h, rays=ctypes.byref(rays), d=p, m=p, rs=p,
             n_chan=1, cs=vol, div=0, yhat=p, ycs=n, acc=p, rec=p, ws=p, ws_size=need):
        if fixed:
            return lib.sphrt_trace_normal_robust_fixed_f64(
                plan, rays, d, m, rs, kind, delta, n_chan, cs, div, yhat, ycs, acc, rec, ws,
                ws_size, None)
        return lib.sphrt_trace_normal_robust_f64(
            plan, rays, d, m, rs, kind, delta, n_chan, cs, div, yhat, ycs, acc, ws, ws_size, None)

    return call, (plan, keep, rays), vol, n, need


def test_robust_normal_refusals_on_the_host():
    """The weighted entry's refusals, an unknown kind and a Huber delta that is not finite and
    > 0, for both entries and both kinds (and the fixed one's null record), each with its word in
    sphrt_last_error before the library asks for a device."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    call, _keep, vol, n, need = _trace_call(lib)
    cases = [
        (dict(plan=None), b'null plan'),
        (dict(rays=None), b'null ray batch'),
        (dict(d=None), b'density, m, yhat or acc'),
        (dict(m=None), b'density, m, yhat or acc'),
        (dict(yhat=None), b'density, m, yhat or acc'),
        (dict(acc=None), b'density, m, yhat or acc'),
        (dict(rs=None), b'null ray_scale'),
        (dict(n_chan=0), b'n_chan'),
        (dict(n_chan=3, div=5), b'ray_chan_div'),
        (dict(cs=vol - 1), b'chan_stride'),
        (dict(n_chan=2, ycs=n - 1), b'y_chan_stride'),
        (dict(ws_size=need - 1), b'workspace too small'),
        (dict(ws=None), b'workspace too small'),
    ]
    for fixed in (False, True):
        for kind, delta in ((ABS, 0.0), (ABS, float('nan')), (HUBER, 0.5)):
            for i, (kw, word) in enumerate(cases):
                assert call(fixed, kind, delta, **kw) != 0, (fixed, kind, i)
                assert word in lib.sphrt_last_error(), (fixed, kind, i, lib.sphrt_last_error())
        for kind in (0, 3, -1, 7):
            assert call(fixed, kind, 0.5) != 0
            assert b'unknown residual kind' in lib.sphrt_last_error()
        for delta in BAD_DELTAS:
            assert call(fixed, HUBER, delta) != 0, delta
            assert b'delta' in lib.sphrt_last_error()
    assert call(True, HUBER, 0.5, rec=None) != 0 and b'null scale record' in lib.sphrt_last_error()
    assert call(True, ABS, 0.0, rec=None) != 0 and b'null scale record' in lib.sphrt_last_error()


def test_robust_residual_refusals_on_the_host():
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    p, none = ctypes.c_void_p(16), None
    fn = lib.sphrt_robust_residual_f64
    for kind, delta in ((ABS, 0.0), (HUBER, 0.25)):
        assert fn(p, p, 1, 0, kind, delta, p, p, none, p, p, none) != 0
        assert b'empty' in lib.sphrt_last_error()
        for k in (0, 1, 6, 7, 9, 10):     # yhat, y, ray_scale, weight, r_scaled, partial_sums
            args = [p, p, 1, 8, kind, delta, p, p, none, p, p, none]
            args[k] = none
            assert fn(*args) != 0 and b'null' in lib.sphrt_last_error(), k
    for kind in (0, 3, -2):
        assert fn(p, p, 1, 8, kind, 0.5, p, p, none, p, p, none) != 0
        assert b'unknown residual kind' in lib.sphrt_last_error()
    for delta in BAD_DELTAS:
        assert fn(p, p, 1, 8, HUBER, delta, p, p, none, p, p, none) != 0, delta
        assert b'delta' in lib.sphrt_last_error()


def _huber_by_hand(r, delta):
    a = np.abs(r)
    return np.where(a < delta, 0.5 * r * r, delta * (a - 0.5 * delta))


@pytest.mark.parametrize('ydt', [tr.float64, tr.float32], ids=['y64', 'y32'])
def test_huber_loss_value_and_gradient_by_hand(ydt):
    """HuberLoss over the oracle-backed CpuOperator: lam * mean(mask * h(f(d) - y)) and its
    gradient A^T((lam / N) * mask * clamp(f(d) - y, +-delta)), both written out in numpy."""
    from cpu_operator import CpuOperator
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    from sph_raytracer_amd.loss import HuberLoss, Loss
    grid, geom = SphericalGrid(shape=(6, 5, 8)), ConeRectGeom((9, 7), pos=(5, 0.3, 1), fov=(25, 25))
    op = CpuOperator(grid, geom)
    g = tr.Generator().manual_seed(5)
    d = tr.rand(grid.shape, dtype=tr.float64, generator=g)
    y = (op(d).detach() + tr.randn(geom.shape, dtype=tr.float64, generator=g) * 0.4).to(ydt)
    mask = tr.rand(geom.shape, dtype=tr.float64, generator=g) * 2 - 0.5
    mask[0, :3] = 0
    delta, lam = 0.3, 2.5
    r = op(d).detach().numpy() - y.double().numpy()
    inner = float((np.abs(r) < delta).mean())
    assert 0.2 < inner < 0.8, inner                         # both branches
    for pm, m_np in ((mask, mask.numpy()), (1, np.ones(r.shape))):
        fn = lam * HuberLoss(delta=delta, projection_mask=pm)
        assert isinstance(fn, Loss) and fn.kind == 'fidelity' and fn.delta == delta
        dd = d.clone().requires_grad_()
        val = fn(op, y, dd, None)
        assert val.dtype == tr.float64
        want = lam * np.mean(m_np * _huber_by_hand(r, delta))
        assert abs(float(val.detach()) - want) <= 1e-14 * abs(want)
        val.backward()
        back = (lam / r.size) * m_np * np.clip(r, -delta, delta)
        gw = op.T(tr.from_numpy(back)).numpy()
        err = np.abs(dd.grad.numpy() - gw).max()
        assert err <= 1e-13 * np.abs(gw).max(), err
    # the default delta is 1; a delta that is not finite and > 0 is refused
    assert HuberLoss().delta == 1.0 and HuberLoss(volume_mask=2).volume_mask == 2
    assert HuberLoss(delta=np.float32(0.5)).delta == 0.5 and type(HuberLoss(delta=2).delta) is float
    for bad in (0, -1.0, float('inf'), float('nan'), None, True, '1', tr.tensor(0.5)):
        with pytest.raises(ValueError, match='delta'):
            HuberLoss(delta=bad)


def test_distributed_gd_keeps_robust_terms_out_of_its_direct_loop():
    """distributed.gd's pre-filter: only unmasked terms that are not robust reach _direct_plan."""
    from sph_raytracer_amd.distributed import _declined
    from sph_raytracer_amd.loss import AbsLoss, HuberLoss, NegRegularizer, SquareLoss
    assert not _declined([SquareLoss(), NegRegularizer()]) and not _declined([0.5 * SquareLoss()])
    assert _declined([AbsLoss()]) and _declined([HuberLoss(delta=0.5), NegRegularizer()])
    assert _declined([NegRegularizer(), 2 * AbsLoss()])
    assert _declined([SquareLoss(projection_mask=tr.ones(3))])


def test_bad_loss_arguments_are_refused_before_any_device(monkeypatch):
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid, _lib

    def never(*a, **k):
        raise AssertionError('an argument error must come before the device')

    monkeypatch.setattr(_lib, 'require_gpu', never)
    grid, geom = SphericalGrid((4, 4, 4)), ConeRectGeom((4, 5), (5, 0, 0))
    op = _operator(grid, geom)
    x, m = tr.ones(4, 4, 4), tr.ones(4, 5)
    for loss in ('l1', 'Abs', '', None, 1, ['abs'], {'huber': 1}):
        with pytest.raises(ValueError, match="'square', 'abs' or 'huber'"):
            op.residual_gradient(x, m, loss=loss)
    with pytest.raises(ValueError, match='needs a finite delta > 0'):
        op.residual_gradient(x, m, loss='huber')
    for bad in (0, 0.0, -0.5, float('inf'), float('nan'), True, tr.tensor(0.5)):
        with pytest.raises(ValueError, match='needs a finite delta > 0'):
            op.residual_gradient(x, m, loss='huber', delta=bad)
    # a real number is a delta, whatever its type (a tensor is not: reading it could sync)
    from sph_raytracer_amd.raytracer import _robust_args
    for good in (0.5, 1, np.float32(0.5), np.float64(0.5), np.int64(2)):
        assert _robust_args('huber', good) == (HUBER, float(good))
    assert _robust_args('abs', None) == (ABS, 0.0) and _robust_args('square', None) is None
    for loss in ('square', 'abs'):
        with pytest.raises(ValueError, match="delta belongs to loss='huber'"):
            op.residual_gradient(x, m, loss=loss, delta=0.5)
    for loss, kw in (('abs', {}), ('huber', dict(delta=0.5))):
        for shape in ((4, 6), (5, 4), (3,), (1, 4, 5)):
            with pytest.raises(ValueError, match='do not broadcast'):
                op.residual_gradient(x, m, 0.5, weights=tr.ones(shape), loss=loss, **kw)
        with pytest.raises(TypeError, match='bool, float32 or float64'):
            op.residual_gradient(x, m, weights=tr.ones(4, 5, dtype=tr.int32), loss=loss, **kw)
        with pytest.raises(ValueError, match='ray shape'):
            op.residual_gradient(x, tr.ones(4, 6), loss=loss, **kw)
