"""Host side of weighted least squares (sphrt_trace_normal_weighted_f64 / _fixed_f64,
sphrt_wsq_residual_f64, MatrixFreeOperator.residual_gradient(weights=...)): the entries are
declared, exported and bound; their refusals fire on the host; weights that do not broadcast to
the measurements are refused before any device is looked for.  (No compute call: no GPU here.
retrieval._loop_terms asks for coefficients on a GPU before it looks at a mask, so its mask
conditions are in tests/test_gpu_weighted_gradient.py.)"""
import ctypes
import os
import re

import pytest
import torch as tr

from test_matrix_free_gradient_cpu import _host_plan, _operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'sphrt_trace_normal_weighted_f64': 14, 'sphrt_trace_normal_weighted_fixed_f64': 15,
           'sphrt_wsq_residual_f64': 10}


def test_entries_declared_exported_and_bound():
    from sph_raytracer_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, 'include', 'sphrt.h')).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for entry, n_args in ENTRIES.items():
        m = re.search(r'int\s+' + entry + r'\s*\(([^;]*)\)\s*;', hdr)
        assert m, f'{entry} is not declared in include/sphrt.h'
        assert len(m.group(1).split(',')) == n_args
        assert 'const double *ray_scale' in m.group(1)
        assert entry in _lib.EXPORTED and hasattr(raw, entry)
        fn = getattr(_lib.load(), entry)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
        assert ctypes.c_double not in fn.argtypes        # no scalar factor: ray_scale, a pointer
    # the unweighted entries keep their signatures (scale by value, 14 and 15 arguments)
    lib = _lib.load()
    assert len(lib.sphrt_trace_normal_f64.argtypes) == 14
    assert len(lib.sphrt_trace_normal_fixed_f64.argtypes) == 15
    assert lib.sphrt_trace_normal_f64.argtypes[4] is ctypes.c_double
    assert len(lib.sphrt_sq_residual_f64.argtypes) == 9
    # the header states the fixed-point bound of the weighted entry
    fixed = hdr[hdr.index('Replaces sphrt_trace_normal_weighted_f64'):
                hdr.index('int sphrt_trace_normal_weighted_fixed_f64')]
    assert 'max|ray_scale|' in fixed and 'fa = S * L * L' in fixed and 'fb = S * L' in fixed


def test_weighted_normal_refusals_on_the_host():
    """sphrt_trace_normal_f64's refusals and a null ray_scale, for both entries (and the fixed
    one's null record), each with its word in sphrt_last_error before the library asks for a
    device."""
    from sph_raytracer_amd import SphericalGrid, _lib
    lib = _lib.load()
    grid = SphericalGrid(shape=(4, 5, 6))
    plan, _keep = _host_plan(grid)
    vol, n = 4 * 5 * 6, 10
    rays = _lib.RayBatch()
    rays.ndim = 1
    rays.shape[0] = n
    rays.xs_stride[0] = rays.rays_stride[0] = 3
    p = ctypes.c_void_p(16)      # never dereferenced: every call below fails its checks first
    rays.xs = rays.rays = rays.start = 16
    need = lib.sphrt_trace_workspace_bytes(plan.handle, n)
    h = plan.handle

    def call(fixed, plan=h, rays=ctypes.byref(rays), d=p, m=p, rs=p, n_chan=1, cs=vol, div=0,
             yhat=p, ycs=n, acc=p, rec=p, ws=p, ws_size=need):
        if fixed:
            return lib.sphrt_trace_normal_weighted_fixed_f64(
                plan, rays, d, m, rs, n_chan, cs, div, yhat, ycs, acc, rec, ws, ws_size, None)
        return lib.sphrt_trace_normal_weighted_f64(
            plan, rays, d, m, rs, n_chan, cs, div, yhat, ycs, acc, ws, ws_size, None)

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
        for i, (kw, word) in enumerate(cases):
            assert call(fixed, **kw) != 0, (fixed, i)
            assert word in lib.sphrt_last_error(), (fixed, i, lib.sphrt_last_error())
    assert call(True, rec=None) != 0 and b'null scale record' in lib.sphrt_last_error()


def test_wsq_residual_refusals_on_the_host():
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    p, none = ctypes.c_void_p(16), None
    fn = lib.sphrt_wsq_residual_f64
    assert fn(p, p, 1, 0, p, p, none, p, p, none) != 0 and b'empty' in lib.sphrt_last_error()
    for k in (0, 1, 4, 5, 7, 8):          # yhat, y, ray_scale, weight, r_scaled, partial_sums
        args = [p, p, 1, 8, p, p, none, p, p, none]
        args[k] = none
        assert fn(*args) != 0 and b'null' in lib.sphrt_last_error(), k


def test_weights_that_do_not_broadcast_are_refused_before_any_device(monkeypatch):
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid, _lib

    def never(*a, **k):
        raise AssertionError('a weights error must come before the device')

    monkeypatch.setattr(_lib, 'require_gpu', never)
    grid, geom = SphericalGrid((4, 4, 4)), ConeRectGeom((4, 5), (5, 0, 0))
    op = _operator(grid, geom)
    x, m = tr.ones(4, 4, 4), tr.ones(4, 5)
    for shape in ((4, 6), (5, 4), (3,), (2, 4, 5), (1, 4, 5)):
        with pytest.raises(ValueError, match='do not broadcast'):
            op.residual_gradient(x, m, 0.5, weights=tr.ones(shape))
    with pytest.raises(ValueError, match='do not broadcast'):
        op.residual_gradient(tr.ones(3, 4, 4, 4), tr.ones(3, 4, 5), weights=tr.ones(2, 4, 5))
    with pytest.raises(TypeError, match='bool, float32 or float64'):
        op.residual_gradient(x, m, weights=tr.ones(4, 5, dtype=tr.int32))
