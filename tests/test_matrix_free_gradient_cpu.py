"""Host side of the fused residual back-projection (sphrt_trace_normal_f64,
MatrixFreeOperator.residual_gradient, retrieval._fused_plan): the entry is declared, exported and
bound; its refusals fire on the host, before any device call; the Python layer raises layout
errors before it looks for a device; _direct_plan keeps declining what is not an Operator.  (No
compute call: no GPU here.)"""
import ctypes
import os
import re

import pytest
import torch as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'sphrt_trace_normal_f64'


def test_entry_declared_exported_and_bound():
    from sph_raytracer_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, 'include', 'sphrt.h')).read()
    m = re.search(r'int\s+' + ENTRY + r'\s*\(([^;]*)\)\s*;', hdr)
    assert m, f'{ENTRY} is not declared in include/sphrt.h'
    n_args = len(m.group(1).split(','))
    assert ENTRY in _lib.EXPORTED
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), ENTRY)
    fn = getattr(_lib.load(), ENTRY)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args == 14
    assert fn.argtypes[4] is ctypes.c_double            # scale, by value
    # after the no-store adjoint in the header, and saying what it replaces
    decl = re.search(r'int\s+sphrt_trace_backproject_f64\s*\(', hdr)
    assert decl and decl.start() < m.start()
    comment = hdr[decl.start():m.start()]
    assert 'Operator.__call__' in comment and 'Operator.T' in comment
    assert 'raytracer.py:692-748' in comment
    from sph_raytracer_amd import raytracer as rt
    assert callable(rt.MatrixFreeOperator.residual_gradient)


def _host_plan(grid):
    """A plan over host 'tables' (sphrt_plan_create_external never touches them): enough for the
    checks that read the plan's grid, no device needed (as tests/test_matrix_free_cpu.py)."""
    from sph_raytracer_amd import raytracer as rt
    stg = rt._Staging()
    plan = rt._Plan(grid, tr.device('cuda', 0), staging=stg)
    stg.upload('cpu')
    plan.attach(stg)
    return plan, stg


def test_normal_refusals_on_the_host():
    """A null plan, ray batch, density, m, yhat or acc, n_chan < 1, ray_chan_div > 0 with several
    channels, strides that would read or write past the buffers and a short or missing workspace:
    each refused with its word in sphrt_last_error, before the library asks for a device."""
    from sph_raytracer_amd import SphericalGrid, _lib
    lib = _lib.load()
    fn = getattr(lib, ENTRY)
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
    assert need > 0
    h = plan.handle

    def call(plan=h, rays=ctypes.byref(rays), d=p, m=p, scale=0.5, n_chan=1, cs=vol, div=0,
             yhat=p, ycs=n, acc=p, ws=p, ws_size=need):
        return fn(plan, rays, d, m, scale, n_chan, cs, div, yhat, ycs, acc, ws, ws_size, None)

    cases = [
        (lambda: call(plan=None), b'null plan'),
        (lambda: call(rays=None), b'null ray batch'),
        (lambda: call(d=None), b'null'),
        (lambda: call(m=None), b'null'),
        (lambda: call(yhat=None), b'null'),
        (lambda: call(acc=None), b'null'),
        (lambda: call(n_chan=0), b'n_chan'),
        (lambda: call(n_chan=-2), b'n_chan'),
        (lambda: call(n_chan=3, div=5), b'ray_chan_div'),
        (lambda: call(cs=vol - 1), b'chan_stride'),
        (lambda: call(n_chan=2, ycs=n - 1), b'y_chan_stride'),
        (lambda: call(ws_size=need - 1), b'workspace too small'),
        (lambda: call(ws_size=0), b'workspace too small'),
        (lambda: call(ws=None), b'workspace too small'),
    ]
    for i, (run, word) in enumerate(cases):
        assert run() != 0, i
        assert word in lib.sphrt_last_error(), (i, lib.sphrt_last_error())
    for arg in ('d', 'm', 'yhat', 'acc'):      # the message names the entry's own buffers
        assert call(**{arg: None}) != 0 and b'density, m, yhat or acc' in lib.sphrt_last_error()


def _operator(grid, geom):
    """A MatrixFreeOperator as far as the host goes (its constructor needs a GPU for the plan and
    the ray batch): what residual_gradient reads before it touches them."""
    from sph_raytracer_amd import MatrixFreeOperator
    op = object.__new__(MatrixFreeOperator)
    op.grid, op.geom, op._ray_shape = grid, geom, tuple(geom.shape)
    return op


def test_layout_errors_before_any_device(monkeypatch):
    """Measurements that are not line integrals of these rays, a density that is not the one they
    are the output of and an unpairable T are raised before the device is looked for (require_gpu
    is never reached, and neither are the operator's device parts)."""
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid, _lib
    from sph_raytracer_amd.raytracer import _gradient_layout

    def never(*a, **k):
        raise AssertionError('a layout error must come before the device')

    monkeypatch.setattr(_lib, 'require_gpu', never)
    grid, geom = SphericalGrid((4, 4, 4)), ConeRectGeom((4, 5), (5, 0, 0))
    op = _operator(grid, geom)
    x = tr.ones(4, 4, 4)
    with pytest.raises(ValueError, match='ray shape'):
        op.residual_gradient(x, tr.ones(4, 6))
    with pytest.raises(ValueError, match='ray shape'):
        op.residual_gradient(x, tr.ones(5))
    with pytest.raises(ValueError, match='density of shape'):
        op.residual_gradient(x, tr.ones(3, 4, 5))
    with pytest.raises(ValueError, match='density of shape'):
        op.residual_gradient(tr.ones(3, 4, 4, 4), tr.ones(4, 5), scale=2.0)
    with pytest.raises(ValueError, match='density of shape'):
        op.residual_gradient(tr.ones(4, 4, 5), tr.ones(4, 5))
    dyn = SphericalGrid((5, 4, 4, 4))
    coll = sum(ConeRectGeom((4, 5), (5, 0, k)) for k in range(5))
    assert tuple(coll.shape) == (5, 4, 5)
    dop = _operator(dyn, coll)
    with pytest.raises(ValueError, match='cannot pair'):
        dop.residual_gradient(tr.ones(3, 4, 4, 4), tr.ones(3, 4, 5))
    with pytest.raises(ValueError, match='do not match'):
        dop.residual_gradient(tr.ones(5, 4, 4, 4), tr.ones(5, 4, 6))
    with pytest.raises(ValueError, match='density of shape'):
        dop.residual_gradient(tr.ones(4, 4, 4), tr.ones(5, 4, 5))
    with pytest.raises(ValueError, match='density of shape'):
        dop.residual_gradient(tr.ones(5, 4, 4, 5), tr.ones(5, 4, 5))
    # the forward's layout rules, with the measurements held to its output shape
    assert _gradient_layout(grid, (4, 5), (4, 4, 4), (4, 5)) == (1, 0, (4, 5))
    assert _gradient_layout(grid, (4, 5), (2, 2, 4, 4, 4), (2, 2, 4, 5)) == (4, 0, (2, 2, 4, 5))
    assert _gradient_layout(dyn, (5, 4, 5), (5, 4, 4, 4), (5, 4, 5)) == (1, 20, (5, 4, 5))
    assert _gradient_layout(dyn, (4, 5), (5, 4, 4, 4), (5, 4, 5)) == (5, 0, (5, 4, 5))


def test_direct_plan_still_declines_what_is_not_an_operator():
    """_direct_plan is for a stored Operator only (test_gd_with_matrix_free_operator relies on
    it); _fused_plan is for a MatrixFreeOperator on a static grid only."""
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid, retrieval
    from sph_raytracer_amd.loss import SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom = SphericalGrid((4, 4, 4)), ConeRectGeom((4, 5), (5, 0, 0))
    model, sq = FullyDenseModel(grid), SquareLoss()
    c, y = tr.ones(4, 4, 4, dtype=tr.float64), tr.ones(4, 5, dtype=tr.float64)
    op = _operator(grid, geom)
    op.dynamic, op._cdev = False, tr.device('cuda', 0)
    assert retrieval._direct_plan(op, y, model, c, [sq], [c]) is None
    assert retrieval._direct_plan(lambda d: d, y, model, c, [sq], [c]) is None
    assert retrieval._fused_plan(lambda d: d, y, model, c, [sq], [c]) is None
    assert retrieval._fused_plan(op, None, model, c, [sq], [c]) is None
    assert retrieval._fused_plan(op, y, model, c, [sq], [c]) is None     # (host coefficients)
    op.dynamic = True
    assert retrieval._fused_plan(op, y, model, c, [sq], [c]) is None
