"""Host side of the matrix-free pair (sphrt_trace_backproject_f64, back_project,
MatrixFreeOperator): the entry is declared, exported and bound; its refusals fire on the host,
before any device call; the Python layer raises without a GPU, and raises layout errors before it
looks for one.  (No compute call: no GPU here.)"""
import ctypes
import os
import re

import pytest
import torch as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'sphrt_trace_backproject_f64'


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
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args == 11
    # next to the no-store forward in the header
    assert hdr.index('sphrt_trace_integrate_f64') < hdr.index(ENTRY)
    import sph_raytracer_amd as pkg
    from sph_raytracer_amd import raytracer as rt
    assert pkg.MatrixFreeOperator is rt.MatrixFreeOperator and pkg.back_project is rt.back_project
    assert {'MatrixFreeOperator', 'back_project'} <= set(pkg.__all__)
    for name in ('regs', 'lens', 'segments', 'plot'):
        assert not hasattr(rt.MatrixFreeOperator, name)


def _host_plan(grid):
    """A plan over host 'tables' (sphrt_plan_create_external never touches them): enough for the
    checks that read the plan's grid, no device needed."""
    from sph_raytracer_amd import raytracer as rt
    stg = rt._Staging()
    plan = rt._Plan(grid, tr.device('cuda', 0), staging=stg)
    stg.upload('cpu')
    plan.attach(stg)
    return plan, stg


def test_backproject_refusals_on_the_host():
    """Null pointers, n_chan < 1, ray_chan_div > 0 with several channels, strides that would
    write or read past the buffers and a short or missing workspace: each refused with a message
    in sphrt_last_error, before the library asks for a device."""
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

    def call(plan=h, rays=ctypes.byref(rays), y=p, n_chan=1, ycs=n, div=0, acc=p, cs=vol, ws=p,
             ws_size=need):
        return fn(plan, rays, y, n_chan, ycs, div, acc, cs, ws, ws_size, None)

    cases = [
        (lambda: call(plan=None), b'null plan'),
        (lambda: call(rays=None), b'null ray batch'),
        (lambda: call(y=None), b'null'),
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
    # the same checks as the no-store forward's
    assert lib.sphrt_trace_integrate_f64(h, ctypes.byref(rays), p, 0, vol, 0, p, n, p, need,
                                         None) != 0


def _case():
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    return SphericalGrid((4, 4, 4)), ConeRectGeom((4, 5), (5, 0, 0))


def test_no_cpu_fallback_matrix_free():
    """test_no_cpu_fallback's rule: without a GPU the matrix-free pair fails loudly."""
    if tr.cuda.is_available():
        pytest.skip('GPU present')
    from sph_raytracer_amd import MatrixFreeOperator, back_project
    grid, geom = _case()
    with pytest.raises(RuntimeError, match='GPU'):
        back_project(grid, geom, tr.ones(geom.shape))
    with pytest.raises(RuntimeError, match='GPU'):
        MatrixFreeOperator(grid, geom)(tr.ones(grid.shape))
    with pytest.raises(RuntimeError, match='GPU'):
        MatrixFreeOperator(grid, geom, device='cuda')


def test_reference_modes_are_refused():
    """ftype=float32 / invalid=True: NotImplementedError naming Operator, before any device."""
    from sph_raytracer_amd import MatrixFreeOperator
    grid, geom = _case()
    for kw in (dict(ftype=tr.float32), dict(invalid=True)):
        with pytest.raises(NotImplementedError, match='Operator'):
            MatrixFreeOperator(grid, geom, **kw)


def test_layout_errors_before_any_device(monkeypatch):
    """A wrong trailing shape, an unpairable T and a dynamic grid without time slices are raised
    before the device is looked for (require_gpu is never reached)."""
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid, _lib, back_project
    from sph_raytracer_amd.raytracer import _adjoint_layout

    def never(*a, **k):
        raise AssertionError('a layout error must come before the device')

    monkeypatch.setattr(_lib, 'require_gpu', never)
    grid, geom = _case()
    with pytest.raises(ValueError, match='ray shape'):
        back_project(grid, geom, tr.ones(4, 6))
    with pytest.raises(ValueError, match='ray shape'):
        back_project(grid, geom, tr.ones(5))
    dyn = SphericalGrid((5, 4, 4, 4))
    coll = sum(ConeRectGeom((4, 5), (5, 0, k)) for k in range(5))
    assert tuple(coll.shape) == (5, 4, 5)
    with pytest.raises(ValueError, match='cannot pair'):
        back_project(dyn, coll, tr.ones(3, 4, 5))
    with pytest.raises(ValueError, match='do not match'):
        back_project(dyn, coll, tr.ones(5, 4, 6))
    with pytest.raises(NotImplementedError):
        back_project(dyn, coll, tr.ones(5, 4, 5), time_slices=False)
    # the rules of _layout_for, read backwards
    assert _adjoint_layout(grid, (4, 5), (4, 5)) == (1, 0, (4, 4, 4))
    assert _adjoint_layout(grid, (4, 5), (3, 4, 5)) == (3, 0, (3, 4, 4, 4))
    assert _adjoint_layout(grid, (4, 5), (2, 2, 4, 5)) == (4, 0, (2, 2, 4, 4, 4))
    assert _adjoint_layout(dyn, (5, 4, 5), (5, 4, 5)) == (1, 20, (5, 4, 4, 4))
    assert _adjoint_layout(dyn, (4, 5), (5, 4, 5)) == (5, 0, (5, 4, 4, 4))
