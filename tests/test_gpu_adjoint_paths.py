"""Every path of the adjoint (Operator.T, the autograd backward, T(time_slices=True)) against an
independent reference, with spies that say which path ran.

Paths: the general transposed adjoint (the voxel-major CSR's forward), its steady-state bindings
in the CPython entry (_fastc_T; _fastc_A for the time-paired gradient of a dynamic grid), and the
float64-atomic kernel (sphrt_adjoint_accumulate: adjoint_mode = 'atomic', and the fallback of a
view <-> time pairing without a time-paired CSR).  adjoint_mode is read on every call: the
bindings serve 'transpose' only and stay bound while 'atomic' is set.

Reference: the C oracle's own trace of the same grid and rays (oracle.trace_segments, never
op.segments()) and a float64 numpy accumulate over it (oracle.adjoint per channel; for the
ray // div time pairing, over the columns (ray // div) * vol + voxel, the way oracle.forward
reads its channels).

Tolerances (the project's own): float64 adjoint within 1e-10 x max|reference|
(test_gpu_fuzz.py), float32 within 1e-5 x max|reference|; atomic against transposed in float64
within 1e-12 (rtol, and atol 1e-12 x max: test_gpu_properties.py); repeated calls in 'transpose'
mode bitwise equal.

Which path ran: a counting wrapper over _lib.load().sphrt_adjoint_accumulate (raytracer.py looks
the entry up per call) and a wrapper over the instance attribute op._fastfn that records the
capsule of every call (_fastc, _fastc_T, _fastc_A) and whether it returned a tensor.

Geometries: the smallest at which the paths still differ; every case asserts, on the reference
alone, that at least half its rays cross the grid and at least half its voxels (columns) are
touched, and the property of the trace that selects its path."""
import math

import numpy as np
import pytest
import torch as tr

pytestmark = pytest.mark.gpu

F64, F32 = tr.float64, tr.float32
TOL = {F64: 1e-10, F32: 1e-5}
SGRID, DGRID, T_DYN = (12, 10, 14), (5, 12, 10, 16), 5


def _orbit(n):
    return [(5 * tr.cos(th), 5 * tr.sin(th), 1) for th in tr.linspace(0, 2 * tr.pi, n)]


class _Ref:
    """The oracle's trace of (grid, geom) and float64 accumulates over it."""

    def __init__(self, grid, geom):
        from oracle import oracle
        from sph_raytracer_amd.raytracer import find_starts
        oracle.use_mkl_sqrt(False)
        self.oracle = oracle
        g = oracle.Grid.from_boundaries(grid.r_b.numpy(), grid.e_b.numpy(), grid.a_b.numpy())
        xs, rays = geom.ray_starts, geom.rays
        self.ptr, self.vox, self.seg = oracle.trace_segments(
            g, xs.numpy(), rays.numpy(), find_starts(grid, xs).numpy())
        self.n = len(self.ptr) - 1
        self.vol = math.prod(grid.shape[-3:])
        self.ray = np.repeat(np.arange(self.n), np.diff(self.ptr))

    def coverage(self, div=0, n_t=1):
        """(fraction of rays with a segment, fraction of the columns touched)."""
        cols = self.vox if not div else (self.ray // div) * self.vol + self.vox
        return (float((np.diff(self.ptr) > 0).mean()),
                np.unique(cols).size / (n_t * self.vol))

    def adjoint(self, y, n_chan=1, div=0, n_t=1):
        """y (n_chan, n) -> (n_chan, vol); with div, y (n,) -> (n_t, vol): ray r into time
        slice r // div."""
        y = y.detach().cpu().double().numpy().reshape(n_chan, self.n)
        if div:
            cols = (self.ray // div) * self.vol + self.vox
            return self.oracle.adjoint(self.ptr, cols, self.seg, y[0],
                                       n_t * self.vol).reshape(n_t, self.vol)
        return np.stack([self.oracle.adjoint(self.ptr, self.vox, self.seg, yc, self.vol)
                         for yc in y])

    def forward(self, x, div=0):
        return np.asarray(self.oracle.forward(self.ptr, self.vox, self.seg,
                                              x.detach().cpu().double().numpy(), self.vol,
                                              ray_chan_div=div)).reshape(-1)


def _check_coverage(ref, **kw):
    hit, cov = ref.coverage(**kw)
    assert hit >= 0.5 and cov >= 0.5, (hit, cov)


def _assert_close(got, want, tol):
    got = got.detach().cpu().double().numpy().reshape(-1)
    want = np.asarray(want).reshape(-1)
    assert got.shape == want.shape
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert scale > 0 and err <= tol * scale, (err, scale)


def _assert_modes_agree(atomic, transposed, dt):
    if dt == F64:
        assert tr.allclose(atomic, transposed, rtol=1e-12,
                           atol=1e-12 * float(transposed.abs().max()))


class _Spy:
    """Counts the launches of the atomic entry point and records op._fastfn's calls as
    (capsule name, returned a tensor)."""

    def __init__(self, monkeypatch, op):
        from sph_raytracer_amd import _lib
        assert _lib.load_fast() is not None, 'the CPython fast path was not built'
        lib = _lib.load()
        real = lib.sphrt_adjoint_accumulate
        self.op, self.atomic, self.fast, self._inner = op, 0, [], None

        def counted(*args):
            self.atomic += 1
            return real(*args)

        def fastfn(capsule, arg):
            out = self._inner(capsule, arg)
            name = next(k for k in ('_fastc', '_fastc_T', '_fastc_A')
                        if getattr(op, k) is capsule)
            self.fast.append((name, out is not None))
            return out

        self._fastfn = fastfn
        monkeypatch.setattr(lib, 'sphrt_adjoint_accumulate', counted)

    def run(self, fn):
        """-> (fn(), atomic launches, the adjoint bindings' calls).  (A first binding sets
        op._fastfn: the wrapper goes back on before every call.)"""
        cur = self.op.__dict__.get('_fastfn')
        if cur is not None and cur is not self._fastfn:
            self._inner, self.op._fastfn = cur, self._fastfn
        self.atomic, self.fast = 0, []
        out = fn()
        return out, self.atomic, [f for f in self.fast if f[0] != '_fastc']


def _rand(shape, dt, seed, gpu):
    return tr.rand(tuple(shape), dtype=dt, generator=tr.Generator().manual_seed(seed)).to(gpu)


# ---- static cases -------------------------------------------------------------------------------
def _static_geom(name):
    from sph_raytracer_amd import ConeCircGeom, ConeRectGeom
    if name == 'S1':
        return ConeRectGeom((24, 20), pos=(5, 0.3, 1), fov=(25, 25))
    if name == 'S2':
        return ConeCircGeom((12, 16), pos=(3, 1, 1), fov=(0, 45))
    if name == 'S3':
        return sum(ConeRectGeom((10, 12), pos=p, fov=(25, 25)) for p in _orbit(8))
    return sum(ConeCircGeom((12, 16), pos=p, fov=(0, 12)) for p in _orbit(8))


# name -> (the trace has another ray order than the geometry, the transposed CSR's columns are
# geometry rays): geometry-order trace; wedges with trace-row columns; view tiles with geometry
# columns; view tiles with trace-row columns
_SELECTS = {'S1': (False, False), 'S2': (True, False), 'S3': (True, True), 'S4': (True, False)}
_RAYS = {'S1': 480, 'S2': 192, 'S3': 960, 'S4': 1536}


@pytest.fixture(scope='module', params=sorted(_SELECTS))
def static_case(request):
    from sph_raytracer_amd import SphericalGrid
    name = request.param
    grid, geom = SphericalGrid(shape=SGRID), _static_geom(name)
    ref = _Ref(grid, geom)
    assert ref.n == _RAYS[name]
    _check_coverage(ref)
    return name, grid, geom, ref


def _static_op(case, gpu):
    from sph_raytracer_amd import Operator
    name, grid, geom, ref = case
    op = Operator(grid, geom, device=gpu)
    reordered, geom_cols = _SELECTS[name]
    assert (op._csr['ray_id'] is not None) == reordered
    assert op._tcols_geom() == geom_cols
    assert (op._adjoint_trace_order() is not None) == (reordered and not geom_cols)
    assert op._layout(grid.shape) == (1, 0, tuple(geom.shape))
    assert op._csr['n'] == ref.n
    return op


@pytest.mark.parametrize('dt', [F64, F32])
def test_static_mode_sequence(static_case, dt, gpu, monkeypatch):
    """'transpose' (general path, then _fastc_T), 'atomic' (sphrt_adjoint_accumulate once, no
    binding serves), 'transpose' again (the bound path, the earlier bits)."""
    name, grid, geom, ref = static_case
    op = _static_op(static_case, gpu)
    spy = _Spy(monkeypatch, op)
    y = _rand(geom.shape, dt, 1, gpu)
    want = ref.adjoint(y)
    try:
        assert op._fastc_T is None
        a0, n_at, fast = spy.run(lambda: op.T(y))
        assert n_at == 0 and not any(s for _, s in fast)         # the general path
        assert op._fastc_T is not None
        assert a0.shape == tuple(grid.shape) and a0.dtype == dt
        _assert_close(a0, want, TOL[dt])
        for _ in range(2):
            a, n_at, fast = spy.run(lambda: op.T(y))
            assert n_at == 0 and fast == [('_fastc_T', True)]
            assert tr.equal(a, a0)
        op.adjoint_mode = 'atomic'
        b, n_at, fast = spy.run(lambda: op.T(y))
        assert n_at == 1 and not any(s for _, s in fast)
        assert b.shape == a0.shape and b.dtype == dt
        _assert_close(b, want, TOL[dt])
        _assert_modes_agree(b, a0, dt)
        assert op._fastc_T is not None                            # (stays bound)
        op.adjoint_mode = 'transpose'
        c1, n_at1, _ = spy.run(lambda: op.T(y))
        c2, n_at2, fast = spy.run(lambda: op.T(y))
        assert n_at1 == 0 and n_at2 == 0 and fast == [('_fastc_T', True)]
        assert tr.equal(c1, a0) and tr.equal(c2, a0)
    finally:
        op.adjoint_mode = 'transpose'


@pytest.mark.parametrize('mode', ['transpose', 'atomic'])
def test_static_three_channels_autograd(static_case, mode, gpu, monkeypatch):
    """grad of (op(xc) * yc).sum() for xc of shape (3, ...): each channel against the reference;
    the atomic kernel with n_chan = 3 in 'atomic' mode, never in 'transpose'."""
    name, grid, geom, ref = static_case
    op = _static_op(static_case, gpu)
    spy = _Spy(monkeypatch, op)
    op.T(_rand(geom.shape, F64, 2, gpu))
    op.T(_rand(geom.shape, F64, 2, gpu))                          # (_fastc_T bound and used)
    try:
        op.adjoint_mode = mode
        for dt in (F64, F32):
            xc = _rand((3,) + tuple(grid.shape), dt, 3, gpu).requires_grad_()
            yc = _rand((3,) + tuple(geom.shape), dt, 4, gpu)
            grad, n_at, fast = spy.run(lambda: tr.autograd.grad((op(xc) * yc).sum(), xc)[0])
            assert n_at == (1 if mode == 'atomic' else 0) and not any(s for _, s in fast)
            assert grad.shape == xc.shape and grad.dtype == dt
            want = ref.adjoint(yc, n_chan=3)
            for c in range(3):
                _assert_close(grad[c], want[c], TOL[dt])
    finally:
        op.adjoint_mode = 'transpose'


@pytest.mark.parametrize('mode', ['transpose', 'atomic'])
def test_static_inputs_the_binding_declines(static_case, mode, gpu, monkeypatch):
    """y as a strided view, on the CPU, and as float64 for a float32 density: no binding serves
    (declined, or not tried), the result still meets the tolerance in both modes."""
    name, grid, geom, ref = static_case
    op = _static_op(static_case, gpu)
    spy = _Spy(monkeypatch, op)
    y = _rand(geom.shape, F64, 5, gpu)
    op.T(y)
    _, _, fast = spy.run(lambda: op.T(y))
    assert fast == [('_fastc_T', True)]                           # bound for y's shape and dtype
    n_want = 1 if mode == 'atomic' else 0
    try:
        op.adjoint_mode = mode
        shape = tuple(geom.shape)
        big = _rand(shape[:-1] + (2 * shape[-1] + 1,), F64, 6, gpu)
        yn = big[..., 1::2]
        assert yn.shape == y.shape and not yn.is_contiguous()
        got, n_at, fast = spy.run(lambda: op.T(yn))
        assert n_at == n_want and not any(s for _, s in fast)
        assert fast == ([('_fastc_T', False)] if mode == 'transpose' else [])
        _assert_close(got, ref.adjoint(yn), TOL[F64])
        yh = y.cpu()
        got, n_at, fast = spy.run(lambda: op.T(yh))
        assert n_at == n_want and not any(s for _, s in fast)
        assert got.device == gpu and got.dtype == F64
        _assert_close(got, ref.adjoint(y), TOL[F64])
        got, n_at, fast = spy.run(lambda: op._apply_adjoint(y, tuple(grid.shape), F32, gpu))
        assert n_at == n_want and fast == []
        assert got.dtype == F32 and got.shape == tuple(grid.shape)
        _assert_close(got, ref.adjoint(y), TOL[F32])
    finally:
        op.adjoint_mode = 'transpose'


# ---- dynamic cases ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dyn():
    """D: 5 views <-> 5 time slices; D1: the first of the views at every time step."""
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


def _dyn_op(dyn, device):
    from sph_raytracer_amd import Operator
    grid, geom, _, ref, _ = dyn
    op = Operator(grid, geom, dynamic=True, device=device)
    assert op._layout(DGRID) == (1, ref.n // T_DYN, tuple(geom.shape))
    assert op._layout((1,) + DGRID[1:]) == (1, 0, tuple(geom.shape))
    assert op._csr['n'] == ref.n
    return op, ref.n // T_DYN


def _backward(op, x, y):
    xg = x.clone().requires_grad_(True)
    (op(xg) * y).sum().backward()
    return xg.grad


def _paired_transpose(op, div):
    pt = op._paired(T_DYN, div)['transposed']['desc']
    assert pt.order & 4                       # dense output ranges
    return pt


@pytest.mark.parametrize('dt', [F64, F32])
def test_dynamic_mode_sequence(dyn, dt, gpu, monkeypatch):
    """The time-paired gradient through backward and T(time_slices=True): general path, then
    _fastc_A; 'atomic' launches the atomic kernel (div > 0) for both; 'transpose' again gives the
    bound path and the earlier bits."""
    grid, geom, _, ref, _ = dyn
    op, div = _dyn_op(dyn, 'cuda')
    spy = _Spy(monkeypatch, op)
    x, y = _rand(DGRID, dt, 7, gpu), _rand(geom.shape, dt, 8, gpu)
    want = ref.adjoint(y, div=div, n_t=T_DYN)
    try:
        g0, n_at, fast = spy.run(lambda: _backward(op, x, y))
        assert n_at == 0 and not any(s for _, s in fast)          # the general path
        assert op._fastc_A is not None and op._paired(T_DYN, div) is not None
        _paired_transpose(op, div)
        assert g0.shape == DGRID and g0.dtype == dt
        _assert_close(g0, want, TOL[dt])
        for _ in range(2):
            g, n_at, fast = spy.run(lambda: _backward(op, x, y))
            assert n_at == 0 and fast == [('_fastc_A', True)]
            assert tr.equal(g, g0)
        t, n_at, fast = spy.run(lambda: op.T(y, time_slices=True))
        assert n_at == 0 and fast == [('_fastc_A', True)] and tr.equal(t, g0)
        op.adjoint_mode = 'atomic'
        for fn in (lambda: _backward(op, x, y), lambda: op.T(y, time_slices=True)):
            b, n_at, fast = spy.run(fn)
            assert n_at == 1 and not any(s for _, s in fast)
            assert b.shape == DGRID and b.dtype == dt
            _assert_close(b, want, TOL[dt])
            _assert_modes_agree(b, g0, dt)
        assert op._fastc_A is not None
        op.adjoint_mode = 'transpose'
        for fn in (lambda: _backward(op, x, y), lambda: op.T(y, time_slices=True)):
            c1, n_at1, _ = spy.run(fn)
            c2, n_at2, fast = spy.run(fn)
            assert n_at1 == 0 and n_at2 == 0 and fast == [('_fastc_A', True)]
            assert tr.equal(c1, g0) and tr.equal(c2, g0)
    finally:
        op.adjoint_mode = 'transpose'


@pytest.mark.parametrize('device', ['cuda', tr.device('cuda', 0)], ids=['cuda', 'cuda:0'])
def test_time_slices_takes_the_binding(dyn, device, gpu, monkeypatch):
    """T(time_slices=True) on an Operator whose device names the GPU with or without an index:
    the first call binds, every later one is served by _fastc_A; bitwise the backward's
    gradient."""
    grid, geom, _, ref, _ = dyn
    op, div = _dyn_op(dyn, device)
    spy = _Spy(monkeypatch, op)
    for dt in (F64, F32):
        x, y = _rand(DGRID, dt, 9, gpu), _rand(geom.shape, dt, 10, gpu)
        t0, n_at, fast = spy.run(lambda: op.T(y, time_slices=True))
        assert n_at == 0 and not any(s for _, s in fast)
        assert t0.device == gpu and t0.shape == DGRID and t0.dtype == dt
        _assert_close(t0, ref.adjoint(y, div=div, n_t=T_DYN), TOL[dt])
        for _ in range(2):
            t, n_at, fast = spy.run(lambda: op.T(y, time_slices=True))
            assert n_at == 0 and fast == [('_fastc_A', True)] and tr.equal(t, t0)
        # (the first forward of a dtype binds _fastc, which sets op._fastfn anew: the spy sees
        # the backward of the second one)
        g, n_at, _ = spy.run(lambda: _backward(op, x, y))
        assert n_at == 0 and tr.equal(g, t0)
        g, n_at, fast = spy.run(lambda: _backward(op, x, y))
        assert n_at == 0 and fast == [('_fastc_A', True)] and tr.equal(g, t0)


@pytest.mark.parametrize('mode', ['transpose', 'atomic'])
def test_paired_binding_serves_its_density_shape_only(dyn, mode, gpu, monkeypatch):
    """With the (5, ...) gradient bound for y's shape, the adjoint of a (1, nr, ne, na) density
    (every view into the one slice: the same y) is not served by that binding: shape
    (1, nr, ne, na), the reference's sum over all views."""
    grid, geom, _, ref, _ = dyn
    op, div = _dyn_op(dyn, 'cuda')
    spy = _Spy(monkeypatch, op)
    one = (1,) + DGRID[1:]
    try:
        for dt in (F64, F32):
            x, y = _rand(DGRID, dt, 11, gpu), _rand(geom.shape, dt, 12, gpu)
            g0 = _backward(op, x, y)
            g, _, fast = spy.run(lambda: _backward(op, x, y))
            assert fast == [('_fastc_A', True)] and tr.equal(g, g0)    # the (5, ...) binding
            want = ref.adjoint(y)                                         # every ray, one slice
            assert np.allclose(want, ref.adjoint(y, div=div, n_t=T_DYN).sum(0)[None],
                               rtol=1e-12, atol=0)
            op.adjoint_mode = mode
            n_want = 1 if mode == 'atomic' else 0
            got, n_at, fast = spy.run(lambda: op._apply_adjoint(y, one, dt, gpu))
            assert n_at == n_want and not any(s for _, s in fast)
            assert got.shape == one and got.dtype == dt
            _assert_close(got, want, TOL[dt])
            x1 = _rand(one, dt, 13, gpu)
            got, n_at, fast = spy.run(lambda: _backward(op, x1, y))
            assert n_at == n_want and not any(s for _, s in fast)
            assert got.shape == one and got.dtype == dt
            _assert_close(got, want, TOL[dt])
            op.adjoint_mode = 'transpose'
            g, _, fast = spy.run(lambda: _backward(op, x, y))           # still bound, same bits
            assert fast == [('_fastc_A', True)] and tr.equal(g, g0)
    finally:
        op.adjoint_mode = 'transpose'


def test_pairing_without_a_paired_csr(dyn, gpu, monkeypatch):
    """The fallback when the time-paired CSR cannot be built (_paired -> None, as for T * vol
    beyond 32-bit columns): the forward gathers time slices on the trace's CSR (kFwdDynamic), the
    backward runs the atomic kernel although the mode says 'transpose', nothing is bound."""
    grid, geom, _, ref, _ = dyn
    op, div = _dyn_op(dyn, gpu)
    op._csr[('paired', T_DYN, div)] = None
    spy = _Spy(monkeypatch, op)
    assert op.adjoint_mode == 'transpose'
    for dt in (F64, F32):
        x, y = _rand(DGRID, dt, 14, gpu), _rand(geom.shape, dt, 15, gpu)
        t = 'float, float' if dt == F32 else 'double, double'
        assert op._forward_kernel_name(x).startswith(f'forward_kernel<{t}, 2,')
        fx = op(x)
        assert fx.shape == tuple(geom.shape) and fx.dtype == dt
        _assert_close(fx, ref.forward(x, div=div), TOL[dt])
        want = ref.adjoint(y, div=div, n_t=T_DYN)
        for _ in range(2):
            g, n_at, fast = spy.run(lambda: _backward(op, x, y))
            assert n_at == 1 and fast == []
            assert g.shape == DGRID and g.dtype == dt
            _assert_close(g, want, TOL[dt])
        t1, n_at, fast = spy.run(lambda: op.T(y, time_slices=True))
        assert n_at == 1 and fast == []
        _assert_close(t1, want, TOL[dt])
    assert op._fastc_A is None and op._paired(T_DYN, div) is None


@pytest.mark.parametrize('dt', [F64, F32])
def test_single_view_every_time_step(dyn, dt, gpu, monkeypatch):
    """D1: one geometry seen at every time step (n_chan = T, div = 0): the gradient of a
    (5, ...) density in 'transpose' and in 'atomic' (the atomic kernel over T channels)."""
    from sph_raytracer_amd import Operator
    grid, _, single, _, ref1 = dyn
    op = Operator(grid, single, device=gpu)
    assert op._layout(DGRID) == (T_DYN, 0, (T_DYN,) + tuple(single.shape))
    assert op._csr['ray_id'] is not None and op._csr['n'] == ref1.n
    spy = _Spy(monkeypatch, op)
    x = _rand(DGRID, dt, 16, gpu)
    y = _rand((T_DYN,) + tuple(single.shape), dt, 17, gpu)
    want = ref1.adjoint(y, n_chan=T_DYN)
    try:
        g0, n_at, fast = spy.run(lambda: _backward(op, x, y))
        assert n_at == 0 and not any(s for _, s in fast)
        _assert_close(g0, want, TOL[dt])
        g1, n_at, _ = spy.run(lambda: _backward(op, x, y))
        assert n_at == 0 and tr.equal(g1, g0)
        t0, n_at, _ = spy.run(lambda: op.T(y, time_slices=True))
        assert n_at == 0 and tr.equal(t0, g0)
        op.adjoint_mode = 'atomic'
        for fn in (lambda: _backward(op, x, y), lambda: op.T(y, time_slices=True)):
            b, n_at, fast = spy.run(fn)
            assert n_at == 1 and not any(s for _, s in fast)
            assert b.shape == DGRID and b.dtype == dt
            _assert_close(b, want, TOL[dt])
            _assert_modes_agree(b, g0, dt)
        op.adjoint_mode = 'transpose'
        g2, n_at, _ = spy.run(lambda: _backward(op, x, y))
        assert n_at == 0 and tr.equal(g2, g0)
    finally:
        op.adjoint_mode = 'transpose'


def test_dense_ranges_refuse_a_misaligned_output(dyn, gpu):
    """The time-paired transposed CSR zeroes its output ranges with 16-byte stores placed by
    element index: sphrt_forward_* refuses an output that is not 16-byte aligned on the host,
    before any launch; with an aligned one it gives the gradient."""
    from sph_raytracer_amd import _lib
    grid, geom, _, ref, _ = dyn
    op, div = _dyn_op(dyn, gpu)
    y = _rand(geom.shape, F64, 18, gpu)
    g = op._apply_adjoint(y, DGRID, F64, gpu)
    _assert_close(g, ref.adjoint(y, div=div, n_t=T_DYN), TOL[F64])
    pt = _paired_transpose(op, div)
    lib = _lib.load()
    assert pt.n_rays == math.prod(DGRID) and pt.n_blocks == lib.sphrt_csr_blocks_dense(pt.n_segments)
    yt = y.reshape(-1).contiguous()
    buf = tr.zeros(pt.n_rays + 4, dtype=F64, device=gpu)
    off = buf[1:1 + pt.n_rays]
    assert buf.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 8
    rc = lib.sphrt_forward_f64(pt, _lib.ptr(yt), 1, yt.numel(), 0, _lib.ptr(off), pt.n_rays,
                               _lib.stream_of(gpu))
    assert rc != 0
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        _lib.check(rc, 'forward')
    y32 = yt.float()
    buf32 = tr.zeros(pt.n_rays + 4, dtype=F32, device=gpu)
    for k in (1, 2, 3):
        off32 = buf32[k:k + pt.n_rays]
        assert off32.data_ptr() % 16 == 4 * k
        rc = lib.sphrt_forward_f32(pt, _lib.ptr(y32), 1, y32.numel(), 0, _lib.ptr(off32),
                                   pt.n_rays, _lib.stream_of(gpu))
        with pytest.raises(RuntimeError, match='16-byte aligned'):
            _lib.check(rc, 'forward')
    tr.cuda.synchronize(gpu)
    assert not buf.any() and not buf32.any()                      # nothing was written
    out = buf[2:2 + pt.n_rays]
    assert out.data_ptr() % 16 == 0
    rc = lib.sphrt_forward_f64(pt, _lib.ptr(yt), 1, yt.numel(), 0, _lib.ptr(out), pt.n_rays,
                               _lib.stream_of(gpu))
    _lib.check(rc, 'forward')
    assert tr.equal(out.reshape(g.shape), g)
