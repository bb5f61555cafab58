"""Weighted least squares on the GPU: MatrixFreeOperator.residual_gradient(weights=...) (the
trace's weighted normal modes, sphrt_trace_normal_weighted_f64 / _fixed_f64), the weighted loss
tail sphrt_wsq_residual_f64, and gd()'s direct loops with a SquareLoss(projection_mask=tensor)
over a stored Operator and over a MatrixFreeOperator.

References: the C oracle's own trace (test_gpu_adjoint_paths._Ref: forward, and adjoint of the
residual s_i * (fwd_i - m_i) formed in numpy); for the loops, this project's autograd loop of
the same masked problem; for the loss tail, torch's elementwise ops.  Never the new entries.

Tolerances (the project's own): float64 within 1e-10 x max|reference|, float32 within 1e-5 x;
against the two separate calls op.T(s * (op(x) - m)) rtol 1e-12 and atol 1e-12 x max; yhat
bitwise the float64 forward; the stored loop's iterates bitwise the autograd loop's and its
losses within 1e-13 relative; the fused loop within 1e-9 of the autograd loop (the gd_circ16
pins' bounds)."""
import numpy as np
import pytest
import torch as tr

import golden_cases as gc
from gpu_helpers import exact_stats
from test_gpu_adjoint_paths import (DGRID, F32, F64, SGRID, T_DYN, TOL, _assert_close,
                                    _check_coverage, _orbit, _rand, _Ref, _static_geom)
from test_gpu_matrix_free_deterministic import _bits, _flat_geom, _lattice_subset
from test_gpu_matrix_free_gradient import (SCALE, _assert_separate_agree, _exact_waves,
                                           _gd_circ16, _ref_forward)

pytestmark = pytest.mark.gpu


def _weights(shape, seed, gpu, dt=F64):
    """Random weights in (-0.6, 1.4) with about a fifth exact zeros."""
    w = _rand(shape, F64, seed, 'cpu') * 2 - 0.6
    w[_rand(shape, F64, seed + 1000, 'cpu') < 0.2] = 0
    assert bool((w == 0).any()) and bool((w < 0).any()) and bool((w > 0).any())
    return w.to(dt).to(gpu)


def _factors(w, scale, shape):
    """ray_scale as the issue defines it: weights.to(float64) * scale, one rounding -> numpy."""
    s = w.detach().cpu().to(F64).numpy() * np.float64(scale)
    return np.broadcast_to(s, tuple(shape)).reshape(-1)


def _ref_weighted(ref, fwd, m, s, **kw):
    """The oracle's A^T(s * (fwd - m)) from its own forward `fwd` (numpy)."""
    r = s * (fwd.reshape(-1) - m.detach().cpu().double().numpy().reshape(-1))
    return ref.adjoint(tr.from_numpy(r), **kw)


def _op(grid, geom, gpu, **kw):
    from sph_raytracer_amd import MatrixFreeOperator
    return MatrixFreeOperator(grid, geom, device=gpu, **kw)


# ---- 1. static grids -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def static_cases():
    """name -> (grid, geom, reference, MatrixFreeOperator): built once per geometry, read-only."""
    cache = {}

    def get(name, gpu):
        if name not in cache:
            from sph_raytracer_amd import SphericalGrid
            grid, geom = SphericalGrid(shape=SGRID), _static_geom(name)
            ref = _Ref(grid, geom)
            _check_coverage(ref)
            cache[name] = (grid, geom, ref, _op(grid, geom, gpu))
        return cache[name]

    return get


@pytest.mark.parametrize('lead', [(), (3,)], ids=['1ch', '3ch'])
@pytest.mark.parametrize('name', ['S1', 'S3'])
def test_static_weighted_gradient(name, lead, gpu, static_cases):
    grid, geom, ref, op = static_cases(name, gpu)
    n_chan = 3 if lead else 1
    x = _rand(lead + SGRID, F64, 141, gpu)
    m = _rand(lead + tuple(geom.shape), F64, 142, gpu)
    w = _weights(m.shape, 143, gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=w)
    assert yhat.shape == m.shape and yhat.dtype == F64 and yhat.device == gpu
    assert grad.shape == x.shape and grad.dtype == F64 and grad.device == gpu
    ax = op(x)
    assert tr.equal(yhat, ax)
    fwd = _ref_forward(ref, x, n_chan)
    _assert_close(grad, _ref_weighted(ref, fwd, m, _factors(w, SCALE, m.shape), n_chan=n_chan),
                  TOL[F64])
    _assert_separate_agree(grad, op.T((w * SCALE) * (ax - m)))
    # float32 in, float32 out (float32 weights too)
    x32, m32, w32 = x.float(), m.float(), w.float()
    y32, g32 = op.residual_gradient(x32, m32, SCALE, weights=w32)
    assert y32.dtype == F32 and g32.dtype == F32 and y32.shape == m.shape and g32.shape == x.shape
    fwd32 = _ref_forward(ref, x32, n_chan)
    _assert_close(y32, fwd32, TOL[F32])
    _assert_close(g32, _ref_weighted(ref, fwd32, m32, _factors(w32, SCALE, m.shape),
                                     n_chan=n_chan), TOL[F32])


@pytest.mark.parametrize('lead', [(), (3,)], ids=['1ch', '3ch'])
def test_broadcast_bool_and_host_weights(lead, gpu, static_cases):
    """Weights of shape geom.shape[1:] broadcast over the views (and channels); a bool mask;
    CPU inputs give CPU results."""
    grid, geom, ref, op = static_cases('S3', gpu)
    n_chan = 3 if lead else 1
    x = _rand(lead + SGRID, F64, 144, gpu)
    m = _rand(lead + tuple(geom.shape), F64, 145, gpu)
    fwd = _ref_forward(ref, x, n_chan)
    wb = _weights(tuple(geom.shape)[1:], 146, gpu)
    assert wb.dim() < m.dim()
    _, grad = op.residual_gradient(x, m, SCALE, weights=wb)
    _assert_close(grad, _ref_weighted(ref, fwd, m, _factors(wb, SCALE, m.shape), n_chan=n_chan),
                  TOL[F64])
    mask = _rand(m.shape, F64, 147, gpu) < 0.6
    assert mask.dtype == tr.bool and bool(mask.any()) and not bool(mask.all())
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=mask)
    assert tr.equal(yhat, op(x))
    _assert_close(grad, _ref_weighted(ref, fwd, m, _factors(mask, SCALE, m.shape),
                                      n_chan=n_chan), TOL[F64])
    # host tensors in (the weights too), host tensors out; the default scale is 1
    wc = _weights(m.shape, 148, 'cpu', F32)
    yc, gc_ = op.residual_gradient(x.cpu(), m.cpu(), weights=wc)
    assert yc.device.type == 'cpu' and gc_.device.type == 'cpu' and gc_.dtype == F64
    _assert_close(gc_, _ref_weighted(ref, fwd, m, _factors(wc, 1.0, m.shape), n_chan=n_chan),
                  TOL[F64])
    # GPU data with host weights
    _, gh = op.residual_gradient(x, m, weights=wc)
    assert gh.device == gpu
    _assert_separate_agree(gh, gc_.to(gpu))


# ---- 2. both code sites --------------------------------------------------------------------------
@pytest.mark.parametrize('deterministic', [False, True], ids=['atomic', 'fixed'])
def test_wave_path_on_lattice_ties(deterministic, gpu):
    """consume_list behind every wave-level path: a tie lattice, whose deferred rays go through
    exact_walk_wave (4 waves per ray at this K) and the rest through the trace kernel."""
    from sph_raytracer_amd.raytracer import _Plan
    name = gc.LATTICE_CASES[0]
    case = gc.load(name)
    grid = gc.make_grid(case)
    geom = gc.FixtureGeom(dict(case, xs=case['xs'].copy(), rays=case['rays'].copy()))
    assert _exact_waves(int(_Plan(grid, gpu).K)) == 4
    deferred = exact_stats(grid, geom, gpu)[0]
    ref = _Ref(grid, geom)
    hit = int((np.diff(ref.ptr) > 0).sum())
    assert 0 < deferred < hit, (deferred, hit)
    op = _op(grid, geom, gpu, deterministic=deterministic)
    x, m = _rand(grid.shape, F64, 149, gpu), _rand(geom.shape, F64, 150, gpu)
    w = _weights(m.shape, 151, gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=w)
    assert tr.equal(yhat, op(x))
    fwd = _ref_forward(ref, x, 1)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_weighted(ref, fwd, m, _factors(w, SCALE, m.shape)), TOL[F64])


@pytest.mark.parametrize('deterministic', [False, True], ids=['atomic', 'fixed'])
def test_serial_exact_walk_with_channels(deterministic, gpu):
    """The serial exact_walk (K = 2013 > 1815: no wave's LDS holds the list) with three channels:
    the scattering walk forms every channel's residual with that channel's own factor."""
    from sph_raytracer_amd.raytracer import _Plan
    grid, geom = _lattice_subset(1000, gpu)
    K = int(_Plan(grid, gpu).K)
    assert K == 2 * (1000 + 1) + 2 * 5 + 5 + 1 and K > 1815 and _exact_waves(K) == 0
    ref = _Ref(grid, geom)
    deferred = exact_stats(grid, geom, gpu)[0]
    assert 0 < deferred <= int((np.diff(ref.ptr) > 0).sum())
    op = _op(grid, geom, gpu, deterministic=deterministic)
    x = _rand((3,) + tuple(grid.shape), F64, 152, gpu)
    m = _rand((3,) + tuple(geom.shape), F64, 153, gpu)
    w = _weights(m.shape, 154, gpu)
    assert not tr.equal(w[0], w[1])                    # (a factor per channel, not per ray)
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=w)
    assert tr.equal(yhat, op(x))
    fwd = _ref_forward(ref, x, 3)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_weighted(ref, fwd, m, _factors(w, SCALE, m.shape), n_chan=3),
                  TOL[F64])


# ---- 3. time-paired dynamic grid -----------------------------------------------------------------
@pytest.mark.parametrize('deterministic', [False, True], ids=['atomic', 'fixed'])
def test_dynamic_view_time_pairing(deterministic, gpu):
    """5 views <-> 5 time slices (ray_chan_div > 0): ray i's factor is ray_scale[i]."""
    from sph_raytracer_amd import ConeCircGeom, SphericalGrid
    grid = SphericalGrid(shape=DGRID)
    geom = sum(ConeCircGeom((24, 16), pos=p, fov=(0, 12)) for p in _orbit(T_DYN))
    ref = _Ref(grid, geom)
    div = ref.n // T_DYN
    _check_coverage(ref, div=div, n_t=T_DYN)
    op = _op(grid, geom, gpu, dynamic=True, deterministic=deterministic)
    assert op._layout(DGRID) == (1, div, tuple(geom.shape))
    x, m = _rand(DGRID, F64, 155, gpu), _rand(geom.shape, F64, 156, gpu)
    w = _weights(m.shape, 157, gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=w)
    assert yhat.shape == tuple(geom.shape) and grad.shape == DGRID
    assert tr.equal(yhat, op(x))
    fwd = ref.forward(x, div=div)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_weighted(ref, fwd, m, _factors(w, SCALE, m.shape), div=div,
                                      n_t=T_DYN), TOL[F64])


# ---- 4. exact properties -------------------------------------------------------------------------
def test_unit_weights_are_the_unweighted_call_bitwise(gpu, static_cases):
    """Weights of all ones with scale 0.37, deterministic: the same record (S = 0.37) and the
    same terms as residual_gradient(x, m, 0.37), so the same bits."""
    grid, geom, ref, _ = static_cases('S3', gpu)
    op = _op(grid, geom, gpu, deterministic=True)
    x = _rand((3,) + SGRID, F64, 158, gpu)
    m = _rand((3,) + tuple(geom.shape), F64, 159, gpu)
    y0, g0 = op.residual_gradient(x, m, 0.37)
    assert bool(g0.any())
    for ones in (tr.ones(m.shape, dtype=F64, device=gpu), tr.ones(geom.shape, dtype=F32),
                 tr.ones(1, dtype=tr.bool, device=gpu)):
        y1, g1 = op.residual_gradient(x, m, 0.37, weights=ones)
        assert tr.equal(y1, y0) and tr.equal(g1, g0)


@pytest.mark.parametrize('deterministic', [False, True], ids=['atomic', 'fixed'])
def test_zero_weights_and_zero_residual(deterministic, gpu, static_cases):
    """All-zero weights: no non-zero element in grad.  m = op(x): grad exactly zero whatever the
    finite weights (the scatter uses the sum the same kernel integrated)."""
    grid, geom, ref, _ = static_cases('S3', gpu)
    op = _op(grid, geom, gpu, deterministic=deterministic)
    x = _rand((3,) + SGRID, F64, 160, gpu)
    m = _rand((3,) + tuple(geom.shape), F64, 161, gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=tr.zeros_like(m))
    assert tr.equal(yhat, op(x)) and grad.shape == x.shape and not grad.any()
    assert not grad.isnan().any()
    w = _weights(m.shape, 162, gpu) * 1e3
    y0, g0 = op.residual_gradient(x, yhat, SCALE, weights=w)
    assert tr.equal(y0, yhat) and g0.shape == x.shape and not g0.any() and not g0.isnan().any()


def test_nan_under_a_zero_weight_stays_nan(gpu, static_cases):
    """Rays of weight zero are not skipped: NaN * 0 is NaN, as in torch's op.T(w * (op(x) - m))
    (atomic mode: the voxels that ray reaches, and only those)."""
    grid, geom, ref, op = static_cases('S1', gpu)
    x, m = _rand(SGRID, F64, 163, gpu), _rand(geom.shape, F64, 164, gpu)
    w = tr.ones_like(m)
    ray = int(np.argmax(np.diff(ref.ptr)))                 # a ray that crosses the grid
    m.view(-1)[ray], w.view(-1)[ray] = float('nan'), 0.0
    _, grad = op.residual_gradient(x, m, SCALE, weights=w)
    want = np.zeros(ref.vol, dtype=bool)
    want[ref.vox[ref.ptr[ray]:ref.ptr[ray + 1]]] = True
    assert want.any() and not want.all()
    assert np.array_equal(grad.isnan().cpu().numpy().reshape(-1), want)


# ---- 5. deterministic mode -----------------------------------------------------------------------
def test_deterministic_bits(gpu, static_cases):
    """Two calls give equal bits; so does the same ray set in another order (the method of
    test_two_calls_and_a_permutation_are_equal); the result is within tolerance of the oracle;
    a weight that is not finite raises ValueError."""
    grid, geom, ref, _ = static_cases('S3', gpu)
    op = _op(grid, geom, gpu, deterministic=True)
    x, m = _rand(SGRID, F64, 165, gpu), _rand(geom.shape, F64, 166, gpu)
    w = _weights(m.shape, 167, gpu)
    yh, g = op.residual_gradient(x, m, SCALE, weights=w)
    yh2, g2 = op.residual_gradient(x, m, SCALE, weights=w)
    assert tr.equal(yh, yh2) and tr.equal(g, g2)
    fwd = _ref_forward(ref, x, 1)
    _assert_close(g, _ref_weighted(ref, fwd, m, _factors(w, SCALE, m.shape)), TOL[F64])
    perm = np.random.default_rng(168).permutation(ref.n)
    pop = _op(grid, _flat_geom(geom, perm), gpu, deterministic=True)
    pt = tr.from_numpy(perm).to(gpu)
    yhp, gp = pop.residual_gradient(x, m.reshape(-1)[pt], SCALE, weights=w.reshape(-1)[pt])
    assert tr.equal(yhp, yh.reshape(-1)[pt]) and tr.equal(gp, g)
    for bad in (float('inf'), -float('inf'), float('nan')):
        wb = w.clone()
        wb.view(-1)[7] = bad
        with pytest.raises(ValueError, match='finite'):
            op.residual_gradient(x, m, SCALE, weights=wb)
    with pytest.raises(ValueError, match='finite'):
        op.residual_gradient(x, m, float('inf'), weights=w)


# ---- 6. the weighted loss tail alone -------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 7, 100001, 700000])
@pytest.mark.parametrize('ydt', [F64, F32], ids=['y64', 'y32'])
@pytest.mark.parametrize('mode', ['in_order', 'order', 'unaligned'])
def test_wsq_residual_kernel(n, ydt, mode, gpu):
    """sphrt_wsq_residual_f64: r_scaled = (yhat - y) * s elementwise as torch computes it
    (bitwise), in order, through a ray map and from pointers offset by one element; the partial
    sums of w * (r * r), w >= 0, within 1e-13 relative of torch's sum."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    g = tr.Generator(device='cpu').manual_seed(n)
    yhat = tr.randn(n + 1, generator=g, dtype=F64).to(gpu)
    y = tr.randn(n + 1, generator=g, dtype=F64).to(ydt).to(gpu)
    s = tr.randn(n + 1, generator=g, dtype=F64).to(gpu)
    w = tr.rand(n + 1, generator=g, dtype=F64).to(gpu)
    s[::5], w[::3] = 0, 0
    order = None
    if mode == 'unaligned':
        yhat, y, s, w = yhat[1:], y[1:], s[1:], w[1:]
    else:
        yhat, y, s, w = yhat[:n], y[:n], s[:n], w[:n]
    if mode == 'order':
        order = tr.randperm(n, generator=g).to(tr.int32).to(gpu)
    out = tr.empty(n, dtype=F64, device=gpu)
    part = tr.full((lib.sphrt_loss_partials(n),), float('nan'), dtype=F64, device=gpu)
    _lib.check(lib.sphrt_wsq_residual_f64(_lib.ptr(yhat), _lib.ptr(y), int(ydt == F64), n,
                                          _lib.ptr(s), _lib.ptr(w), _lib.ptr(order),
                                          _lib.ptr(out), _lib.ptr(part), _lib.stream_of(gpu)),
               'wsq_residual')
    r = yhat - y.to(F64)
    if order is not None:
        r, s, w = r[order.long()], s[order.long()], w[order.long()]
    assert tr.equal(out, r * s)
    assert not tr.isnan(part).any()
    ref = float((w * (r * r)).sum())
    assert abs(float(part.sum()) - ref) <= 1e-13 * abs(ref)


# ---- 7. gd on a stored Operator ------------------------------------------------------------------
@pytest.fixture(scope='module')
def circ16(gpu):
    """The 16^3 grid and 12 ConeCirc views of (20, 16) of test_gd_direct_matches_autograd, its
    stored Operator and float64 measurements of the same phantom."""
    from sph_raytracer_amd import ConeCircGeom, Operator, SphericalGrid
    grid = SphericalGrid(shape=(16, 16, 16))
    geom = sum(ConeCircGeom(shape=(20, 16), pos=(5 * tr.cos(th), 5 * tr.sin(th), 1),
                            fov=(0, 45)) for th in tr.linspace(0, 2 * tr.pi, 12))
    x = tr.zeros(grid.shape, dtype=F64, device=gpu)
    x[:, 8:, :8] = 1
    x[:, :8, 8:] = 1
    op = Operator(grid, geom, device=gpu)
    return grid, geom, op, op(x)


def _mask(kind, shape, gpu):
    if kind == 'zero_one':
        m = (_rand(shape, F64, 170, gpu) > 1 / 3).to(F64)
        assert 0.2 < float((m == 0).double().mean()) < 0.45
    elif kind == 'float32':
        m = _rand(shape, F32, 171, gpu) * 2
    elif kind == 'bool':
        m = _rand(shape, F64, 172, gpu) > 0.4
    else:
        m = _rand(tuple(shape)[1:], F64, 173, gpu) * 1.5        # (20, 16), over the views
        assert m.dim() == len(shape) - 1
    return m


def _run_gd(op, meas, grid, mask, lams, **kw):
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    fns = [lams[0] * SquareLoss(projection_mask=mask)] + \
        ([lams[1] * NegRegularizer()] if lams[1] else [])
    c, yh, hist = retrieval.gd(op, meas.clone(), FullyDenseModel(grid), lr=1e-1,
                               num_iterations=25, loss_fns=fns, progress_bar=False, **kw)
    return c.detach().clone(), yh.detach().clone(), [list(v) for v in hist.values()]


@pytest.mark.parametrize('lams, meas_dtype', [((1, 1), F64), ((0.5, 2), F64), ((0.5, None), F32),
                                              ((1, 1), F32)])
@pytest.mark.parametrize('kind', ['zero_one', 'float32', 'bool', 'broadcast'])
def test_gd_direct_with_mask_matches_autograd(kind, lams, meas_dtype, gpu, monkeypatch, circ16):
    """gd() with SquareLoss(projection_mask=mask) + NegRegularizer over a stored Operator takes
    `_gd_direct` and gives the autograd loop's coefficients and reconstruction bitwise, its loss
    histories within 1e-13 relative — with the measurements permuted into trace order
    (`_trace_position_rows`) and, with that declined, through the kernel's `order` argument."""
    from sph_raytracer_amd import Operator, retrieval
    grid, geom, op, meas64 = circ16
    meas = meas64.to(meas_dtype)
    mask = _mask(kind, meas.shape, gpu)
    calls, rows = [], []
    direct, orig_rows = retrieval._gd_direct, Operator._trace_position_rows

    def spy(*a, **k):
        calls.append(1)
        return direct(*a, **k)

    monkeypatch.setattr(retrieval, '_gd_direct', spy)
    monkeypatch.setattr(Operator, '_trace_position_rows',
                        lambda self, sd: rows.append(orig_rows(self, sd)) or rows[-1])
    ca, ya, ha = _run_gd(op, meas, grid, mask, lams)
    assert len(calls) == 1
    assert len(rows) == 1 and rows[0] is not None       # (y, w and s permuted into trace order)
    with monkeypatch.context() as mp:
        mp.setattr(retrieval, '_direct_plan', lambda *a: None)
        cb, yb, hb = _run_gd(op, meas, grid, mask, lams)
    assert len(calls) == 1
    assert len(ha) == len(hb) == (2 if lams[1] else 1) and len(ha[0]) == 25
    assert ha[0][-1] < ha[0][0]
    for la, lb in zip(ha, hb):
        assert np.allclose(la, lb, rtol=1e-13, atol=0), (la, lb)
    assert tr.equal(ca, cb) and tr.equal(ya, yb)
    # the kernel's `order` branch: the trace-position forward declined
    assert op._adjoint_trace_order() is not None
    monkeypatch.setattr(Operator, '_trace_position_rows', lambda self, sd: None)
    cc, yc, hc = _run_gd(op, meas, grid, mask, lams)
    assert len(calls) == 2
    for lc, lb in zip(hc, hb):
        assert np.allclose(lc, lb, rtol=1e-13, atol=0), (lc, lb)
    assert tr.equal(cc, cb) and tr.equal(yc, yb)


def test_direct_plan_mask_conditions(gpu, circ16):
    """A projection_mask the direct loop takes: a constant tensor on y's device, bool, float32 or
    float64, broadcastable to y.  Anything else, a volume_mask and a NegRegularizer's masks keep
    declining; the plan stays the tuple (sq, neg)."""
    from sph_raytracer_amd import MatrixFreeOperator, retrieval
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom, op, meas = circ16
    model = FullyDenseModel(grid)
    c = tr.ones(grid.shape, dtype=F64, device=gpu)
    mfo = MatrixFreeOperator(grid, geom, device=gpu)
    good = _mask('zero_one', meas.shape, gpu)

    def plans(fns):
        return (retrieval._direct_plan(op, meas, model, c, fns, [c]),
                retrieval._fused_plan(mfo, meas, model, c, fns, [c]))

    for mask in (good, good.float(), good.bool(), good[0], good[0, :, :1], good[:1]):
        sq, neg = SquareLoss(projection_mask=mask), NegRegularizer()
        assert plans([sq, neg]) == ((sq, neg), (sq, neg))
        assert plans([sq]) == ((sq, None), (sq, None))
    declined = [
        SquareLoss(projection_mask=good.clone().requires_grad_()),
        SquareLoss(projection_mask=good.cpu()),
        SquareLoss(projection_mask=good.to(tr.int32)),
        SquareLoss(projection_mask=good.half()),
        SquareLoss(projection_mask=good[:, :-1]),
        SquareLoss(projection_mask=good[None]),
        SquareLoss(projection_mask=2),
        SquareLoss(volume_mask=tr.ones(grid.shape, dtype=F64, device=gpu)),
        SquareLoss(projection_mask=good, volume_mask=tr.ones(grid.shape, dtype=F64, device=gpu)),
    ]
    for sq in declined:
        assert plans([sq]) == (None, None)
    for neg in (NegRegularizer(projection_mask=good),
                NegRegularizer(volume_mask=tr.ones(grid.shape, dtype=F64, device=gpu))):
        assert plans([SquareLoss(), neg]) == (None, None)


# ---- 8. masked measurements do not matter --------------------------------------------------------
def test_masked_measurements_do_not_matter(gpu, circ16):
    """With a 0/1 mask, other finite values of y where the mask is 0 leave the coefficients, the
    reconstruction and both loss histories unchanged (stored Operator: a deterministic adjoint)."""
    grid, geom, op, meas = circ16
    mask = _mask('zero_one', meas.shape, gpu)
    other = tr.where(mask == 0, (_rand(meas.shape, F64, 174, gpu) - 0.5) * 1e3, meas)
    assert not tr.equal(other, meas) and tr.equal(other * mask, meas * mask)
    ca, ya, ha = _run_gd(op, meas, grid, mask, (0.5, 2))
    cb, yb, hb = _run_gd(op, other, grid, mask, (0.5, 2))
    assert tr.equal(ca, cb) and tr.equal(ya, yb)
    assert ha == hb and len(ha[0]) == 25


# ---- 9. gd on a MatrixFreeOperator ---------------------------------------------------------------
def _gd_masked_mfo(op, meas, model, mask, n_it):
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    sq, neg = SquareLoss(projection_mask=mask), NegRegularizer()
    coeffs, y_res, losses = retrieval.gd(op, meas.clone(), model, lr=0.1, num_iterations=n_it,
                                         loss_fns=[sq, neg], progress_bar=False)
    return coeffs.detach().clone(), y_res.detach().clone(), list(losses[sq]), list(losses[neg])


@pytest.mark.parametrize('kind', ['zero_one', 'float32'])
def test_gd_with_mask_takes_the_fused_loop(kind, gpu, monkeypatch):
    """gd() over a MatrixFreeOperator with a projection_mask: _fused_plan accepts; one
    _normal_into per iteration, one forward after the loop, no adjoint; with deterministic=True
    two runs give equal bits; against the autograd loop of the same masked problem the bounds of
    the gd_circ16 pins (coefficients and reconstruction 1e-9, loss 1e-9 relative, regulariser
    1e-12)."""
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    case, op, meas, model, _, _ = _gd_circ16(gpu)
    n_it = int(case['iterations'])
    mask = _mask(kind, meas.shape, gpu)
    c0 = tr.ones(model.coeffs_shape, dtype=F64, device=gpu)
    sq, neg = SquareLoss(projection_mask=mask), NegRegularizer()
    assert retrieval._direct_plan(op, meas, model, c0, [sq, neg], [c0]) is None
    assert retrieval._fused_plan(op, meas, model, c0, [sq, neg], [c0]) == (sq, neg)
    calls = {'forward': [], 'adjoint': 0, 'normal': 0, 'weighted': 0}
    fwd, adj, normal = op._apply_forward, op._apply_adjoint, op._normal_into

    def forward(density):
        calls['forward'].append(fwd(density))
        return calls['forward'][-1]

    def adjoint(*a, **k):
        calls['adjoint'] += 1
        return adj(*a, **k)

    def normal_into(*a, **k):
        calls['normal'] += 1
        calls['weighted'] += k.get('weighted') is not None
        return normal(*a, **k)

    monkeypatch.setattr(op, '_apply_forward', forward)
    monkeypatch.setattr(op, '_apply_adjoint', adjoint)
    monkeypatch.setattr(op, '_normal_into', normal_into)
    fused = _gd_masked_mfo(op, meas, model, mask, n_it)
    assert len(calls['forward']) == 1 and calls['adjoint'] == 0
    assert calls['normal'] == calls['weighted'] == n_it
    assert tr.equal(fused[1], calls['forward'][0].detach())
    op.deterministic = True
    det = [_gd_masked_mfo(op, meas, model, mask, n_it) for _ in range(2)]
    op.deterministic = False
    assert calls['normal'] == calls['weighted'] == 3 * n_it and calls['adjoint'] == 0
    assert tr.equal(det[0][0], det[1][0]) and tr.equal(det[0][1], det[1][1])
    assert _bits(det[0][2]) == _bits(det[1][2]) and _bits(det[0][3]) == _bits(det[1][3])
    # the autograd loop of the same masked problem
    monkeypatch.setattr(retrieval, '_fused_plan', lambda *a, **k: None)
    auto = _gd_masked_mfo(op, meas, model, mask, n_it)
    assert calls['normal'] == 3 * n_it and calls['adjoint'] == n_it
    assert len(auto[2]) == n_it and auto[2][-1] < auto[2][0]
    for what, got in (('fused', fused), ('deterministic', det[0])):
        l_sq, l_neg, a_sq, a_neg = (np.array(v) for v in (got[2], got[3], auto[2], auto[3]))
        assert len(l_sq) == n_it
        e_sq = float((np.abs(l_sq - a_sq) / a_sq).max())
        e_neg = float(np.abs(l_neg - a_neg).max())
        e_c = float((got[0] - auto[0]).abs().max())
        e_y = gc.rel_close(got[1].cpu().numpy(), auto[1].cpu().numpy(), 1e-9)
        print(f'masked gd_circ16 ({kind}), {what} loop against autograd: loss_sq rel {e_sq:.3g}, '
              f'loss_neg abs {e_neg:.3g}, coeffs abs {e_c:.3g}, y_result rel {e_y:.3g}')
        assert e_sq <= 1e-9 and e_neg <= 1e-12 and e_c <= 1e-9 and e_y <= 1e-9
