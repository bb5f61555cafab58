"""Poisson fidelity on the GPU: the loss tail sphrt_poisson_residual_f64, the trace's Poisson
normal mode (sphrt_trace_normal_poisson_f64) behind MatrixFreeOperator.residual_gradient(
loss='poisson'), its two-trace deterministic form, and gd()'s direct loops with a PoissonLoss over
a stored Operator and over a MatrixFreeOperator.

References: for the loss tail, torch on the device — torch.autograd.grad through
poisson_nll_loss, and the documented summation tree over torch's own elementwise terms; for the
trace mode, op(x) and op.T of the weight formed in torch from that same forward; for one case per
geometry, the C oracle's own forward and adjoint (test_gpu_adjoint_paths._Ref); for the loops,
this project's autograd loop of the same problem.  Never the new entries.

Bounds, all derived here.  Atomic against op.T(psi): the two sum the same float64 terms in
another order, so per voxel n_rays * 2^-53 * op.T(|psi|).  Against the oracle, from the README's
1e-10 line-integral parity DELTA: the oracle adjoint of |ray_scale| * m * DELTA / (p + eps)^2 (the
weight's change under a forward off by DELTA) plus DELTA times the oracle adjoint of |psi| (the
lengths' own parity), under the asserted condition that every ray with m > 0 has an oracle
forward >= 0.05.  Deterministic: bitwise.  gd: bitwise the autograd loop's over the stored
Operator and the deterministic MatrixFreeOperator, losses within 1e-13 relative; the atomic
MatrixFreeOperator within test_gpu_robust_gradient's MARGIN and 1e-9 relative."""
import math

import numpy as np
import pytest
import torch as tr
import torch.nn.functional as F

import golden_cases as gc
from gpu_helpers import exact_stats
from test_gpu_adjoint_paths import (DGRID, F32, F64, SGRID, T_DYN, _check_coverage, _orbit, _rand,
                                    _Ref, _static_geom)
from test_gpu_matrix_free_deterministic import _bits, _flat_geom, _lattice_subset
from test_gpu_matrix_free_gradient import SCALE, _exact_waves, _ref_forward
from test_gpu_robust_gradient import MARGIN, _same_bits_or_nan
from test_gpu_weighted_gradient import _factors, _mask, _weights, circ16  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = 1e-8
DELTA = 1e-10           # the README's line-integral parity
GAIN = 4.0              # counts per unit line integral (checked with the oracle alone: the
P_MIN = 0.05            # condition below holds for seeds 301..310 on every geometry here)


def _op(grid, geom, gpu, **kw):
    from sph_raytracer_amd import MatrixFreeOperator
    return MatrixFreeOperator(grid, geom, device=gpu, **kw)


def _psi_t(p, m, rs, eps):
    """The Poisson weight in torch, in the header's operation order."""
    return rs + ((-rs) * m) / (p + eps)


# ---- 1. the loss tail alone ----------------------------------------------------------------------
def _tree_sum(terms, n_part):
    """The documented summation of sphrt_loss_partials(n) workgroups of 256 threads over `terms`
    (flat, on the device): thread t of workgroup b adds the elements b * 256 + t + k * n_part * 256
    for k = 0, 1, ... onto +0.0; the wave's 64 values by the xor butterfly 32 .. 1; the four wave
    totals, in order, onto +0.0.  (Padding with +0.0 changes no bit: a sum that started at +0.0 is
    never -0.0.)  -> the n_part partial sums."""
    n, sweep = terms.numel(), n_part * 256
    k = -(-n // sweep)
    pad = tr.zeros(k * sweep, dtype=F64, device=terms.device)
    pad[:n] = terms
    pad = pad.view(k, n_part, 256)
    acc = tr.zeros(n_part, 256, dtype=F64, device=terms.device)
    for i in range(k):
        acc = acc + pad[i]
    v = acc.view(n_part, 4, 64)
    lane = tr.arange(64, device=terms.device)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ off]
    out = tr.zeros(n_part, dtype=F64, device=terms.device)
    for w in range(4):
        out = out + v[:, w, 0]
    return out


# (yhat, y) pairs: q = yhat + eps of +0 (yhat = -eps), of eps itself (yhat = +-0), negative,
# denormal (with the denormal eps below), inf, NaN; each with y = 0 and with a count
_SPECIAL_YHAT = [0.0, -0.0, None, -1.0, -1e-310, 5e-324, 1e-310, float('inf'), -float('inf'),
                 float('nan'), 2.0]            # None: -eps


def _specials(eps):
    yh = [(-eps if v is None else v) for v in _SPECIAL_YHAT]
    return yh + yh, [0.0] * len(yh) + [3.0] * len(yh)


@pytest.mark.parametrize('n', [1, 63, 257, 262145, 786433])
@pytest.mark.parametrize('ydt', [F64, F32], ids=['y64', 'y32'])
@pytest.mark.parametrize('ordered', [False, True], ids=['in_order', 'order'])
def test_poisson_residual_kernel(ordered, ydt, n, gpu):
    """sphrt_poisson_residual_f64 past one element per thread (262144 threads a launch): r_scaled
    bitwise the gradient torch.autograd.grad leaves at p for (s * poisson_nll_loss(p, y)).sum() on
    the device, which is bitwise s + ((-s) * y) / (p + eps) — the header's sequence; the partial
    sums bitwise the documented tree over torch's own elementwise w * (p - y * log(p + eps)); a
    NaN for a NaN.  With counts, and with the special values of _specials under eps = 1e-8 and
    under a denormal eps (q itself denormal, q = +0)."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    g = tr.Generator(device='cpu').manual_seed(n)
    yhat0 = tr.rand(n, generator=g, dtype=F64) * 3
    yhat0[tr.rand(n, generator=g, dtype=F64) < 0.2] = 0            # rays that miss
    y0 = tr.poisson(2 * yhat0, generator=g)
    s = tr.randn(n, generator=g, dtype=F64).to(gpu)
    w = tr.rand(n, generator=g, dtype=F64).to(gpu)
    s[::5], w[::3] = 0, 0
    order = tr.randperm(n, generator=g).to(tr.int32).to(gpu) if ordered else None
    sel = order.long() if ordered else slice(None)
    n_part = lib.sphrt_loss_partials(n)
    for eps, special in ((EPS, False), (EPS, True), (1e-310, True), (0.5, False)):
        yhat, y = yhat0.clone(), y0.clone()
        if special:
            sy, sm = _specials(eps)
            k = min(n, len(sy))
            yhat[:k] = tr.tensor(sy[:k], dtype=F64)
            y[:k] = tr.tensor(sm[:k], dtype=F64)
        yhat, y = yhat.to(gpu), y.to(ydt).to(gpu)
        out = tr.empty(n, dtype=F64, device=gpu)
        part = tr.full((n_part,), float('nan'), dtype=F64, device=gpu)
        _lib.check(lib.sphrt_poisson_residual_f64(
            _lib.ptr(yhat), _lib.ptr(y), int(ydt == F64), n, eps, _lib.ptr(s), _lib.ptr(w),
            _lib.ptr(order), _lib.ptr(out), _lib.ptr(part), _lib.stream_of(gpu)),
            'poisson_residual')
        p = yhat.clone().requires_grad_()
        y64 = y.to(F64)
        nll = F.poisson_nll_loss(p, y64, log_input=False, full=False, eps=eps, reduction='none')
        auto, = tr.autograd.grad((s * nll).sum(), p)
        assert _same_bits_or_nan(auto, _psi_t(p.detach(), y64, s, eps))     # the header's sequence
        assert _same_bits_or_nan(out, auto[sel]), (eps, special)
        terms = (w * nll.detach())[sel]
        want = _tree_sum(terms, n_part)
        assert _same_bits_or_nan(part, want), (eps, special)
        if not special:
            assert bool(tr.isfinite(part).all()) and bool(tr.isfinite(out).all())


# ---- 2. the trace mode ---------------------------------------------------------------------------
CASES = ['S1-1ch', 'S1-3ch', 'S3-1ch', 'S3-3ch', 'lattice', 'serial-3ch', 'dynamic']


@pytest.fixture(scope='module')
def geoms():
    """case -> dict(grid, geom, ref, lead, div, n_t, x, fwd, m, w): the geometry, the oracle's trace
    of it, a density in [0.5, 1.5], the oracle's forward, Poisson counts of GAIN * that forward
    (a missed ray counts 0) and signed weights — built once per case, read-only."""
    cache = {}

    def get(case, gpu):
        if case in cache:
            return cache[case]
        from sph_raytracer_amd import ConeCircGeom, SphericalGrid
        seed = 301 + CASES.index(case)
        lead, div, n_t, okw = (), 0, 1, {}
        if case.startswith('S'):
            grid, geom = SphericalGrid(shape=SGRID), _static_geom(case[:2])
            lead = (3,) if case.endswith('3ch') else ()
        elif case == 'lattice':
            c = gc.load(gc.LATTICE_CASES[0])
            grid = gc.make_grid(c)
            geom = gc.FixtureGeom(dict(c, xs=c['xs'].copy(), rays=c['rays'].copy()))
        elif case == 'serial-3ch':
            grid, geom = _lattice_subset(1000, gpu)
            lead = (3,)
        else:
            grid = SphericalGrid(shape=DGRID)
            geom = sum(ConeCircGeom((24, 16), pos=p, fov=(0, 12)) for p in _orbit(T_DYN))
            n_t, okw = T_DYN, dict(dynamic=True)
        ref = _Ref(grid, geom)
        if n_t > 1:
            div = ref.n // T_DYN
            _check_coverage(ref, div=div, n_t=T_DYN)
        dshape = lead + tuple(grid.shape)
        mshape = lead + tuple(geom.shape)
        x = 0.5 + _rand(dshape, F64, seed, gpu)
        fwd = ref.forward(x, div=div) if div else _ref_forward(ref, x, 3 if lead else 1)
        fwd = np.asarray(fwd).reshape(-1)
        counts = np.random.default_rng(seed).poisson(GAIN * fwd).astype(np.float64)
        # the condition of the oracle-anchored bound, on the oracle alone
        assert (counts > 0).any() and (fwd[counts > 0] >= P_MIN).all()
        assert (counts[fwd == 0] == 0).all()
        m = tr.from_numpy(counts).reshape(mshape).to(gpu)
        w = _weights(mshape, seed + 50, gpu)
        cache[case] = dict(grid=grid, geom=geom, ref=ref, lead=lead, div=div, n_t=n_t, okw=okw, x=x,
                           fwd=fwd, m=m, w=w)
        return cache[case]

    return get


def _adjoint(op, c, y):
    return op.T(y, time_slices=True) if c['div'] else op.T(y)


def _check_paths(case, c, gpu):
    """The property of the trace that selects the case's code site (as test_gpu_robust_gradient)."""
    from sph_raytracer_amd.raytracer import _Plan
    if case not in ('lattice', 'serial-3ch'):
        return
    K = int(_Plan(c['grid'], gpu).K)
    deferred = exact_stats(c['grid'], c['geom'], gpu)[0]
    hit = int((np.diff(c['ref'].ptr) > 0).sum())
    if case == 'lattice':       # exact_walk_wave for the deferred rays, the trace kernel for the rest
        assert _exact_waves(K) == 4 and 0 < deferred < hit, (K, deferred, hit)
    else:                       # the lane-serial exact_walk: no wave's LDS holds the list
        assert K > 1815 and _exact_waves(K) == 0 and 0 < deferred <= hit, (K, deferred, hit)


@pytest.mark.parametrize('case', CASES)
def test_poisson_gradient_atomic(case, gpu, geoms):
    """yhat bitwise op(x); grad within the reordering bound of op.T(psi), psi formed in torch from
    that yhat; and within the oracle-anchored bound of the oracle's own forward and adjoint."""
    c = geoms(case, gpu)
    _check_paths(case, c, gpu)
    op = _op(c['grid'], c['geom'], gpu, **c['okw'])
    x, m, w, ref = c['x'], c['m'], c['w'], c['ref']
    ax = op(x)
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=w, loss='poisson', eps=EPS)
    assert yhat.shape == m.shape and yhat.dtype == F64 and yhat.device == gpu
    assert grad.shape == x.shape and grad.dtype == F64 and grad.device == gpu
    assert tr.equal(yhat, ax)
    rs = w.to(F64) * SCALE
    psi = _psi_t(ax, m, rs, EPS)
    assert bool(tr.isfinite(psi).all()) and bool((psi != 0).any())
    want, bound = _adjoint(op, c, psi), ref.n * 2.0 ** -53 * _adjoint(op, c, psi.abs())
    err = (grad - want).abs()
    print(f'poisson {case}: atomic against op.T(psi) max err {float(err.max()):.3g}, '
          f'max bound {float(bound.max()):.3g}, max |grad| {float(want.abs().max()):.3g}')
    assert bool((err <= bound).all()), float((err - bound).max())
    # without weights and eps: the scalar expanded once, torch's default eps
    _, g1 = op.residual_gradient(x, m, SCALE, loss='poisson')
    p1 = _psi_t(ax, m, tr.full_like(ax, SCALE), 1e-8)
    assert bool(((g1 - _adjoint(op, c, p1)).abs()
                 <= ref.n * 2.0 ** -53 * _adjoint(op, c, p1.abs())).all())
    # the oracle
    s = _factors(w, SCALE, m.shape)
    fwd, mm = c['fwd'], m.detach().cpu().numpy().reshape(-1)
    kw = dict(div=c['div'], n_t=c['n_t']) if c['div'] else dict(n_chan=3 if c['lead'] else 1)
    psi_o = s * (1.0 - mm / (fwd + EPS))
    g_o = np.asarray(ref.adjoint(tr.from_numpy(psi_o), **kw)).reshape(-1)
    b_o = np.asarray(ref.adjoint(tr.from_numpy(np.abs(s) * mm * DELTA / (fwd + EPS) ** 2), **kw)) \
        + DELTA * np.asarray(ref.adjoint(tr.from_numpy(np.abs(psi_o)), **kw))
    e_o = np.abs(grad.cpu().numpy().reshape(-1) - g_o)
    print(f'poisson {case}: against the oracle max err {e_o.max():.3g}, max bound {b_o.max():.3g}')
    assert np.abs(g_o).max() > 0 and (e_o <= b_o.reshape(-1)).all(), (e_o - b_o.reshape(-1)).max()


@pytest.mark.parametrize('case', CASES)
def test_poisson_gradient_deterministic(case, gpu, geoms):
    """op.deterministic: two traces — bitwise op(x) and op.T(psi) of the same operator, and equal
    bits on a second run."""
    c = geoms(case, gpu)
    op = _op(c['grid'], c['geom'], gpu, deterministic=True, **c['okw'])
    x, m, w = c['x'], c['m'], c['w']
    ax = op(x)
    yh, g = op.residual_gradient(x, m, SCALE, weights=w, loss='poisson', eps=EPS)
    yh2, g2 = op.residual_gradient(x, m, SCALE, weights=w, loss='poisson', eps=EPS)
    assert tr.equal(yh, ax) and tr.equal(yh, yh2) and tr.equal(g, g2)
    psi = _psi_t(ax, m, w.to(F64) * SCALE, EPS)
    assert tr.equal(g, _adjoint(op, c, psi))
    assert g.shape == x.shape and bool(g.any())


def test_deterministic_split_batch(gpu, geoms):
    """The documented two-trace sequence through the C ABI with the rays split in two: both halves'
    weights added into one accumulator under one record (formed from the whole batch's weights)
    give the whole batch's bits."""
    from sph_raytracer_amd import _lib
    c = geoms('S1-1ch', gpu)
    grid, geom, x, m, w = c['grid'], c['geom'], c['x'], c['m'], c['w']
    op = _op(grid, geom, gpu, deterministic=True)
    lib, vol, n = _lib.load(), math.prod(SGRID), c['ref'].n
    yh, g = op.residual_gradient(x, m, SCALE, weights=w, loss='poisson', eps=EPS)
    st = _lib.stream_of(gpu)
    rs = (w.to(F64) * SCALE).reshape(-1).contiguous()
    xf, mf = x.reshape(-1).contiguous(), m.reshape(-1).contiguous()
    rec = tr.zeros(2, dtype=tr.int64, device=gpu)
    out = tr.empty(vol, dtype=F64, device=gpu)
    acc = tr.zeros(2 * vol, dtype=tr.int64, device=gpu)
    yhat, psi = tr.empty(n, dtype=F64, device=gpu), tr.empty(n, dtype=F64, device=gpu)
    bounds = ((0, n // 2), (n // 2, n))
    halves = [_op(grid, _flat_geom(geom, np.arange(lo, hi)), gpu, deterministic=True)
              for lo, hi in bounds]
    for h, (lo, hi) in zip(halves, bounds):
        plan, batch, ws = h._parts
        _lib.check(lib.sphrt_trace_integrate_f64(plan.handle, batch.desc, _lib.ptr(xf), 1, vol, 0,
                                                 _lib.ptr(yhat[lo:hi]), hi - lo, _lib.ptr(ws),
                                                 ws.numel(), st), 'i')
    part = tr.empty(lib.sphrt_loss_partials(n), dtype=F64, device=gpu)
    _lib.check(lib.sphrt_poisson_residual_f64(_lib.ptr(yhat), _lib.ptr(mf), 1, n, EPS, _lib.ptr(rs),
                                              _lib.ptr(rs), None, _lib.ptr(psi), _lib.ptr(part), st),
               'p')
    L = 2.0 * float(grid.r_b[-1])
    _lib.check(lib.sphrt_fixed_scale_f64(_lib.ptr(psi), n, L, None, 0, 0.0, _lib.ptr(rec), st), 's')
    for h, (lo, hi) in zip(halves, bounds):
        plan, batch, ws = h._parts
        _lib.check(lib.sphrt_trace_backproject_fixed_f64(
            plan.handle, batch.desc, _lib.ptr(psi[lo:hi]), 1, hi - lo, 0, _lib.ptr(acc), vol,
            _lib.ptr(rec), _lib.ptr(ws), ws.numel(), st), 'b')
    _lib.check(lib.sphrt_fixed_finalize_f64(_lib.ptr(acc), vol, _lib.ptr(rec), _lib.ptr(out), st), 'f')
    assert tr.equal(yhat.reshape(geom.shape), yh) and tr.equal(out.reshape(SGRID), g)


def test_host_tensors_and_float32(gpu, geoms):
    """Host tensors in, host tensors out; float32 in, float32 out (computed in float64)."""
    c = geoms('S3-3ch', gpu)
    op = _op(c['grid'], c['geom'], gpu)
    x, m, w = c['x'], c['m'], c['w']
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=w, loss='poisson', eps=0.5)
    yc, g_c = op.residual_gradient(x.cpu(), m.cpu(), SCALE, weights=w[0].cpu().float(),
                                   loss='poisson', eps=0.5)
    assert yc.device.type == 'cpu' and g_c.device.type == 'cpu' and g_c.dtype == F64
    assert tr.equal(yc, yhat.cpu())
    psi = _psi_t(yhat, m, (w[0].float().to(F64) * SCALE).expand(m.shape), 0.5)
    bound = c['ref'].n * 2.0 ** -53 * op.T(psi.abs())
    assert bool(((g_c.to(gpu) - op.T(psi)).abs() <= bound).all())
    y32, g32 = op.residual_gradient(x.float(), m.float(), SCALE, weights=w, loss='poisson', eps=0.5)
    assert y32.dtype == F32 and g32.dtype == F32 and y32.shape == m.shape and g32.shape == x.shape
    ax32 = op(x.float().to(F64))
    p32 = _psi_t(ax32, m.float().to(F64), w.to(F64) * SCALE, 0.5)
    want, reorder = op.T(p32), c['ref'].n * 2.0 ** -53 * op.T(p32.abs())
    # (the float64 sum within the reordering bound, then one rounding to float32)
    assert bool(((g32.to(F64) - want).abs() <= 2.0 ** -24 * (want.abs() + reorder) + reorder).all())


# ---- 3. gd ---------------------------------------------------------------------------------------
REGS = ['alone', 'neg', 'neg_smooth']


@pytest.fixture(scope='module')
def counts16(circ16, gpu):  # noqa: F811
    """circ16's grid and stored Operator with photon counts of 6 * op(1 + phantom) and a start in
    [2, 3): Adam at lr 0.02 moves a coefficient by at most lr * max(1, (1 - b1) / sqrt(1 - b2)) =
    0.064 an iteration, 1.6 over 25, so every density stays positive and p + eps > 0 throughout."""
    grid, geom, op, meas = circ16
    y = tr.poisson(6 * (meas + op(tr.ones(grid.shape, dtype=F64, device=gpu))).cpu(),
                   generator=tr.Generator().manual_seed(331)).to(gpu)
    assert bool((y > 0).any()) and bool((y == 0).any())
    c0 = 2 + _rand(grid.shape, F64, 332, gpu)
    return grid, geom, op, y, c0


def _terms(regs, pm, lam=1, fid=None):
    from sph_raytracer_amd.loss import NegRegularizer, PoissonLoss, SmoothRegularizer
    fid = lam * PoissonLoss(eps=EPS, projection_mask=pm) if fid is None else fid
    fns = [fid]
    if regs != 'alone':
        fns.append(2 * NegRegularizer())
    if regs == 'neg_smooth':
        fns.append(0.5 * SmoothRegularizer(weights=(1, 0.5, 2)))
    return fns


def _run_gd(op, y, grid, c0, fns, n_it=25):
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.model import FullyDenseModel
    c, yh, hist = retrieval.gd(op, y.clone(), FullyDenseModel(grid), coeffs=c0.clone(), lr=0.02,
                               num_iterations=n_it, loss_fns=fns, progress_bar=False)
    losses = [list(hist[fn]) for fn in fns]
    assert all(len(v) == n_it and np.isfinite(v).all() for v in losses)
    assert float(c.detach().min()) > 0                                   # p + eps > 0 throughout
    return c.detach().clone(), yh.detach().clone(), losses


def _spy(monkeypatch):
    from sph_raytracer_amd import retrieval
    calls, direct = [], retrieval._gd_direct
    monkeypatch.setattr(retrieval, '_gd_direct', lambda *a, **k: calls.append(1) or direct(*a, **k))
    return calls


def _no_plans(mp):
    from sph_raytracer_amd import retrieval
    mp.setattr(retrieval, '_direct_plan', lambda *a: None)
    mp.setattr(retrieval, '_fused_plan', lambda *a: None)


@pytest.mark.parametrize('ydt', [F64, F32], ids=['y64', 'y32'])
@pytest.mark.parametrize('regs', REGS)
@pytest.mark.parametrize('mask', ['unit', 'zero_one', 'float32', 'broadcast'])
def test_gd_direct_poisson_matches_autograd_stored(mask, regs, ydt, gpu, monkeypatch, counts16):
    """gd() with a PoissonLoss (+ NegRegularizer, + SmoothRegularizer) over a stored Operator takes
    `_gd_direct` and gives the autograd loop's coefficients and reconstruction bitwise, its loss
    histories within 1e-13 relative — with the measurements permuted into trace order and, with
    that declined, through the kernel's `order` argument."""
    from sph_raytracer_amd import Operator
    grid, geom, op, y64, c0 = counts16
    y = y64.to(ydt)
    pm = 1 if mask == 'unit' else _mask(mask, y.shape, gpu)
    lam = 0.5 if regs == 'neg' else 1
    calls = _spy(monkeypatch)
    ca, ya, ha = _run_gd(op, y, grid, c0, _terms(regs, pm, lam))
    assert len(calls) == 1
    with monkeypatch.context() as mp:
        _no_plans(mp)
        cb, yb, hb = _run_gd(op, y, grid, c0, _terms(regs, pm, lam))
    assert len(calls) == 1
    assert len(ha) == len(hb) == 1 + REGS.index(regs) and ha[0][-1] < ha[0][0]
    for la, lb in zip(ha, hb):
        assert np.allclose(la, lb, rtol=1e-13, atol=0), (la, lb)
    assert tr.equal(ca, cb) and tr.equal(ya, yb) and not tr.equal(ca, c0)
    # the kernel's `order` branch: the trace-position forward declined
    assert op._adjoint_trace_order() is not None
    monkeypatch.setattr(Operator, '_trace_position_rows', lambda self, sd: None)
    cc, yc, hc = _run_gd(op, y, grid, c0, _terms(regs, pm, lam))
    assert len(calls) == 2
    for lc_, lb in zip(hc, hb):
        assert np.allclose(lc_, lb, rtol=1e-13, atol=0), (lc_, lb)
    assert tr.equal(cc, cb) and tr.equal(yc, yb)


@pytest.mark.parametrize('regs', REGS)
@pytest.mark.parametrize('mask', ['unit', 'zero_one', 'float32', 'broadcast'])
def test_gd_direct_poisson_matrix_free(mask, regs, gpu, monkeypatch, counts16):
    """gd() with a PoissonLoss over a MatrixFreeOperator takes `_gd_direct`: atomic, one
    _poisson_into per iteration and no adjoint, iterates within MARGIN of the autograd loop's and
    losses within 1e-9 relative; deterministic, one forward and one fixed-point back-projection per
    iteration (two traces), iterates bitwise the autograd loop's over the same operator, losses
    within 1e-13 relative, and two runs with equal bits."""
    grid, geom, _, y, c0 = counts16
    op = _op(grid, geom, gpu)
    pm = 1 if mask == 'unit' else _mask(mask, y.shape, gpu)
    calls = _spy(monkeypatch)
    seen = {'poisson': 0, 'forward': 0, 'back': 0, 'adjoint': 0}
    for name, key in (('_poisson_into', 'poisson'), ('_forward_into', 'forward'),
                      ('_backproject_fixed_into', 'back'), ('_apply_adjoint', 'adjoint')):
        def wrap(*a, _f=getattr(op, name), _k=key, **k):
            seen[_k] += 1
            return _f(*a, **k)
        monkeypatch.setattr(op, name, wrap)
    n_it = 25
    fused = _run_gd(op, y, grid, c0, _terms(regs, pm))
    assert len(calls) == 1 and seen == {'poisson': n_it, 'forward': 0, 'back': 0, 'adjoint': 0}
    with monkeypatch.context() as mp:
        _no_plans(mp)
        auto = _run_gd(op, y, grid, c0, _terms(regs, pm))
    assert len(calls) == 1 and seen['adjoint'] == n_it and seen['poisson'] == n_it
    e_c = float((fused[0] - auto[0]).abs().max())
    e_y = float((fused[1] - auto[1]).abs().max() / auto[1].abs().max())
    print(f'poisson gd ({mask}, {regs}), atomic loop against autograd: coeffs abs {e_c:.3g}, '
          f'y_result rel {e_y:.3g}')
    assert e_c <= MARGIN and e_y <= MARGIN
    for la, lb in zip(fused[2], auto[2]):
        assert np.allclose(la, lb, rtol=1e-9, atol=1e-12), (la, lb)
    op.deterministic = True
    det = [_run_gd(op, y, grid, c0, _terms(regs, pm)) for _ in range(2)]
    assert len(calls) == 3 and seen['forward'] == 2 * n_it and seen['back'] == 2 * n_it
    assert seen['poisson'] == n_it and seen['adjoint'] == n_it
    assert tr.equal(det[0][0], det[1][0]) and tr.equal(det[0][1], det[1][1])
    assert [_bits(v) for v in det[0][2]] == [_bits(v) for v in det[1][2]]
    with monkeypatch.context() as mp:
        _no_plans(mp)
        dauto = _run_gd(op, y, grid, c0, _terms(regs, pm))
    op.deterministic = False
    assert len(calls) == 3 and seen['adjoint'] == 2 * n_it
    assert tr.equal(det[0][0], dauto[0]) and tr.equal(det[0][1], dauto[1])
    for la, lb in zip(det[0][2], dauto[2]):
        assert np.allclose(la, lb, rtol=1e-13, atol=0), (la, lb)


def test_loop_terms_accept_and_decline(gpu, counts16):
    """Exactly one PoissonLoss, scalar lam, unit volume_mask: both plans take it, with the
    regularisers under the ordering rule; a subclass, a tensor lam, a volume_mask, a second
    fidelity term and a dynamic operator decline to the autograd loop."""
    from sph_raytracer_amd import MatrixFreeOperator, SphericalGrid, retrieval
    from sph_raytracer_amd.loss import (NegRegularizer, PoissonLoss, SmoothRegularizer,
                                        SquareLoss)
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom, op, y, c0 = counts16
    model = FullyDenseModel(grid)
    c = c0.clone()
    mfo = MatrixFreeOperator(grid, geom, device=gpu)
    good = _mask('zero_one', y.shape, gpu)
    ones = tr.ones(grid.shape, dtype=F64, device=gpu)

    def plans(fns):
        return (retrieval._direct_plan(op, y, model, c, fns, [c]),
                retrieval._fused_plan(mfo, y, model, c, fns, [c]))

    for kw in ({}, dict(projection_mask=good), dict(projection_mask=good.bool()),
               dict(projection_mask=good[0].float()), dict(eps=0.5)):
        fid, neg, sm = 0.5 * PoissonLoss(**kw), NegRegularizer(), SmoothRegularizer()
        assert plans([fid]) == ((fid, None),) * 2
        assert plans([fid, neg]) == ((fid, neg),) * 2 and plans([neg, fid]) == ((fid, neg),) * 2
        assert plans([fid, neg, sm]) == ((fid, neg, sm),) * 2
        assert plans([sm, fid]) == ((fid, None, sm),) * 2
        assert plans([neg, fid, sm]) == (None,) * 2           # (the ordering rule)
    assert plans([PoissonLoss(volume_mask=ones)]) == (None,) * 2
    assert plans([PoissonLoss(projection_mask=good.cpu())]) == (None,) * 2
    assert plans([PoissonLoss(projection_mask=2)]) == (None,) * 2
    assert plans([PoissonLoss() * tr.tensor(0.5, device=gpu)]) == (None,) * 2
    assert plans([PoissonLoss() * tr.tensor(0.5)]) == (None,) * 2
    assert plans([PoissonLoss(), SquareLoss()]) == (None,) * 2
    assert plans([PoissonLoss(), PoissonLoss()]) == (None,) * 2
    assert plans([PoissonLoss(use_grad=False)]) == (None,) * 2

    class MyPoisson(PoissonLoss):
        pass

    assert plans([MyPoisson()]) == (None,) * 2
    dgrid, sgeom = SphericalGrid(shape=DGRID), _static_geom('S1')
    dop = MatrixFreeOperator(dgrid, sgeom, device=gpu)
    dc = tr.ones(DGRID, dtype=F64, device=gpu)
    yd = _rand(sgeom.shape, F64, 333, gpu)
    assert retrieval._fused_plan(dop, yd, FullyDenseModel(dgrid), dc, [PoissonLoss()], [dc]) is None


def test_declined_terms_run_the_autograd_loop(gpu, monkeypatch, counts16):
    """A subclass, a tensor lam and a volume_mask: gd() runs, and `_gd_direct` does not."""
    from sph_raytracer_amd.loss import PoissonLoss
    grid, geom, op, y, c0 = counts16
    calls = _spy(monkeypatch)

    class MyPoisson(PoissonLoss):
        pass

    ones = tr.ones(grid.shape, dtype=F64, device=gpu)
    base = _run_gd(op, y, grid, c0, [PoissonLoss(eps=EPS)], n_it=3)
    assert len(calls) == 1
    for fid in (MyPoisson(eps=EPS), PoissonLoss(eps=EPS) * tr.tensor(1.0, dtype=F64, device=gpu),
                PoissonLoss(eps=EPS, volume_mask=ones)):
        got = _run_gd(op, y, grid, c0, [fid], n_it=3)
        assert len(calls) == 1
        assert tr.equal(got[0], base[0])          # (the same arithmetic: bitwise the direct loop's)
