"""Robust fidelity on the GPU: MatrixFreeOperator.residual_gradient(loss='abs' | 'huber') (the
trace's robust normal modes, sphrt_trace_normal_robust_f64 / _fixed_f64), the robust loss tail
sphrt_robust_residual_f64, and gd()'s direct loops with an AbsLoss or a HuberLoss over a stored
Operator and over a MatrixFreeOperator.

References: the C oracle's own trace (test_gpu_adjoint_paths._Ref: forward, and adjoint of
s_i * psi(fwd_i - m_i) formed in numpy from the oracle's forward); for the loops, this project's
autograd loop of the same problem; for the loss tail, torch's elementwise ops on the device.
Never the new entries.

Conditions, asserted on the oracle's residuals alone (`_conditions`): under ABS every residual
not deliberately zeroed is farther from zero than 1e-6 x max|fwd|, so no sign can flip inside
the 1e-10 parity band; under HUBER delta is the median |residual|, and at least a fifth of the
rays fall in each branch.

Tolerances (the project's own): float64 within 1e-10 x max|reference|, float32 within 1e-5 x;
against the two separate calls op.T(s * psi(op(x) - m)) rtol 1e-12 and atol 1e-12 x max; yhat
bitwise the float64 forward; the stored loop's iterates bitwise the autograd loop's and its
losses within 1e-13 relative; the fused loop within 1e-9 of the autograd loop; the deterministic
form additionally within half a quantum per add of the oracle."""
import math

import numpy as np
import pytest
import torch as tr
import torch.nn.functional as F

import golden_cases as gc
from gpu_helpers import exact_stats
from test_gpu_adjoint_paths import (DGRID, F32, F64, SGRID, T_DYN, TOL, _assert_close,
                                    _check_coverage, _orbit, _rand, _Ref, _static_geom)
from test_gpu_matrix_free_deterministic import _bits, _flat_geom, _lattice_subset
from test_gpu_matrix_free_gradient import (SCALE, _assert_separate_agree, _exact_waves,
                                           _gd_circ16, _ref_forward)
from test_gpu_weighted_gradient import _factors, _mask, _weights, circ16  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = ['abs', 'huber']
ABS, HUBER = 1, 2
MARGIN = 1e-6


def _op(grid, geom, gpu, **kw):
    from sph_raytracer_amd import MatrixFreeOperator
    return MatrixFreeOperator(grid, geom, device=gpu, **kw)


def _conditions(kind, fwd, m, zeroed=None):
    """The oracle's residuals fwd - m (numpy, flat) -> delta (None for 'abs'), the conditions of
    the module docstring asserted.  `zeroed`: indices of the rays whose residual the test makes
    exactly zero on the device."""
    r = fwd.reshape(-1) - m.detach().cpu().double().numpy().reshape(-1)
    keep = np.ones(r.size, dtype=bool)
    if zeroed is not None:
        keep[zeroed] = False
    if kind == 'abs':
        assert np.abs(r[keep]).min() > MARGIN * np.abs(fwd).max(), np.abs(r[keep]).min()
        return None
    delta = float(np.median(np.abs(r[keep])))
    inner = float((np.abs(r[keep]) < delta).mean())
    assert delta > 0 and 0.2 <= inner <= 0.8, (delta, inner)
    return delta


def _psi(kind, r, delta):
    return np.sign(r) if kind == 'abs' else np.clip(r, -delta, delta)


def _psi_t(kind, r, delta):
    return tr.sign(r) if kind == 'abs' else tr.clamp(r, -delta, delta)


def _ref_robust(ref, kind, delta, fwd, m, s, zeroed=None, **kw):
    """The oracle's A^T(s * psi(fwd - m)) from its own forward `fwd` (numpy); psi exactly zero at
    the `zeroed` rays."""
    r = fwd.reshape(-1) - m.detach().cpu().double().numpy().reshape(-1)
    if zeroed is not None:
        r[zeroed] = 0.0
    return ref.adjoint(tr.from_numpy(s * _psi(kind, r, delta)), **kw)


def _kw(kind, delta):
    return dict(loss=kind) if kind == 'abs' else dict(loss=kind, delta=delta)


def _zero_some(m, ax, seed):
    """m with every 7th-ish element replaced by op(x)'s own bits -> (m, flat indices)."""
    idx = np.flatnonzero(np.random.default_rng(seed).random(m.numel()) < 0.15)
    assert 0 < idx.size < m.numel()
    m = m.clone()
    it = tr.from_numpy(idx).to(m.device)
    m.view(-1)[it] = ax.reshape(-1)[it]
    return m, idx


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


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('lead', [(), (3,)], ids=['1ch', '3ch'])
@pytest.mark.parametrize('name', ['S1', 'S3'])
def test_static_robust_gradient(name, lead, kind, gpu, static_cases):
    grid, geom, ref, op = static_cases(name, gpu)
    n_chan = 3 if lead else 1
    x = _rand(lead + SGRID, F64, 241, gpu)
    ax = op(x)
    m, zeroed = _zero_some(_rand(lead + tuple(geom.shape), F64, 242, gpu) * 3, ax, 243)
    w = _weights(m.shape, 244, gpu)
    fwd = _ref_forward(ref, x, n_chan)
    delta = _conditions(kind, fwd, m, zeroed)
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=w, **_kw(kind, delta))
    assert yhat.shape == m.shape and yhat.dtype == F64 and yhat.device == gpu
    assert grad.shape == x.shape and grad.dtype == F64 and grad.device == gpu
    assert tr.equal(yhat, ax)
    s = _factors(w, SCALE, m.shape)
    _assert_close(grad, _ref_robust(ref, kind, delta, fwd, m, s, zeroed, n_chan=n_chan), TOL[F64])
    _assert_separate_agree(grad, op.T((w * SCALE) * _psi_t(kind, ax - m, delta)))
    # without weights: the scalar expanded once
    _, g1 = op.residual_gradient(x, m, SCALE, **_kw(kind, delta))
    _assert_close(g1, _ref_robust(ref, kind, delta, fwd, m, np.full(m.numel(), SCALE), zeroed,
                                  n_chan=n_chan), TOL[F64])
    # float32 in, float32 out (float32 weights too; no zeroed rays: a float32 copy of op(x) is
    # not the float64 sum the kernel subtracts it from)
    x32, w32 = x.float(), w.float()
    m32 = (_rand(lead + tuple(geom.shape), F64, 245, gpu) * 3).float()
    fwd32 = _ref_forward(ref, x32, n_chan)
    d32 = _conditions(kind, fwd32, m32)
    y32, g32 = op.residual_gradient(x32, m32, SCALE, weights=w32, **_kw(kind, d32))
    assert y32.dtype == F32 and g32.dtype == F32 and y32.shape == m.shape and g32.shape == x.shape
    _assert_close(y32, fwd32, TOL[F32])
    _assert_close(g32, _ref_robust(ref, kind, d32, fwd32, m32, _factors(w32, SCALE, m.shape),
                                   n_chan=n_chan), TOL[F32])


@pytest.mark.parametrize('kind', KINDS)
def test_exact_zero_residuals_contribute_nothing(kind, gpu, static_cases):
    """m = op(x) bitwise on every ray: psi is 0 (ABS: sign(0) = 0), so grad is exactly zero
    whatever the finite weights; host tensors in, host tensors out."""
    grid, geom, ref, op = static_cases('S3', gpu)
    x = _rand((3,) + SGRID, F64, 246, gpu)
    ax = op(x)
    w = _weights(ax.shape, 247, gpu) * 1e3
    y0, g0 = op.residual_gradient(x, ax, SCALE, weights=w, **_kw(kind, 0.25))
    assert tr.equal(y0, ax) and g0.shape == x.shape and not g0.any() and not g0.isnan().any()
    m = _rand(ax.shape, F64, 248, 'cpu') * 3
    fwd = _ref_forward(ref, x, 3)
    delta = _conditions(kind, fwd, m)
    wc = _weights(tuple(geom.shape)[1:], 249, 'cpu', F32)           # broadcast, on the host
    yc, gc_ = op.residual_gradient(x.cpu(), m, weights=wc, **_kw(kind, delta))
    assert yc.device.type == 'cpu' and gc_.device.type == 'cpu' and gc_.dtype == F64
    _assert_close(gc_, _ref_robust(ref, kind, delta, fwd, m, _factors(wc, 1.0, m.shape),
                                   n_chan=3), TOL[F64])


# ---- 2. both code sites --------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('deterministic', [False, True], ids=['atomic', 'fixed'])
def test_wave_path_on_lattice_ties(deterministic, kind, gpu):
    """consume_list behind every wave-level path: a tie lattice, whose deferred rays go through
    exact_walk_wave (4 waves per ray at this K) and the rest through the trace kernel."""
    from sph_raytracer_amd.raytracer import _Plan
    case = gc.load(gc.LATTICE_CASES[0])
    grid = gc.make_grid(case)
    geom = gc.FixtureGeom(dict(case, xs=case['xs'].copy(), rays=case['rays'].copy()))
    assert _exact_waves(int(_Plan(grid, gpu).K)) == 4
    deferred = exact_stats(grid, geom, gpu)[0]
    ref = _Ref(grid, geom)
    hit = int((np.diff(ref.ptr) > 0).sum())
    assert 0 < deferred < hit, (deferred, hit)            # both sites run
    op = _op(grid, geom, gpu, deterministic=deterministic)
    x = _rand(grid.shape, F64, 250, gpu)
    ax = op(x)
    m, zeroed = _zero_some(_rand(geom.shape, F64, 251, gpu) * 3, ax, 252)
    w = _weights(m.shape, 253, gpu)
    fwd = _ref_forward(ref, x, 1)
    delta = _conditions(kind, fwd, m, zeroed)
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=w, **_kw(kind, delta))
    assert tr.equal(yhat, ax)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_robust(ref, kind, delta, fwd, m, _factors(w, SCALE, m.shape), zeroed),
                  TOL[F64])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('deterministic', [False, True], ids=['atomic', 'fixed'])
def test_serial_exact_walk_with_channels(deterministic, kind, gpu):
    """The serial exact_walk (K = 2013 > 1815: no wave's LDS holds the list;
    exact_kernel<NORMAL_R*>) with three channels: the scattering walk re-forms psi per segment
    from every channel's own residual and weighs it with that channel's own factor."""
    from sph_raytracer_amd.raytracer import _Plan
    grid, geom = _lattice_subset(1000, gpu)
    K = int(_Plan(grid, gpu).K)
    assert K == 2 * (1000 + 1) + 2 * 5 + 5 + 1 and K > 1815 and _exact_waves(K) == 0
    ref = _Ref(grid, geom)
    deferred = exact_stats(grid, geom, gpu)[0]
    assert 0 < deferred <= int((np.diff(ref.ptr) > 0).sum())
    op = _op(grid, geom, gpu, deterministic=deterministic)
    x = _rand((3,) + tuple(grid.shape), F64, 263, gpu)
    ax = op(x)
    m, zeroed = _zero_some(_rand((3,) + tuple(geom.shape), F64, 264, gpu) * 3, ax, 265)
    w = _weights(m.shape, 266, gpu)
    assert not tr.equal(w[0], w[1])                    # (a factor per channel, not per ray)
    fwd = _ref_forward(ref, x, 3)
    delta = _conditions(kind, fwd, m, zeroed)
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=w, **_kw(kind, delta))
    assert tr.equal(yhat, ax)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_robust(ref, kind, delta, fwd, m, _factors(w, SCALE, m.shape), zeroed,
                                    n_chan=3), TOL[F64])


# ---- 3. time-paired dynamic grid -----------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('deterministic', [False, True], ids=['atomic', 'fixed'])
def test_dynamic_view_time_pairing(deterministic, kind, gpu):
    """5 views <-> 5 time slices (ray_chan_div > 0): ray i's factor is ray_scale[i]."""
    from sph_raytracer_amd import ConeCircGeom, SphericalGrid
    grid = SphericalGrid(shape=DGRID)
    geom = sum(ConeCircGeom((24, 16), pos=p, fov=(0, 12)) for p in _orbit(T_DYN))
    ref = _Ref(grid, geom)
    div = ref.n // T_DYN
    _check_coverage(ref, div=div, n_t=T_DYN)
    op = _op(grid, geom, gpu, dynamic=True, deterministic=deterministic)
    assert op._layout(DGRID) == (1, div, tuple(geom.shape))
    x = _rand(DGRID, F64, 254, gpu)
    ax = op(x)
    m, zeroed = _zero_some(_rand(geom.shape, F64, 255, gpu) * 3, ax, 256)
    w = _weights(m.shape, 257, gpu)
    fwd = ref.forward(x, div=div)
    delta = _conditions(kind, fwd, m, zeroed)
    yhat, grad = op.residual_gradient(x, m, SCALE, weights=w, **_kw(kind, delta))
    assert yhat.shape == tuple(geom.shape) and grad.shape == DGRID
    assert tr.equal(yhat, ax)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_robust(ref, kind, delta, fwd, m, _factors(w, SCALE, m.shape), zeroed,
                                    div=div, n_t=T_DYN), TOL[F64])
    _assert_separate_agree(grad, op.T((w * SCALE) * _psi_t(kind, ax - m, delta),
                                      time_slices=True))


# ---- 4. deterministic mode -----------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_deterministic_bits_split_and_bound(kind, gpu, static_cases):
    """Two calls give equal bits; the two halves of the rays added into one accumulator under one
    record (through the C ABI) give the whole batch's bits; the result is within half a quantum
    per add of the oracle (on top of the oracle's own float64 tolerance), the quantum at most
    2^-60 x the bound max|s| * fa of a term."""
    from sph_raytracer_amd import _lib
    grid, geom, ref, _ = static_cases('S1', gpu)
    op = _op(grid, geom, gpu, deterministic=True)
    lib, vol, n = _lib.load(), math.prod(SGRID), ref.n
    x = _rand(SGRID, F64, 258, gpu)
    ax = op(x)
    m, zeroed = _zero_some(_rand(geom.shape, F64, 259, gpu) * 3, ax, 260)
    w = _weights(m.shape, 261, gpu)
    fwd = _ref_forward(ref, x, 1)
    delta = _conditions(kind, fwd, m, zeroed)
    yh, g = op.residual_gradient(x, m, SCALE, weights=w, **_kw(kind, delta))
    yh2, g2 = op.residual_gradient(x, m, SCALE, weights=w, **_kw(kind, delta))
    assert tr.equal(yh, ax) and tr.equal(yh, yh2) and tr.equal(g, g2)
    # the error bound
    s = _factors(w, SCALE, m.shape)
    want = np.asarray(_ref_robust(ref, kind, delta, fwd, m, s, zeroed)).reshape(-1)
    L = 2.0 * float(grid.r_b[-1])
    fa = L if kind == 'abs' else delta * L
    quantum = 2.0 * np.abs(s).max() * fa * 2.0 ** -61       # 2^(E - 61), 2^E <= 2 B
    adds = np.bincount(ref.vox, minlength=vol)
    err = np.abs(g.cpu().numpy().reshape(-1) - want)
    assert (err <= TOL[F64] * np.abs(want).max() + 0.5 * quantum * adds).all(), err.max()
    # the split batch
    halves = [_op(grid, _flat_geom(geom, np.arange(lo, hi)), gpu, deterministic=True)
              for lo, hi in ((0, n // 2), (n // 2, n))]
    st = _lib.stream_of(gpu)
    rs = (w.to(F64) * SCALE).reshape(-1).contiguous()
    xf, mf = x.reshape(-1), m.reshape(-1)
    rec = tr.zeros(2, dtype=tr.int64, device=gpu)
    out = tr.empty(vol, dtype=F64, device=gpu)
    acc = tr.zeros(2 * vol, dtype=tr.int64, device=gpu)
    yhat = tr.empty(n, dtype=F64, device=gpu)
    _lib.check(lib.sphrt_fixed_scale_f64(_lib.ptr(rs), n, fa, None, 0, 0.0, _lib.ptr(rec), st), 's')
    for h, (lo, hi) in zip(halves, ((0, n // 2), (n // 2, n))):
        plan, batch, ws = h._parts
        mm, ss, yy = mf[lo:hi].contiguous(), rs[lo:hi].contiguous(), yhat[lo:hi]
        _lib.check(lib.sphrt_trace_normal_robust_fixed_f64(
            plan.handle, batch.desc, _lib.ptr(xf), _lib.ptr(mm), _lib.ptr(ss),
            ABS if kind == 'abs' else HUBER, delta or 0.0, 1, vol, 0, _lib.ptr(yy), hi - lo,
            _lib.ptr(acc), _lib.ptr(rec), _lib.ptr(ws), ws.numel(), st), 'n')
    _lib.check(lib.sphrt_fixed_finalize_f64(_lib.ptr(acc), vol, _lib.ptr(rec), _lib.ptr(out), st), 'f')
    assert tr.equal(yhat.reshape(geom.shape), yh) and tr.equal(out.reshape(SGRID), g)


# ---- 5. the robust loss tail alone ---------------------------------------------------------------
SPECIAL = [0.0, -0.0, float('inf'), -float('inf'), float('nan'), 5e-324, -5e-324, 1e-310, 0.25,
           -0.25]                      # residuals (y = 0 there); 0.25 is delta itself


def _same_bits_or_nan(a, b):
    return bool(((a.view(tr.int64) == b.view(tr.int64)) | (a.isnan() & b.isnan())).all())


@pytest.mark.parametrize('n', [1, 63, 257, 262145, 786433])
@pytest.mark.parametrize('ydt', [F64, F32], ids=['y64', 'y32'])
@pytest.mark.parametrize('ordered', [False, True], ids=['in_order', 'order'])
@pytest.mark.parametrize('kind', KINDS)
def test_robust_residual_kernel(kind, ordered, ydt, n, gpu):
    """sphrt_robust_residual_f64 past one element per thread (262144 threads a launch): r_scaled
    bitwise torch's sign(r) * s / clamp(r, +-delta) * s on the device (a NaN for a NaN), equal in
    value to autograd's own backward of s * |y - f| and s * huber_loss(f, y) (which differ from
    it only in the sign of a zero under ABS) — for residuals of +-0, +-inf, NaN and denormals
    too; the partial sums within 1e-13 relative of torch's sum on finite data, and non-finite
    exactly when torch's is."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    delta = 0.25
    code, dl = (ABS, 0.0) if kind == 'abs' else (HUBER, delta)
    g = tr.Generator(device='cpu').manual_seed(n)
    yhat0 = (tr.randn(n, generator=g, dtype=F64) * 0.4).to(gpu)
    y = (tr.randn(n, generator=g, dtype=F64) * 0.4).to(ydt).to(gpu)
    s = tr.randn(n, generator=g, dtype=F64).to(gpu)
    w = tr.rand(n, generator=g, dtype=F64).to(gpu)
    s[::5], w[::3] = 0, 0
    order = tr.randperm(n, generator=g).to(tr.int32).to(gpu) if ordered else None
    for special in (False, True):
        yhat = yhat0.clone()
        if special:
            k = min(n, len(SPECIAL))
            y[:k] = 0
            yhat[:k] = tr.tensor(SPECIAL[:k], dtype=F64, device=gpu)
        out = tr.empty(n, dtype=F64, device=gpu)
        part = tr.full((lib.sphrt_loss_partials(n),), float('nan'), dtype=F64, device=gpu)
        _lib.check(lib.sphrt_robust_residual_f64(
            _lib.ptr(yhat), _lib.ptr(y), int(ydt == F64), n, code, dl, _lib.ptr(s), _lib.ptr(w),
            _lib.ptr(order), _lib.ptr(out), _lib.ptr(part), _lib.stream_of(gpu)), 'robust_residual')
        sel = order.long() if ordered else slice(None)
        f = yhat.clone().requires_grad_()
        y64 = y.to(F64)
        r = (f.detach() - y64)[sel]
        assert _same_bits_or_nan(out, _psi_t(kind, r, delta) * s[sel])
        if kind == 'abs':
            elem = (y64 - f).abs()
        else:
            elem = F.huber_loss(f, y64, reduction='none', delta=delta)
        (s * elem).sum().backward()
        auto = f.grad[sel]
        assert bool(((out == auto) | (out.isnan() & auto.isnan())).all())
        want = float((w * elem.detach())[sel].sum())
        got = float(part.sum())
        if special and n > 2:
            assert not math.isfinite(want) and not math.isfinite(got)
            assert math.isnan(want) == math.isnan(got)
        else:
            assert abs(got - want) <= 1e-13 * abs(want), (got, want)
    if kind == 'abs':       # what the header records: NaN and +-0 residuals have psi = +0
        z = tr.zeros(3, dtype=F64, device=gpu)
        assert tr.equal(tr.sign(tr.tensor([float('nan'), 0.0, -0.0], device=gpu, dtype=F64))
                        .view(tr.int64), z.view(tr.int64))


# ---- 6. gd on a stored Operator ------------------------------------------------------------------
def _fidelity(kind, **kw):
    from sph_raytracer_amd.loss import AbsLoss, HuberLoss
    return AbsLoss(**kw) if kind == 'abs' else HuberLoss(delta=0.4, **kw)


def _run_gd(op, meas, grid, fid, lam_neg, n_it=25):
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.loss import NegRegularizer
    from sph_raytracer_amd.model import FullyDenseModel
    fns = [fid] + ([lam_neg * NegRegularizer()] if lam_neg else [])
    c, yh, hist = retrieval.gd(op, meas.clone(), FullyDenseModel(grid), lr=1e-1,
                               num_iterations=n_it, loss_fns=fns, progress_bar=False)
    return c.detach().clone(), yh.detach().clone(), [list(hist[fn]) for fn in fns]


@pytest.mark.parametrize('lam, lam_neg, meas_dtype', [(1, None, F64), (0.5, 2, F64), (1, 1, F32)])
@pytest.mark.parametrize('mask', ['unit', 'zero_one', 'float32', 'broadcast'])
@pytest.mark.parametrize('kind', KINDS)
def test_gd_direct_robust_matches_autograd(kind, mask, lam, lam_neg, meas_dtype, gpu, monkeypatch,
                                           circ16):  # noqa: F811
    """gd() with an AbsLoss or a HuberLoss (+ NegRegularizer) over a stored Operator takes
    `_gd_direct` and gives the autograd loop's coefficients and reconstruction bitwise, its loss
    histories within 1e-13 relative — with the measurements permuted into trace order and, with
    that declined, through the kernel's `order` argument."""
    from sph_raytracer_amd import Operator, retrieval
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom, op, meas64 = circ16
    meas = meas64.to(meas_dtype)
    pm = 1 if mask == 'unit' else _mask(mask, meas.shape, gpu)

    def fid():
        return lam * _fidelity(kind, projection_mask=pm)

    c0 = tr.ones(grid.shape, dtype=F64, device=gpu)
    f0 = fid()
    assert retrieval._direct_plan(op, meas, FullyDenseModel(grid), c0, [f0], [c0]) == (f0, None)
    calls = []
    direct = retrieval._gd_direct
    monkeypatch.setattr(retrieval, '_gd_direct', lambda *a, **k: calls.append(1) or direct(*a, **k))
    ca, ya, ha = _run_gd(op, meas, grid, fid(), lam_neg)
    assert len(calls) == 1
    with monkeypatch.context() as mp:
        mp.setattr(retrieval, '_direct_plan', lambda *a: None)
        cb, yb, hb = _run_gd(op, meas, grid, fid(), lam_neg)
    assert len(calls) == 1
    assert len(ha) == len(hb) == (2 if lam_neg else 1) and len(ha[0]) == 25
    assert ha[0][-1] < ha[0][0]
    for la, lb in zip(ha, hb):
        assert np.allclose(la, lb, rtol=1e-13, atol=0), (la, lb)
    assert tr.equal(ca, cb) and tr.equal(ya, yb)
    # the kernel's `order` branch: the trace-position forward declined
    assert op._adjoint_trace_order() is not None
    monkeypatch.setattr(Operator, '_trace_position_rows', lambda self, sd: None)
    cc, yc, hc = _run_gd(op, meas, grid, fid(), lam_neg)
    assert len(calls) == 2
    for lc_, lb in zip(hc, hb):
        assert np.allclose(lc_, lb, rtol=1e-13, atol=0), (lc_, lb)
    assert tr.equal(cc, cb) and tr.equal(yc, yb)


# ---- 7. gd on a MatrixFreeOperator ---------------------------------------------------------------
def _recording(kind, log, **kw):
    """A subclass of the loss that records y - f(d) and f(d): by itself it takes the autograd
    loop, since the plans match exact types."""
    from sph_raytracer_amd.loss import AbsLoss, HuberLoss
    base = AbsLoss if kind == 'abs' else HuberLoss

    class Recording(base):
        def compute(self, f, y, d, c):
            with tr.no_grad():
                fd = f(d)
                log.append(((y - fd).detach(), fd.detach()))
            return super().compute(f, y, d, c)

    return Recording(delta=0.4, **kw) if kind == 'huber' else Recording(**kw)


GD_START_SEED = 274     # (see test_gd_robust_takes_the_fused_loop)


@pytest.mark.parametrize('with_neg', [True, False], ids=['neg', 'alone'])
@pytest.mark.parametrize('mask', ['unit', 'zero_one'])
@pytest.mark.parametrize('kind', KINDS)
def test_gd_robust_takes_the_fused_loop(kind, mask, with_neg, gpu, monkeypatch):
    """gd() over a MatrixFreeOperator with a robust term, with a NegRegularizer and alone:
    _fused_plan accepts ((fid, neg) or (fid, None)); one _robust_into per iteration, one forward
    after the loop, no adjoint; with deterministic=True two runs give equal bits, and the scale
    record is formed by the first iteration only; coefficients and reconstruction within 1e-9 of
    the autograd loop over the same operator (ABS: 10 iterations, every non-zero residual of the
    autograd run outside the margin at every iteration; an exact zero is a ray that misses the
    grid — f(d) exactly 0 — with y = 0, in both loops).  The start is 0.5 + rand (GD_START_SEED,
    chosen with the oracle-backed CPU operator so that the margin holds several times over in
    all four ABS cases): from all ones the rays through the phantom's unit quadrants alone start
    with residuals of a rounding error or zero."""
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.loss import NegRegularizer
    case, op, meas, model, _, _ = _gd_circ16(gpu)
    n_it = 10 if kind == 'abs' else int(case['iterations'])
    pm = 1 if mask == 'unit' else _mask(mask, meas.shape, gpu)
    c0 = 0.5 + _rand(model.coeffs_shape, F64, GD_START_SEED, gpu)

    def run(fid):
        neg = NegRegularizer() if with_neg else None
        fns = [fid, neg] if with_neg else [fid]
        c, y_res, losses = retrieval.gd(op, meas.clone(), model, coeffs=c0.clone(), lr=0.1,
                                        num_iterations=n_it, loss_fns=fns, progress_bar=False)
        assert list(losses) == fns
        return (c.detach().clone(), y_res.detach().clone(), list(losses[fid]),
                list(losses[neg]) if with_neg else [])

    fid = _fidelity(kind, projection_mask=pm)
    neg = NegRegularizer() if with_neg else None
    fns0 = [fid, neg] if with_neg else [fid]
    assert retrieval._direct_plan(op, meas, model, c0, fns0, [c0]) is None
    assert retrieval._fused_plan(op, meas, model, c0, fns0, [c0]) == (fid, neg)
    calls = {'forward': [], 'adjoint': 0, 'robust': 0, 'scaled': 0}
    fwd, adj, robust = op._apply_forward, op._apply_adjoint, op._robust_into

    def forward(density):
        calls['forward'].append(fwd(density))
        return calls['forward'][-1]

    def adjoint(*a, **k):
        calls['adjoint'] += 1
        return adj(*a, **k)

    def robust_into(*a, **k):
        calls['robust'] += 1
        calls['scaled'] += bool(k.get('scaled'))
        return robust(*a, **k)

    monkeypatch.setattr(op, '_apply_forward', forward)
    monkeypatch.setattr(op, '_apply_adjoint', adjoint)
    monkeypatch.setattr(op, '_robust_into', robust_into)
    fused = run(fid)
    assert len(calls['forward']) == 1 and calls['adjoint'] == 0 and calls['robust'] == n_it
    assert calls['scaled'] == 0                          # (float64 atomics: no record)
    assert tr.equal(fused[1], calls['forward'][0].detach())
    op.deterministic = True
    det = [run(_fidelity(kind, projection_mask=pm)) for _ in range(2)]
    op.deterministic = False
    assert calls['robust'] == 3 * n_it and calls['adjoint'] == 0
    assert calls['scaled'] == 2 * (n_it - 1)             # (the record: once per loop)
    assert tr.equal(det[0][0], det[1][0]) and tr.equal(det[0][1], det[1][1])
    assert _bits(det[0][2]) == _bits(det[1][2]) and _bits(det[0][3]) == _bits(det[1][3])
    # the autograd loop of the same problem: the recording subclass takes it by itself
    log = []
    rec = _recording(kind, log, projection_mask=pm)
    assert retrieval._fused_plan(op, meas, model, c0, [rec, neg] if with_neg else [rec],
                                 [c0]) is None
    auto = run(rec)
    assert calls['robust'] == 3 * n_it and calls['adjoint'] == n_it and len(log) == n_it
    if kind == 'abs':
        for res, fd in log:
            zero = res == 0
            assert bool((meas[zero] == 0).all()) and bool((fd[zero] == 0).all())
            assert float(res[~zero].abs().min()) > MARGIN * float(fd.abs().max())
    for what, got in (('fused', fused), ('deterministic', det[0])):
        e_l = float((np.abs(np.array(got[2]) - np.array(auto[2])) / np.array(auto[2])).max())
        e_neg = float(np.abs(np.array(got[3]) - np.array(auto[3])).max()) if with_neg else 0.0
        e_c = float((got[0] - auto[0]).abs().max())
        e_y = gc.rel_close(got[1].cpu().numpy(), auto[1].cpu().numpy(), 1e-9)
        print(f'robust gd_circ16 ({kind}, {mask}, neg {with_neg}), {what} loop against autograd: loss rel '
              f'{e_l:.3g}, loss_neg abs {e_neg:.3g}, coeffs abs {e_c:.3g}, y_result rel {e_y:.3g}')
        assert e_l <= 1e-9 and e_neg <= 1e-12 and e_c <= 1e-9 and e_y <= 1e-9


# ---- 8. what keeps declining ---------------------------------------------------------------------
def test_loop_terms_decline(gpu, circ16):  # noqa: F811
    """One fidelity term of exactly SquareLoss, AbsLoss or HuberLoss; a dynamic operator, a
    volume_mask, two fidelity terms or a subclass return None; distributed.gd's pre-filter sends
    a robust loss to the autograd loop."""
    from sph_raytracer_amd import MatrixFreeOperator, SphericalGrid, retrieval
    from sph_raytracer_amd.distributed import _declined
    from sph_raytracer_amd.loss import AbsLoss, HuberLoss, NegRegularizer, SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom, op, meas = circ16
    model = FullyDenseModel(grid)
    c = tr.ones(grid.shape, dtype=F64, device=gpu)
    mfo = MatrixFreeOperator(grid, geom, device=gpu)
    good = _mask('zero_one', meas.shape, gpu)
    ones = tr.ones(grid.shape, dtype=F64, device=gpu)

    def plans(fns):
        return (retrieval._direct_plan(op, meas, model, c, fns, [c]),
                retrieval._fused_plan(mfo, meas, model, c, fns, [c]),
                retrieval._loop_terms(op, meas, model, c, fns, [c]))

    for make in (AbsLoss, lambda **kw: HuberLoss(delta=0.3, **kw)):
        for kw in ({}, dict(projection_mask=good), dict(projection_mask=good.bool()),
                   dict(projection_mask=good[0].float())):
            fid, neg = 0.5 * make(**kw), NegRegularizer()
            assert plans([fid, neg]) == ((fid, neg),) * 3
            assert plans([neg, fid]) == ((fid, neg),) * 3
            assert plans([fid]) == ((fid, None),) * 3
        assert plans([make(volume_mask=ones)]) == (None,) * 3
        assert plans([make(projection_mask=good, volume_mask=ones)]) == (None,) * 3
        assert plans([make(projection_mask=good.cpu())]) == (None,) * 3
        assert plans([make(projection_mask=2)]) == (None,) * 3
        assert plans([make(), SquareLoss()]) == (None,) * 3
        assert plans([make(), make()]) == (None,) * 3
        assert plans([make(use_grad=False)]) == (None,) * 3
    assert plans([AbsLoss(), HuberLoss()]) == (None,) * 3

    class MyAbs(AbsLoss):
        pass

    class MyHuber(HuberLoss):
        pass

    assert plans([MyAbs()]) == (None,) * 3 and plans([MyHuber(delta=0.3)]) == (None,) * 3
    # a dynamic operator
    dgrid = SphericalGrid(shape=DGRID)
    sgeom = _static_geom('S1')
    dop = MatrixFreeOperator(dgrid, sgeom, device=gpu)
    dc = tr.ones(DGRID, dtype=F64, device=gpu)
    y = _rand(sgeom.shape, F64, 262, gpu)
    for fid in (AbsLoss(), HuberLoss(delta=0.3)):
        assert retrieval._fused_plan(dop, y, FullyDenseModel(dgrid), dc, [fid], [dc]) is None
        assert _declined([fid]) and _declined([NegRegularizer(), fid])
    assert not _declined([SquareLoss(), NegRegularizer()])
