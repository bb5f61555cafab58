"""The gd matrix's cases on the CPU reference alone (tests/gd_cases.py): the covering array covers
every pair of factor levels; each case's inputs exercise what its factors name (no case passes
vacuously); three cases' reference iterates are reproduced bit for bit by a hand-written loop of
plain float64 torch without autograd, the gradients written out from `_gd_direct`'s docstring; and
the committed sensitivity table, from which the GPU bounds come, is recomputed.  No GPU."""
import itertools

import numpy as np
import pytest
import torch as tr

import gd_cases as gc

F64 = tr.float64

# pairs of levels left out on purpose: ((factor, level), (factor, level), reason); at most 5 %
EXCLUDED = []


# ---- 1. coverage ---------------------------------------------------------------------------------
def test_every_pair_of_levels_is_covered():
    names = list(gc.FACTORS)
    pairs = [((fa, a), (fb, b)) for fa, fb in itertools.combinations(names, 2)
             for a in gc.FACTORS[fa] for b in gc.FACTORS[fb]]
    assert len(pairs) == 10 * 16 + 5 * 8
    assert len(EXCLUDED) <= 0.05 * len(pairs)
    left_out = {(p, q) for p, q, _ in EXCLUDED}
    assert left_out <= set(pairs)
    seen = {((fa, getattr(c, fa)), (fb, getattr(c, fb))) for c in gc.CASES
            for fa, fb in itertools.combinations(names, 2)}
    missing = [p for p in pairs if p not in seen and p not in left_out]
    assert not missing, missing
    assert 20 <= len(gc.CASES) <= 30 and len(set(gc.NAMES)) == len(gc.CASES)
    for c in gc.CASES:
        assert all(getattr(c, f) in levels for f, levels in gc.FACTORS.items())
        assert (c.smooth is not None) == (c.R in ('smooth', 'both'))
    smooth = [c for c in gc.CASES if c.smooth]
    assert {c.smooth for c in smooth} >= {'square', 'abs'}        # quadratic and not
    assert {c.wrap for c in smooth} == {None, False}              # the ring closed and open
    assert {c.why for c in gc.DECLINED} == {'neg_fid_smooth', 'smooth_neg_fid', 'volume_mask',
                                            'tensor_lam'}


def test_geometries():
    """circ16 is view-tiled, rect7 is not; rect7's sizes span two workgroups of the loss kernels
    and are no multiple of their 256 threads; the full rings close (wrap_a=None: closed)."""
    from sph_raytracer_amd import raytracer as rt
    from sph_raytracer_amd.loss import SmoothRegularizer
    shapes = {name: tuple(gc.cpu_operator(name).ray_shape) for name in ('circ16', 'rect7')}
    assert rt._view_tiles(shapes['circ16'], False) is not None
    assert rt._view_tiles(shapes['rect7'], False) is None
    grid, _ = gc.geometry('rect7')
    for n in (int(np.prod(shapes['rect7'])), int(np.prod(grid.shape))):
        assert 256 < n <= 512 and n % 256
    for c in gc.CASES:
        assert c.geometry == {'stored_reordered': 'circ16', 'stored_in_order': 'rect7'}.get(
            c.O, c.geometry)
    assert {c.geometry for c in gc.CASES if c.O.startswith('mf')} == {'circ16', 'rect7'}
    for name in shapes:
        assert SmoothRegularizer().wraps(gc.cpu_operator(name))


# ---- 2. the inputs hold what the factors name ----------------------------------------------------
class _Recorder:
    """The operator, keeping (density, forward) of every call."""

    def __init__(self, op):
        self.op, self.grid, self.device, self.log = op, op.grid, op.device, []

    def __call__(self, d):
        p = self.op(d)
        self.log.append((d.detach().clone(), p.detach().clone()))
        return p


@pytest.mark.parametrize('name', gc.NAMES + gc.DECLINED_NAMES)
def test_reference_inputs(name):
    case = gc.BY_NAME[name]
    rec = _Recorder(gc.cpu_operator(case.geometry))
    res, (y, mask, c0), (fid, neg, smooth) = gc.run_gd(rec, case, gc.inputs(case))
    its = rec.log[:gc.N_IT]                     # (the last call is the returned forward)
    assert len(rec.log) == gc.N_IT + 1
    ref = gc.reference(name)
    assert np.array_equal(res.c, ref.c) and res.hist == ref.hist     # the run is reproducible
    assert y.dtype == (F64 if case.Y == 'f64' else tr.float32)
    yd = y.detach().to(F64)
    w = mask.to(F64).expand(y.shape) if isinstance(mask, tr.Tensor) else tr.ones_like(yd)
    for h in res.hist:
        assert len(h) == gc.N_IT and np.isfinite(h).all()
    assert np.isfinite(res.c).all() and np.isfinite(res.y).all()
    k_fid = 0 if not isinstance(case, gc.Declined) else \
        {'neg_fid_smooth': 1, 'smooth_neg_fid': 2}.get(case.why, 0)
    assert res.hist[k_fid][-1] < res.hist[k_fid][0]
    if case.F == 'poisson':
        assert all(float((p + gc.POISSON_EPS).min()) > 0 for _, p in its)
        assert float(yd.min()) >= 0 and bool((yd == yd.round()).all()) and float(yd.max()) >= 2
    if case.F == 'huber':
        for _, p in (its[0], its[-1]):
            beyond = ((p - yd).abs() > gc.HUBER_DELTA) & (w > 0)
            frac = float(beyond.sum()) / float((w > 0).sum())
            assert 0.2 <= frac <= 0.8, frac
    if neg is not None:
        assert max(float((d < 0).to(F64).mean()) for d, _ in its) >= 0.05
    if case.M != 'unit':
        assert mask.dtype == {'bool': tr.bool, 'f32_views': tr.float32, 'f64_full': F64}[case.M]
        assert mask.dim() == (2 if case.M == 'f32_views' else 3)
        assert 0.10 <= float((w < 1).to(F64).mean()) <= 0.50
    else:
        assert mask == 1
    if smooth is not None:
        k = [fn for fn in (fid, neg, smooth) if fn is not None].index(smooth)
        if not isinstance(case, gc.Declined):
            assert all(v > 0 for v in res.hist[k])


# ---- 3. the reference restated -------------------------------------------------------------------
def _adam(c, g, st, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam's single-tensor step (what it runs for a CPU tensor)."""
    b1, b2 = betas
    st['t'] += 1
    if weight_decay:
        g = g.add(c, alpha=weight_decay)
    st['m'].lerp_(g, 1 - b1)
    st['v'].mul_(b2).addcmul_(g, g, value=1 - b2)
    step_size = lr / (1 - b1 ** st['t'])
    bc2_sqrt = (1 - b2 ** st['t']) ** 0.5
    c.addcdiv_(st['m'], (st['v'].sqrt() / bc2_sqrt).add_(eps), value=-step_size)


def _sgd(c, g, st, lr, momentum):
    if 'buf' not in st:
        st['buf'] = g.clone()
    else:
        st['buf'].mul_(momentum).add_(g)
    c.add_(st['buf'], alpha=-lr)


def _smooth_huber_gradient(d, delta, scale):
    """Gradient of scale * sum over the three axes (the azimuth ring closed) of huber(d[i+1] -
    d[i]): clamp(difference, +-delta) * scale at the upper voxel, its negative at the lower,
    summed as autograd sums them (the last axis first, and there the rolled side first)."""
    terms = []
    for dim in (0, 1):
        n = d.shape[dim]
        psi = (d.narrow(dim, 1, n - 1) - d.narrow(dim, 0, n - 1)).clamp(-delta, delta) * scale
        hi, lo = tr.zeros_like(d), tr.zeros_like(d)
        hi.narrow(dim, 1, n - 1).copy_(psi)
        lo.narrow(dim, 0, n - 1).copy_(-psi)
        terms += [hi, lo]
    psi = (tr.roll(d, -1, -1) - d).clamp(-delta, delta) * scale
    terms += [tr.roll(psi, 1, -1), -psi]
    r_hi, r_lo, e_hi, e_lo, a_hi, a_lo = terms
    return ((((a_hi + a_lo) + e_lo) + e_hi) + r_lo) + r_hi


def _restated(name):
    """N_IT iterations of the case by hand -> the coefficients.  A is applied by the reference's
    own matrix products (CpuOperator._fwd / ._adj on plain tensors: no autograd Function)."""
    case = gc.BY_NAME[name]
    inp, op = gc.inputs(case), gc.cpu_operator(case.geometry)
    y, c = inp.y.to(F64), inp.c0.clone()
    n, v = y.numel(), c.numel()
    w = inp.mask.to(F64).expand(y.shape) if isinstance(inp.mask, tr.Tensor) else None
    _, kw = gc.optimiser(case)
    st = {'t': 0, 'm': tr.zeros_like(c), 'v': tr.zeros_like(c)}
    for _ in range(gc.N_IT):
        p = op._fwd(c)
        if case.F == 'square':          # (f(d) - y) * (2 * (lam / N))
            r = (p - y) * (2 * (gc.LAM_FID / n))
        elif case.F == 'huber':         # s * clamp(f(d) - y, -delta, delta), s = (lam / N) * w
            r = ((gc.LAM_FID / n) * w) * (p - y).clamp(-gc.HUBER_DELTA, gc.HUBER_DELTA)
        else:                           # s + ((-s) * y) / (p + eps)
            s = (gc.LAM_FID / n) * w
            r = s + ((-s) * y) / (p + gc.POISSON_EPS)
        g = op._adj(r, tuple(c.shape))
        if case.R == 'both':            # (g_smooth + g_neg) + g_fid
            g_neg = (c < 0).to(F64) * -(gc.LAM_NEG / v)
            g_smooth = _smooth_huber_gradient(c, gc.SMOOTH_DELTA, gc.LAM_SMOOTH / v)
            g = (g_smooth + g_neg) + g
        if case.P == 'sgd':
            _sgd(c, g, st, kw['lr'], kw['momentum'])
        else:
            _adam(c, g, st, **{k: x for k, x in kw.items() if k != 'fused'})
    return c.numpy()


RESTATED = ['21-square-unit-f64-fid-stored_reordered-sgd',
            '22-huber-f32_views-f32-fid-mf_deterministic-adam_wd',
            '18-poisson-bool-f32-both-stored_in_order-adam']


@pytest.mark.parametrize('name', RESTATED)
def test_reference_restated_by_hand(name):
    case = gc.BY_NAME[name]
    assert (case.F, case.M, case.R) in [('square', 'unit', 'fid'), ('huber', 'f32_views', 'fid'),
                                        ('poisson', 'bool', 'both')]
    if case.R == 'both':
        assert case.smooth == 'huber' and case.wrap is None
    got, ref = _restated(name), gc.reference(name)
    assert not np.array_equal(ref.c, gc.inputs(case).c0.numpy())
    assert np.array_equal(got.view(np.int64), ref.c.view(np.int64)), np.abs(got - ref.c).max()


# ---- 4. the sensitivity table --------------------------------------------------------------------
def _within_two(got, want):
    return got <= 2 * want and want <= 2 * got


@pytest.mark.parametrize('name', gc.NAMES + gc.DECLINED_NAMES)
def test_sensitivity_table(name):
    """The committed d_case is what the reversed-order run gives, to a factor of two, and no case
    is ill-conditioned: d of the coefficients at most 1e-6 of their largest magnitude."""
    d_c, d_y, d_h = gc.sensitivity(name)
    t_c, t_y, t_h = gc.D_CASE[name]
    ref = gc.reference(name)
    print(f'{name}: d_c {d_c:.3e} (table {t_c:.3e}), d_y {d_y:.3e} ({t_y:.3e}), hist {d_h} ({t_h})')
    assert _within_two(d_c, t_c) and _within_two(d_y, t_y)
    assert len(d_h) == len(t_h) == len(ref.hist)
    assert all(_within_two(a, b) for a, b in zip(d_h, t_h))
    assert d_c <= gc.ILL * float(np.abs(ref.c).max())
    b_c, b_y, b_h = gc.bounds(name)
    assert b_c >= gc.FLOOR * float(np.abs(ref.c).max()) and b_c <= 16 * gc.ILL * np.abs(ref.c).max()
    assert b_c == max(16 * t_c, 1e-13 * float(np.abs(ref.c).max()))


def test_reversed_matrix_is_the_same_matrix():
    """The perturbed operator holds the same triplets, last to first."""
    for name in ('circ16', 'rect7'):
        a, b = gc.cpu_operator(name), gc.cpu_operator(name, True)
        for u, v in ((a.ray, b.ray), (a.vox, b.vox), (a.seg, b.seg)):
            assert np.array_equal(u, v[::-1])
        x = tr.rand(tuple(a.grid.shape), dtype=F64, generator=tr.Generator().manual_seed(1))
        pa, pb = a._fwd(x), b._fwd(x)
        assert not tr.equal(pa, pb) and float((pa - pb).abs().max()) <= 1e-14 * float(pa.max())
