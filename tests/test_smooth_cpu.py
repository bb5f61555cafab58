"""Host side of the smoothness regulariser (sphrt_smooth_reg_f64, loss.SmoothRegularizer,
retrieval._loop_terms with a smooth term): the entry is declared, exported and bound; its
refusals fire on the host; the constructor refuses bad arguments; the plain-torch formula equals
a hand-written one on a 2x3x4 volume; the azimuth wrap is inferred from the grid; _loop_terms
accepts and declines what the direct loops can and cannot run (over stand-ins for the operator
and the coefficients: it only reads their attributes, and there is no GPU here); and the order
in which autograd accumulates three terms at a shared leaf, which the direct loop's gradient sum
restates, is pinned.  (No compute call of the library.)"""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, N_ARGS = 'sphrt_smooth_reg_f64', 21
SQUARE, ABS, HUBER = 0, 1, 2
F64 = tr.float64


def test_entry_declared_exported_and_bound():
    from sph_raytracer_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, 'include', 'sphrt.h')).read()
    m = re.search(r'int\s+' + ENTRY + r'\s*\(([^;]*)\)\s*;', hdr)
    assert m, f'{ENTRY} is not declared in include/sphrt.h'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == N_ARGS
    assert args[0] == 'const double *d' and args[1] == 'int64_t n_batch' and args[-1] == 'void *stream'
    assert re.search(r'int kind,\s*double delta,\s*int wrap_a,\s*double inv_n,\s*double lam,'
                     r'\s*double c_neg', m.group(1))
    assert ENTRY in _lib.EXPORTED and hasattr(ctypes.CDLL(_lib.LIB_PATH), ENTRY)
    fn = getattr(_lib.load(), ENTRY)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == N_ARGS
    by_value = [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_double] * 4 + \
        [ctypes.c_int, ctypes.c_double, ctypes.c_int] + [ctypes.c_double] * 3
    assert list(fn.argtypes) == [ctypes.c_void_p] + by_value + [ctypes.c_void_p] * 5
    # the loop's other entries keep their signatures
    assert len(_lib.load().sphrt_neg_reg_f64.argtypes) == 6
    assert len(_lib.load().sphrt_adam_foreach_neg_f64.argtypes) == 15


def test_refusals_on_the_host():
    """Every refusal returns non-zero with its word in sphrt_last_error before any launch: the
    pointers are never dereferenced."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, ENTRY)
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    inf, nan = float('inf'), float('nan')

    def call(d=p, n_batch=1, nt=1, nr=4, ne=5, na=6, wt=0.0, wr=1.0, we=1.0, wa=1.0, kind=SQUARE,
             delta=0.0, wrap=1, inv_n=1 / 120, lam=1.0, c_neg=0.0, g_in=None, g_out=q,
             part_smooth=p, part_neg=None):
        return fn(d, n_batch, nt, nr, ne, na, wt, wr, we, wa, kind, delta, wrap, inv_n, lam, c_neg,
                  g_in, g_out, part_smooth, part_neg, None)

    cases = [(dict(n_batch=0), b'empty volume'), (dict(n_batch=-3), b'empty volume')]
    for ax in ('nt', 'nr', 'ne', 'na'):
        cases += [({ax: 0}, b'axis lengths'), ({ax: -1}, b'axis lengths')]
    cases += [
        (dict(n_batch=2 ** 31), b'2^31'),
        (dict(n_batch=2 ** 62, nt=4, nr=4), b'2^31'),
        (dict(n_batch=2 ** 20, nr=2 ** 11), b'2^31'),                 # exactly 2^31 voxels
        (dict(nt=2 ** 16, nr=2 ** 16, ne=2 ** 16, na=2 ** 16), b'2^31'),
        (dict(n_batch=2 ** 40, nt=2 ** 30, nr=2 ** 30, ne=2 ** 30, na=2 ** 30), b'2^31'),
    ]
    for w in ('wt', 'wr', 'we', 'wa'):
        cases += [({w: bad}, b'weights') for bad in (-1.0, -1e-300, inf, -inf, nan)]
    cases += [({k: bad}, b'inv_n and lam') for k in ('inv_n', 'lam') for bad in (inf, -inf, nan)]
    cases += [(dict(kind=k, delta=0.5), b'unknown residual kind') for k in (3, -1, 7)]
    cases += [(dict(kind=HUBER, delta=bad), b'delta') for bad in (0.0, -1.0, inf, -inf, nan)]
    cases += [(dict(part_smooth=None), b'null part_smooth'), (dict(g_out=None), b'null g_out'),
              (dict(d=None), b'null density'), (dict(g_out=p), b'same buffer')]
    for i, (kw, word) in enumerate(cases):
        for base in (dict(), dict(kind=ABS), dict(kind=HUBER, delta=0.5),
                     dict(g_in=q, part_neg=p, c_neg=0.1)):
            assert call(**{**base, **kw}) != 0, (i, kw, base)
            assert word in lib.sphrt_last_error(), (i, kw, base, lib.sphrt_last_error())


def test_constructor_refusals():
    from sph_raytracer_amd.loss import Loss, SmoothRegularizer
    s = SmoothRegularizer()
    assert isinstance(s, Loss) and s.kind == 'regularizer' and type(s).kind == 'regularizer'
    assert s.weights == (1.0, 1.0, 1.0) and s.time_weight == 0.0 and s.wrap_a is None
    assert s.delta is None and s.lam == 1 and s.use_grad
    s = 0.5 * SmoothRegularizer(weights=[2, np.float32(0.5), 0], time_weight=np.int64(3),
                                kind='huber', delta=2, wrap_a=False, volume_mask=2)
    assert s.weights == (2.0, 0.5, 0.0) and s.time_weight == 3.0 and s.delta == 2.0
    assert type(s.delta) is float and s.lam == 0.5 and s.volume_mask == 2 and s.wrap_a is False
    inf, nan = float('inf'), float('nan')
    for bad in ((1, 1), (1, 1, 1, 1), 1.0, None, (1, -1, 1), (1, 1, inf), (nan, 1, 1),
                (True, 1, 1), ('1', 1, 1), (1, tr.tensor(1.0), 1), tr.ones(3), (None, 1, 1)):
        with pytest.raises(ValueError, match='three weights'):
            SmoothRegularizer(weights=bad)
    for bad in (-1, inf, nan, None, True, '0', tr.tensor(0.5)):
        with pytest.raises(ValueError, match='time_weight'):
            SmoothRegularizer(time_weight=bad)
    for bad in ('l1', 'Square', '', None, 1, ['abs']):
        with pytest.raises(ValueError, match="'square', 'abs' or 'huber'"):
            SmoothRegularizer(kind=bad)
    for bad in (None, 0, 0.0, -0.5, inf, nan, True, '1', tr.tensor(0.5)):
        with pytest.raises(ValueError, match='finite delta > 0'):
            SmoothRegularizer(kind='huber', delta=bad)
    for kind in ('square', 'abs'):
        with pytest.raises(ValueError, match="delta belongs to kind='huber'"):
            SmoothRegularizer(kind=kind, delta=0.5)
    for bad in (0, 1, 'yes', tr.tensor(True)):
        with pytest.raises(ValueError, match='wrap_a'):
            SmoothRegularizer(wrap_a=bad)
    with pytest.raises(ValueError, match='axes'):
        SmoothRegularizer()(None, None, tr.ones(3, 4, dtype=F64), None)


def _rho(r, kind, delta):
    if kind == 'square':
        return r * r
    if kind == 'abs':
        return abs(r)
    return 0.5 * r * r if abs(r) < delta else delta * (abs(r) - 0.5 * delta)


def _psi(r, kind, delta):
    if kind == 'square':
        return 2 * r
    if kind == 'abs':
        return float(np.sign(r))
    return min(max(r, -delta), delta)


def _by_hand(d, w, kind, delta, wrap):
    """P and dP/dd by loops over the edges of a (nr, ne, na) numpy volume."""
    shape, val, grad = d.shape, 0.0, np.zeros(d.shape)
    for idx in np.ndindex(*shape):
        for ax in range(3):
            up = list(idx)
            up[ax] += 1
            if up[ax] == shape[ax]:
                if not (ax == 2 and wrap and shape[ax] > 1):
                    continue
                up[ax] = 0
            up = tuple(up)
            r = d[up] - d[idx]
            val += w[ax] * _rho(r, kind, delta)
            grad[up] += w[ax] * _psi(r, kind, delta)
            grad[idx] -= w[ax] * _psi(r, kind, delta)
    return val / d.size, grad / d.size


@pytest.mark.parametrize('wrap', [False, True], ids=['open', 'wrap'])
@pytest.mark.parametrize('kind', ['square', 'abs', 'huber'])
def test_formula_by_hand(kind, wrap):
    from sph_raytracer_amd.loss import SmoothRegularizer
    delta = 0.6 if kind == 'huber' else None
    w = (0.5, 2.0, 1.25)
    g = tr.Generator().manual_seed(3)
    d = tr.randn(2, 3, 4, dtype=F64, generator=g)
    if kind == 'huber':
        diffs = np.abs(np.diff(d.numpy(), axis=1))
        assert (diffs < delta).any() and (diffs > delta).any()          # both branches
    fn = 3.0 * SmoothRegularizer(weights=w, kind=kind, delta=delta, wrap_a=wrap)
    dd = d.clone().requires_grad_()
    val = fn(None, None, dd, None)
    val.backward()
    want, gwant = _by_hand(d.numpy(), w, kind, delta, wrap)
    assert abs(float(val.detach()) - 3.0 * want) <= 1e-14 * abs(3.0 * want)
    assert np.abs(dd.grad.numpy() - 3.0 * gwant).max() <= 1e-14 * np.abs(3.0 * gwant).max()
    # a volume_mask multiplies d first; float32 stays float32; a non-contiguous view is taken as is
    m = tr.rand(2, 3, 4, dtype=F64, generator=g)
    masked = SmoothRegularizer(weights=w, kind=kind, delta=delta, wrap_a=wrap, volume_mask=m)
    assert abs(float(masked(None, None, d, None)) - _by_hand((m * d).numpy(), w, kind, delta, wrap)[0]) \
        <= 1e-14
    assert fn(None, None, d.float(), None).dtype == tr.float32
    dt = d.permute(0, 2, 1)
    want_t = _by_hand(np.ascontiguousarray(dt.numpy()), w, kind, delta, wrap)[0]
    assert abs(float(fn(None, None, dt, None)) - 3.0 * want_t) <= 1e-14
    # a constant volume: P = 0 and G = 0 exactly
    c = tr.full((2, 3, 4), 0.3, dtype=F64, requires_grad=True)
    v = fn(None, None, c, None)
    v.backward()
    assert float(v.detach()) == 0.0 and bool((c.grad == 0).all())
    # the time axis and the batch axes: (2, 2, 3, 4) with time_weight is the two volumes' edges
    # plus the edges between them; without it the leading axis is batch
    d4 = tr.randn(2, 2, 3, 4, dtype=F64, generator=g)
    plain = SmoothRegularizer(weights=w, kind=kind, delta=delta, wrap_a=wrap)
    timed = SmoothRegularizer(weights=w, time_weight=0.75, kind=kind, delta=delta, wrap_a=wrap)
    within = sum(_by_hand(d4[i].numpy(), w, kind, delta, wrap)[0] for i in range(2)) / 2
    across = 0.75 * sum(_rho(float(r), kind, delta) for r in (d4[1] - d4[0]).reshape(-1)) / 48
    assert abs(float(plain(None, None, d4, None)) - within) <= 1e-14
    assert abs(float(timed(None, None, d4, None)) - (within + across)) <= 1e-14
    d5 = tr.stack([d4, d4 + 1])
    assert abs(float(timed(None, None, d5, None)) - (within + across)) <= 1e-14    # batch: no edges


def test_ramp_and_degenerate_axes():
    from sph_raytracer_amd.loss import SmoothRegularizer
    # a ramp along r under 'square': zero interior gradient, -+2 w_r step / N on the end shells
    nr, ne, na, step, w_r = 5, 3, 4, 0.25, 2.0
    d = (step * tr.arange(nr, dtype=F64))[:, None, None].expand(nr, ne, na).clone().requires_grad_()
    val = SmoothRegularizer(weights=(w_r, 1, 1), wrap_a=True)(None, None, d, None)
    val.backward()
    n = nr * ne * na
    assert float(val.detach()) == w_r * (nr - 1) * ne * na * step ** 2 / n
    assert bool((d.grad[1:-1] == 0).all())
    assert bool((d.grad[0] == -2 * w_r * step / n).all()) and bool((d.grad[-1] == 2 * w_r * step / n).all())
    # n_a = 2 with wrap: the pair is joined by two edges; n_a = 1: no edge, wrap or not
    g = tr.Generator().manual_seed(4)
    d2 = tr.randint(-8, 9, (3, 1, 2), generator=g).to(F64)        # (integers: every sum exact)
    assert bool((d2[..., 0] != d2[..., 1]).any())
    for kind, delta in (('square', None), ('abs', None), ('huber', 0.5)):
        open_, ring = (SmoothRegularizer(weights=(0, 0, 1), kind=kind, delta=delta, wrap_a=wr)
                       for wr in (False, True))
        assert float(ring(None, None, d2, None)) == 2 * float(open_(None, None, d2, None)) > 0
        d1 = tr.randn(5, 3, 1, dtype=F64, generator=g)
        full = [SmoothRegularizer(kind=kind, delta=delta, wrap_a=wr)(None, None, d1, None)
                for wr in (False, True)]
        assert float(full[0]) == float(full[1])
        assert abs(float(full[0]) - _by_hand(d1.numpy(), (1, 1, 1), kind, delta, True)[0]) <= 1e-14
        # a weight of 0 contributes nothing, whatever the axis holds
        bad = d1.clone()
        bad[2, 1, 0] = float('inf')
        off = SmoothRegularizer(weights=(0, 0, 1), kind=kind, delta=delta, wrap_a=True)
        assert float(off(None, None, bad, None)) == 0.0
        assert float(SmoothRegularizer(kind=kind, delta=delta)(None, None, tr.ones(1, 1, 1, dtype=F64),
                                                               None)) == 0.0


def test_wrap_inferred_from_the_grid():
    from sph_raytracer_amd import SphericalGrid
    from sph_raytracer_amd.loss import SmoothRegularizer
    full = types.SimpleNamespace(grid=SphericalGrid(shape=(3, 4, 6)))
    part = types.SimpleNamespace(grid=SphericalGrid(shape=(3, 4, 6), size_a=(-1.0, 2.0)))
    shifted = types.SimpleNamespace(grid=SphericalGrid(shape=(3, 4, 6), size_a=(0.0, 2 * math.pi)))
    near = types.SimpleNamespace(grid=SphericalGrid(
        shape=(3, 4, 6), size_a=(-math.pi, math.pi * (1 - 1e-6))))
    s = SmoothRegularizer()
    assert s.wraps(full) and s.wraps(shifted) and not s.wraps(part) and not s.wraps(near)
    assert not s.wraps(None) and not s.wraps(object())
    assert SmoothRegularizer(wrap_a=False).wraps(full) is False
    assert SmoothRegularizer(wrap_a=True).wraps(part) is True and SmoothRegularizer(wrap_a=True).wraps(None)
    g = tr.Generator().manual_seed(6)
    d = tr.randn(3, 4, 6, dtype=F64, generator=g)
    ring = float(SmoothRegularizer(wrap_a=True)(None, None, d, None))
    open_ = float(SmoothRegularizer(wrap_a=False)(None, None, d, None))
    assert ring != open_
    assert float(s(full, None, d, None)) == ring and float(s(part, None, d, None)) == open_
    assert float(s(None, None, d, None)) == open_


def _loop_setup():
    """Stand-ins `_loop_terms` reads attributes of: an operator and float64 coefficients that
    say they are on a GPU."""
    from sph_raytracer_amd import SphericalGrid
    from sph_raytracer_amd.model import FullyDenseModel
    grid = SphericalGrid(shape=(3, 4, 5))
    dev = tr.device('cpu')
    f = types.SimpleNamespace(grid=grid, _cdev=dev, _ray_shape=(6, 7))
    c = types.SimpleNamespace(dtype=F64, is_cuda=True, device=dev, shape=tuple(grid.shape),
                              is_contiguous=lambda: True)
    return f, tr.zeros(6, 7, dtype=F64), FullyDenseModel(grid), c


def test_loop_terms_with_a_smooth_term():
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.loss import (AbsLoss, HuberLoss, NegRegularizer, SmoothRegularizer,
                                        SquareLoss)
    f, y, model, c = _loop_setup()

    def terms(fns):
        return retrieval._loop_terms(f, y, model, c, fns, [c])

    fid, neg = SquareLoss(), 2 * NegRegularizer()
    assert terms([fid, neg]) == (fid, neg) and terms([neg, fid]) == (fid, neg)   # as before
    assert terms([fid]) == (fid, None)
    for sm in (SmoothRegularizer(), 0.5 * SmoothRegularizer(kind='abs'),
               SmoothRegularizer(kind='huber', delta=0.5, weights=(1, 0, 2), wrap_a=True)):
        for fid in (SquareLoss(), 3 * AbsLoss(), HuberLoss(delta=0.3)):
            assert terms([fid, neg, sm]) == (fid, neg, sm)
            assert terms([fid, sm, neg]) == (fid, neg, sm)
            assert terms([fid, sm]) == (fid, None, sm)
            assert terms([sm, fid]) == (fid, None, sm)
            # three terms: only a leading fidelity term gives g_fid + (g_smooth + g_neg)
            for fns in ([neg, fid, sm], [sm, fid, neg], [neg, sm, fid], [sm, neg, fid]):
                assert terms(fns) is None
    fid, sm = SquareLoss(), SmoothRegularizer()
    assert terms([fid, sm, SmoothRegularizer()]) is None and terms([fid, sm, sm]) is None
    assert terms([sm]) is None and terms([sm, neg]) is None

    class Sub(SmoothRegularizer):
        pass

    assert terms([fid, Sub()]) is None and terms([fid, neg, Sub()]) is None
    assert terms([fid, tr.tensor(0.5) * SmoothRegularizer()]) is None
    assert terms([fid, SmoothRegularizer(volume_mask=tr.ones(3, 4, 5))]) is None
    assert terms([fid, SmoothRegularizer(volume_mask=2)]) is None
    assert terms([fid, SmoothRegularizer(projection_mask=tr.ones(6, 7))]) is None
    assert terms([fid, SmoothRegularizer(use_grad=False)]) is None


def test_distributed_gd_declines_the_smooth_term():
    from sph_raytracer_amd.distributed import _declined
    from sph_raytracer_amd.loss import NegRegularizer, SmoothRegularizer, SquareLoss
    assert not _declined([SquareLoss(), NegRegularizer()])
    assert _declined([SquareLoss(), SmoothRegularizer()])
    assert _declined([SquareLoss(), NegRegularizer(), 0.5 * SmoothRegularizer(kind='abs')])


class _Term(tr.autograd.Function):
    """A term of the total whose gradient at the leaf is a given constant."""

    @staticmethod
    def forward(ctx, x, g):
        ctx.g = g
        return x.sum() * 0

    @staticmethod
    def backward(ctx, grad_out):
        return ctx.g * grad_out, None


@pytest.mark.parametrize('with_lam', [False, True], ids=['plain', 'lam'])
def test_autograd_accumulates_last_plus_middle_plus_first(with_lam):
    """At a leaf shared by the terms [t1, t2, t3] of `total = 0 + t1 + t2 + t3` (gd's loop),
    autograd leaves (g3 + g2) + g1: `_gd_direct` restates that sum as g_fid + (g_smooth + g_neg)
    for a leading fidelity term and `_loop_terms` declines the other orders.  Gradients of very
    different magnitudes make the three groupings round differently.  If a torch upgrade changes
    the order this fails, and with it the bitwise comparison of the three-term direct loop
    against the autograd loop (tests/test_gpu_smooth_reg.py)."""
    gen = tr.Generator().manual_seed(9)
    n = 4096
    g1 = tr.randn(n, dtype=F64, generator=gen)
    g2 = tr.randn(n, dtype=F64, generator=gen) * 1e-3
    g3 = tr.randn(n, dtype=F64, generator=gen) * 1e3
    want = (g3 + g2) + g1
    assert not tr.equal(want, (g1 + g2) + g3) and not tr.equal(want, (g1 + g3) + g2)
    lam = 0.3 if with_lam else 1
    for _ in range(2):
        x = tr.zeros(n, dtype=F64, requires_grad=True)
        total = 0
        for g in (g1, g2, g3):
            val = _Term.apply(x, g / lam if with_lam else g)
            total += lam * val if with_lam else val
        total.backward()
        got = x.grad
        if with_lam:    # (g / lam) * lam need not be g: compare against the same products
            want = ((g3 / lam) * lam + (g2 / lam) * lam) + (g1 / lam) * lam
        assert tr.equal(got, want)
