"""The smoothness regulariser on the GPU: sphrt_smooth_reg_f64 (csrc/loss.hip) against the
plain-torch formula of loss.SmoothRegularizer — bitwise where every sum is exact, to a rounding
bound elsewhere, on degenerate axes, past one element per thread, with ties, with differences of
exactly +-delta and with a NaN voxel; the folded form (g_in, the NegRegularizer's term) against
its parts, bitwise; the autograd Function; and gd()'s direct loops with the term, over a stored
Operator (bitwise the autograd loop) and a MatrixFreeOperator, and the autograd loop on a
dynamic grid with a time weight."""
import math
import types

import numpy as np
import pytest
import torch as tr

from test_gpu_adjoint_paths import DGRID, T_DYN, _orbit, _rand
from test_gpu_matrix_free_deterministic import _bits
from test_gpu_matrix_free_gradient import _gd_circ16
from test_gpu_weighted_gradient import circ16  # noqa: F401

pytestmark = pytest.mark.gpu

F64, F32 = tr.float64, tr.float32
KINDS = [('square', None), ('abs', None), ('huber', 0.5)]
KIND_IDS = [k for k, _ in KINDS]
EPS = 2.0 ** -53


def _reg(kind, delta, **kw):
    from sph_raytracer_amd.loss import SmoothRegularizer
    return SmoothRegularizer(kind=kind, delta=delta, **kw)


def _kernel(reg, d, wrap, lam=1.0, c_neg=0.0, g_in=None, g_out=None, neg=False):
    """One launch of the entry as the loss and gd make it -> (g_out, part_smooth, part_neg), the
    partial buffers pre-filled with NaN (every partial is written)."""
    from sph_raytracer_amd import _lib
    n_part = _lib.load().sphrt_loss_partials(d.numel())
    assert n_part == min(1024, -(-d.numel() // 256))
    part = tr.full((n_part,), float('nan'), dtype=F64, device=d.device)
    part_neg = tr.full((n_part,), float('nan'), dtype=F64, device=d.device) if neg else None
    if g_out is None:
        g_out = tr.full_like(d, float('nan'))
    reg._launch(d, wrap, lam, c_neg, g_in, g_out, part, part_neg)
    return g_out, part, part_neg


def _formula(reg, d, wrap):
    """(value, gradient) of the torch formula on d's device."""
    x = d.detach().clone().requires_grad_()
    val = reg.formula(x, wrap)
    if not val.requires_grad:               # (no axis has an edge: a constant 0)
        return val, tr.zeros_like(d)
    val.backward()
    return val.detach(), x.grad


def _abs_terms(reg, d, wrap):
    """A of the gradient tolerance: the largest per-voxel sum of the absolute terms
    w_ax |rho'(d_i - d_nb)| / N — the reference formula evaluated with |rho'|."""
    tot = tr.zeros_like(d)
    for dim, w in reg._axes(d):
        n = d.shape[dim]
        ring = dim == -1 and wrap
        hi = tr.roll(d, -1, -1) if ring else d.narrow(dim, 1, n - 1)
        lo = d if ring else d.narrow(dim, 0, n - 1)
        r = (hi - lo).abs()
        t = 2 * r if reg.smooth_kind == 'square' else \
            (r != 0).to(F64) if reg.smooth_kind == 'abs' else r.clamp(max=reg.delta)
        t = w * t
        if ring:
            tot += t + tr.roll(t, 1, -1)
        else:
            tot.narrow(dim, 0, n - 1).add_(t)
            tot.narrow(dim, 1, n - 1).add_(t)
    return float(tot.max()) / d.numel()


def _close(reg, d, wrap, G, part, lam=1.0):
    """The issue's bounds: value within 1e-13 relative, |G - G_ref| <= 64 * 2^-53 * A (each side
    makes at most 8 additions and 3 multiplications per voxel)."""
    val, g_ref = _formula(reg, d, wrap)
    got = float(part.sum() / d.numel())
    assert abs(got - float(val)) <= 1e-13 * abs(float(val)), (got, float(val))
    A = _abs_terms(reg, d, wrap) * abs(lam)
    err = float((G - lam * g_ref).abs().max())
    print(f'smooth_reg {reg.smooth_kind} {tuple(d.shape)} wrap {wrap}: value {got:.6g} '
          f'(rel err {abs(got - float(val)) / max(abs(float(val)), 1e-300):.2g}), '
          f'gradient err {err:.3g}, bound {64 * EPS * A:.3g}')
    assert err <= 64 * EPS * A, (err, 64 * EPS * A)


# ---- 1. exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize('wrap', [False, True], ids=['open', 'wrap'])
@pytest.mark.parametrize('kind', KIND_IDS)
@pytest.mark.parametrize('shape, time_weight', [((4, 8, 16), 0), ((2, 4, 8, 16), 4),
                                                ((2, 2, 4, 8, 16), 4)], ids=['3d', 'time', 'batch'])
def test_exact_against_the_formula(shape, time_weight, kind, wrap, gpu):
    """Integer values in [-8, 8], weights that are powers of two, a power-of-two N, delta = 2:
    every product and sum is exact on both sides, so value and gradient are equal (as values:
    the sign of a zero gradient, +0 from the kernel, is not compared)."""
    reg = _reg(kind, 2 if kind == 'huber' else None, weights=(0.5, 2, 1), time_weight=time_weight)
    g = tr.Generator().manual_seed(31)
    d = tr.randint(-8, 9, shape, generator=g).to(F64).to(gpu)
    G, part, _ = _kernel(reg, d, wrap)
    val, g_ref = _formula(reg, d, wrap)
    assert float(val) > 0 and float(g_ref.abs().max()) > 0
    assert float(part.sum() / d.numel()) == float(val)
    assert tr.equal(G, g_ref)
    # the time axis counts: without its weight the leading axis is batch
    if time_weight:
        G0, part0, _ = _kernel(_reg(kind, reg.delta, weights=(0.5, 2, 1)), d, wrap)
        assert float(part0.sum()) < float(part.sum()) and not tr.equal(G0, G)


# ---- 2. edges ------------------------------------------------------------------------------------
EDGE_SHAPES = [((1, 1, 1), False, 0), ((1, 5, 1), False, 0), ((3, 1, 2), True, 0),
               ((5, 3, 1), True, 0), ((7, 5, 3), None, 0), ((3, 5, 4, 7), None, 1.5),
               ((67, 63, 65), None, 0)]


def _data(what, shape, delta, gpu):
    g = tr.Generator().manual_seed(37)
    if what == 'normal':
        d = tr.randn(shape, dtype=F64, generator=g)
    elif what == 'ties':                    # many neighbours exactly equal
        d = tr.round(tr.randn(shape, dtype=F64, generator=g))
    else:                                   # differences of exactly 0, +-delta, +-2 delta
        d = tr.randint(-1, 2, shape, generator=g).to(F64) * (delta or 0.5)
    return d.to(gpu)


@pytest.mark.parametrize('kind, delta', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('shape, wrap, time_weight', EDGE_SHAPES,
                         ids=['x'.join(map(str, s[0])) for s in EDGE_SHAPES])
def test_edges_against_the_formula(shape, wrap, time_weight, kind, delta, gpu):
    reg = _reg(kind, delta, weights=(0.7, 1.3, 2.1), time_weight=time_weight)
    if math.prod(shape) > 1024 * 256:
        assert math.prod(shape) == 274365      # the grid-stride loop's second element
    for what in ('normal', 'ties', 'delta'):
        d = _data(what, shape, delta, gpu)
        for wr in ((False, True) if wrap is None else (wrap,)):
            G, part, _ = _kernel(reg, d, wr, lam=0.75)
            _close(reg, d, wr, G, part, lam=0.75)
            if shape[-1] == 1 and wr:                         # no ring of one: wrap changes nothing
                G1, part1, _ = _kernel(reg, d, False, lam=0.75)
                assert tr.equal(G, G1) and tr.equal(part, part1)
    if shape == (1, 1, 1):
        assert float(G) == 0.0 and float(part.sum()) == 0.0
    if shape == (3, 1, 2):                                    # the double edge
        d = _data('normal', shape, delta, gpu)
        only_a = _reg(kind, delta, weights=(0, 0, 1))
        _, p_open, _ = _kernel(only_a, d, False)
        _, p_ring, _ = _kernel(only_a, d, True)
        assert abs(float(p_ring.sum()) - 2 * float(p_open.sum())) <= 1e-15 * float(p_ring.sum())


# ---- 3. non-finite values ------------------------------------------------------------------------
@pytest.mark.parametrize('kind, delta', KINDS, ids=KIND_IDS)
def test_one_nan_voxel(kind, delta, gpu):
    """One NaN voxel poisons itself and its at most 8 neighbours (6 on a static grid) and nothing
    else, and the value: the NaN pattern of the torch formula (under 'abs' the gradient stays
    finite, sign(NaN) = 0 on the device, and only the value is NaN)."""
    shape = (5, 6, 7)
    reg = _reg(kind, delta, weights=(0.7, 1.3, 2.1))
    clean = _data('normal', shape, delta, gpu)
    for pos in ((2, 3, 3), (0, 0, 0), (4, 5, 6), (1, 2, 0)):
        for wrap in (False, True):
            d = clean.clone()
            d[pos] = float('nan')
            G, part, _ = _kernel(reg, d, wrap)
            val, g_ref = _formula(reg, d, wrap)
            assert math.isnan(float(part.sum())) and math.isnan(float(val))
            assert tr.equal(G.isnan(), g_ref.isnan())
            near = tr.zeros(shape, dtype=tr.bool, device=gpu)
            near[pos] = True
            for ax in range(3):
                for s in (-1, 1):
                    q = list(pos)
                    q[ax] += s
                    if ax == 2 and wrap:
                        q[ax] %= shape[ax]
                    if 0 <= q[ax] < shape[ax]:
                        near[tuple(q)] = True
            assert 4 <= int(near.sum()) <= 7
            if kind == 'abs':
                assert not bool(G.isnan().any())
            else:
                assert tr.equal(G.isnan(), near)
            # the voxels that do not touch the NaN are those of the clean volume, bit for bit
            Gc, _, _ = _kernel(reg, clean, wrap)
            assert tr.equal(G[~near], Gc[~near])
            ok = ~G.isnan()
            A = _abs_terms(reg, d.nan_to_num(0.0), wrap)
            assert float((G[ok] - g_ref[ok]).abs().max()) <= 64 * EPS * A


# ---- 4. the folded form --------------------------------------------------------------------------
def _i64(x):
    return x.contiguous().view(tr.int64)


@pytest.mark.parametrize('kind, delta', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('shape', [(7, 5, 3), (67, 63, 65)], ids=['7x5x3', '67x63x65'])
def test_folded_form(shape, kind, delta, gpu):
    """With g_in and part_neg: g_out = g_in + (G - c_neg [d < 0]) bitwise, G the stand-alone
    call's with the same lam; part_neg what sphrt_neg_reg_f64 leaves; in place the same bits;
    g_in without part_neg adds G itself."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    reg = _reg(kind, delta, weights=(0.7, 1.3, 2.1))
    lam, c_neg = 0.3, 0.37 / math.prod(shape)
    d = _data('normal', shape, delta, gpu)
    assert 0.3 < float((d < 0).double().mean()) < 0.7
    g_in = tr.randn(shape, dtype=F64, generator=tr.Generator().manual_seed(41)).to(gpu) * 1e-3
    for wrap in (False, True):
        G, part, _ = _kernel(reg, d, wrap, lam=lam)
        out, part_f, part_neg = _kernel(reg, d, wrap, lam=lam, c_neg=c_neg, g_in=g_in, neg=True)
        want = g_in + tr.where(d < 0, G - c_neg, G)
        assert tr.equal(_i64(out), _i64(want))
        assert tr.equal(_i64(part_f), _i64(part))
        scratch = tr.zeros_like(d)
        ref_neg = tr.full_like(part_neg, float('nan'))
        _lib.check(lib.sphrt_neg_reg_f64(_lib.ptr(d), d.numel(), c_neg, _lib.ptr(scratch),
                                         _lib.ptr(ref_neg), _lib.stream_of(gpu)), 'neg_reg')
        assert tr.equal(_i64(part_neg), _i64(ref_neg)) and float(part_neg.sum()) > 0
        g = g_in.clone()
        same, part_i, part_neg_i = _kernel(reg, d, wrap, lam=lam, c_neg=c_neg, g_in=g, g_out=g,
                                           neg=True)
        assert same is g and tr.equal(_i64(g), _i64(want))
        assert tr.equal(_i64(part_i), _i64(part)) and tr.equal(_i64(part_neg_i), _i64(ref_neg))
        plain, _, none = _kernel(reg, d, wrap, lam=lam, c_neg=c_neg, g_in=g_in)
        assert none is None and tr.equal(_i64(plain), _i64(g_in + G))


# ---- 5. the Function -----------------------------------------------------------------------------
@pytest.mark.parametrize('kind, delta', KINDS, ids=KIND_IDS)
def test_function_and_formula_paths(kind, delta, gpu):
    from sph_raytracer_amd import SphericalGrid
    shape = (7, 5, 6)
    op = types.SimpleNamespace(grid=SphericalGrid(shape=shape))          # a full ring: wraps
    base = _data('normal', shape, delta, gpu)
    reg = 0.5 * _reg(kind, delta, weights=(0.7, 1.3, 2.1))
    assert reg.wraps(op)
    G, part, _ = _kernel(reg, base, True)
    d = base.clone().requires_grad_()
    val = reg(op, None, d, d)
    assert '_SmoothFunction' in type(val.grad_fn.next_functions[0][0]).__name__ \
        or '_SmoothFunction' in type(val.grad_fn).__name__
    assert float(val.detach()) == 0.5 * float(part.sum() / base.numel())
    val.backward()
    assert tr.equal(_i64(d.grad), _i64(G * 0.5))
    # under no_grad (use_grad=False) the same value, no graph
    mon = 0.5 * _reg(kind, delta, weights=(0.7, 1.3, 2.1), use_grad=False)
    v2 = mon(op, None, d, d)
    assert not v2.requires_grad and float(v2) == float(val.detach())
    # a non-contiguous float64 density takes the formula: the bound of the edge tests
    nc = base.permute(0, 2, 1)
    assert not nc.is_contiguous()
    x = nc.clone(memory_format=tr.preserve_format).requires_grad_()
    assert not x.is_contiguous()
    v = reg(op, None, x, x)
    assert 'SmoothFunction' not in type(v.grad_fn.next_functions[0][0]).__name__
    v.backward()
    dc = nc.contiguous()
    Gc, partc, _ = _kernel(reg, dc, True)
    assert abs(float(v.detach()) - 0.5 * float(partc.sum() / dc.numel())) <= 1e-13 * float(v.detach())
    assert float((x.grad - 0.5 * Gc).abs().max()) <= 64 * EPS * 0.5 * _abs_terms(reg, dc, True)
    # float32 takes the formula in float32: the same bounds with float32's 2^-24 for 2^-53, the
    # value's from its at most n_edges additions of non-negative terms
    x32 = base.to(F32).requires_grad_()
    v32 = reg(op, None, x32, x32)
    assert v32.dtype == F32
    v32.backward()
    d32 = x32.detach().to(F64)
    G32, part32, _ = _kernel(reg, d32, True)
    want = 0.5 * float(part32.sum() / d32.numel())
    n_edges = 3 * base.numel()
    assert abs(float(v32.detach()) - want) <= (n_edges + 4) * 2.0 ** -24 * want
    assert float((x32.grad.to(F64) - 0.5 * G32).abs().max()) \
        <= 64 * 2.0 ** -24 * 0.5 * _abs_terms(reg, d32, True)
    # a backward that is differentiated comes from the formula
    if kind == 'square':
        a = base.clone().requires_grad_()
        g1, = tr.autograd.grad(reg(op, None, a, a), a, create_graph=True)
        (g1 ** 2).sum().backward()
        b = base.clone().requires_grad_()
        g2, = tr.autograd.grad(0.5 * reg.formula(b, True), b, create_graph=True)
        (g2 ** 2).sum().backward()
        assert float(a.grad.abs().max()) > 0
        assert float((a.grad - b.grad).abs().max()) <= 1e-12 * float(b.grad.abs().max())


# ---- 6. gd ---------------------------------------------------------------------------------------
GD_SEED = 274


def _terms(kind, delta, arrangement):
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    fid, neg, sm = SquareLoss(), 2 * NegRegularizer(), 0.5 * _reg(kind, delta)
    return {'neg_smooth': [fid, neg, sm], 'smooth_neg': [fid, sm, neg], 'smooth': [fid, sm]}[
        arrangement], fid, neg, sm


def _run(op, meas, model, fns, c0, n_it=25, **kw):
    from sph_raytracer_amd import retrieval
    c, yh, hist = retrieval.gd(op, meas.clone(), model, coeffs=c0.clone(), lr=1e-1,
                               num_iterations=n_it, loss_fns=fns, progress_bar=False, **kw)
    assert list(hist) == fns
    return c.detach().clone(), yh.detach().clone(), [list(hist[fn]) for fn in fns]


@pytest.mark.parametrize('arrangement', ['neg_smooth', 'smooth_neg', 'smooth'])
@pytest.mark.parametrize('kind, delta', KINDS, ids=KIND_IDS)
def test_gd_direct_matches_autograd(kind, delta, arrangement, gpu, monkeypatch, circ16):  # noqa: F811
    """gd() with [SquareLoss, 2 NegRegularizer, 0.5 SmoothRegularizer] (the regularisers in both
    orders, and without the NegRegularizer) over a stored Operator takes `_gd_direct` once and
    gives the autograd loop's coefficients and reconstruction bitwise, its loss histories within
    1e-13 relative; from 0.5 + rand the smooth term decreases."""
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom, op, meas = circ16
    model = FullyDenseModel(grid)
    c0 = 0.5 + _rand(grid.shape, F64, GD_SEED, gpu)
    fns, fid, neg, sm = _terms(kind, delta, arrangement)
    want = (fid, neg if arrangement != 'smooth' else None, sm)
    assert sm.wraps(op)
    assert retrieval._direct_plan(op, meas, model, c0, fns, [c0]) == want
    calls = []
    direct = retrieval._gd_direct
    monkeypatch.setattr(retrieval, '_gd_direct', lambda *a, **k: calls.append(1) or direct(*a, **k))
    ca, ya, ha = _run(op, meas, model, fns, c0)
    assert len(calls) == 1
    with monkeypatch.context() as mp:
        mp.setattr(retrieval, '_direct_plan', lambda *a: None)
        cb, yb, hb = _run(op, meas, model, _terms(kind, delta, arrangement)[0], c0)
    assert len(calls) == 1
    assert len(ha) == len(hb) == len(fns) and all(len(h) == 25 for h in ha + hb)
    for la, lb in zip(ha, hb):
        assert np.allclose(la, lb, rtol=1e-13, atol=0), (la, lb)
    assert tr.equal(ca, cb) and tr.equal(ya, yb)
    h_sm = ha[fns.index(sm)]
    assert ha[0][-1] < ha[0][0] and 0 < h_sm[-1] < h_sm[0]
    print(f'gd {kind} {arrangement}: fidelity {ha[0][0]:.4g} -> {ha[0][-1]:.4g}, smooth '
          f'{h_sm[0]:.4g} -> {h_sm[-1]:.4g}')


@pytest.mark.parametrize('kind, delta', KINDS, ids=KIND_IDS)
def test_gd_direct_with_sgd_matches_autograd(kind, delta, gpu, monkeypatch, circ16):  # noqa: F811
    """A non-Adam optimiser takes the direct loop with the entry in place of sphrt_neg_reg_f64
    (no Adam launch, no neg_reg launch) and is bitwise the autograd loop."""
    from sph_raytracer_amd import _lib, retrieval
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom, op, meas = circ16
    model = FullyDenseModel(grid)
    c0 = 0.5 + _rand(grid.shape, F64, GD_SEED, gpu)
    calls = []
    direct = retrieval._gd_direct
    monkeypatch.setattr(retrieval, '_gd_direct', lambda *a, **k: calls.append(1) or direct(*a, **k))
    lib = _lib.load()
    seen = {'neg': 0, 'smooth': 0}
    neg_reg, smooth_reg = lib.sphrt_neg_reg_f64, lib.sphrt_smooth_reg_f64

    def count(name, fn):
        def wrapped(*a):
            seen[name] += 1
            return fn(*a)
        return wrapped

    for arrangement in ('neg_smooth', 'smooth'):
        fns = _terms(kind, delta, arrangement)[0]
        with monkeypatch.context() as mp:
            mp.setattr(lib, 'sphrt_neg_reg_f64', count('neg', neg_reg))
            mp.setattr(lib, 'sphrt_smooth_reg_f64', count('smooth', smooth_reg))
            ca, ya, ha = _run(op, meas, model, fns, c0, optim=tr.optim.SGD)
        assert len(calls) == 1 and seen == {'neg': 0, 'smooth': 25}
        with monkeypatch.context() as mp:
            mp.setattr(retrieval, '_direct_plan', lambda *a: None)
            cb, yb, hb = _run(op, meas, model, _terms(kind, delta, arrangement)[0], c0,
                              optim=tr.optim.SGD)
        assert len(calls) == 1
        for la, lb in zip(ha, hb):
            assert np.allclose(la, lb, rtol=1e-13, atol=0), (la, lb)
        assert tr.equal(ca, cb) and tr.equal(ya, yb) and not tr.equal(ca, c0)
        calls.clear()
        seen.update(neg=0, smooth=0)


@pytest.mark.parametrize('arrangement', ['neg_smooth', 'smooth'])
@pytest.mark.parametrize('kind, delta', KINDS, ids=KIND_IDS)
def test_gd_takes_the_fused_loop(kind, delta, arrangement, gpu, monkeypatch):
    """The same over a MatrixFreeOperator: _fused_plan accepts; with deterministic=True two runs
    give equal bits and the coefficients are within 1e-9 of the autograd loop over the same
    operator."""
    from sph_raytracer_amd import retrieval
    case, op, meas, model, _, _ = _gd_circ16(gpu)
    c0 = 0.5 + _rand(model.coeffs_shape, F64, GD_SEED, gpu)
    fns, fid, neg, sm = _terms(kind, delta, arrangement)
    assert retrieval._direct_plan(op, meas, model, c0, fns, [c0]) is None
    assert retrieval._fused_plan(op, meas, model, c0, fns, [c0]) == \
        (fid, neg if arrangement != 'smooth' else None, sm)
    calls = []
    direct = retrieval._gd_direct
    monkeypatch.setattr(retrieval, '_gd_direct', lambda *a, **k: calls.append(1) or direct(*a, **k))
    op.deterministic = True
    try:
        det = [_run(op, meas, model, _terms(kind, delta, arrangement)[0], c0) for _ in range(2)]
        assert len(calls) == 2
        assert tr.equal(det[0][0], det[1][0]) and tr.equal(det[0][1], det[1][1])
        for h0, h1 in zip(det[0][2], det[1][2]):
            assert _bits(h0) == _bits(h1)
        with monkeypatch.context() as mp:
            mp.setattr(retrieval, '_fused_plan', lambda *a: None)
            auto = _run(op, meas, model, _terms(kind, delta, arrangement)[0], c0)
        assert len(calls) == 2
    finally:
        op.deterministic = False
    e_c = float((det[0][0] - auto[0]).abs().max())
    print(f'fused gd {kind} {arrangement}: coefficients within {e_c:.3g} of the autograd loop')
    assert e_c <= 1e-9
    h_sm = det[0][2][fns.index(sm)]
    for k in (0, fns.index(sm)):
        assert np.allclose(det[0][2][k], auto[2][k], rtol=1e-9, atol=0)
    assert 0 < h_sm[-1] < h_sm[0]


# ---- 7. a dynamic grid ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind, delta', KINDS, ids=KIND_IDS)
def test_gd_on_a_dynamic_grid_with_a_time_weight(kind, delta, gpu, monkeypatch):
    """The direct plans decline dynamic operators: gd runs the autograd loop, the smooth term
    through its Function on the (t, r, e, a) density, to the end with a finite total that
    decreases from its first to its last value; the time weight counts."""
    from sph_raytracer_amd import ConeCircGeom, Operator, SphericalGrid, retrieval
    from sph_raytracer_amd.loss import SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    grid = SphericalGrid(shape=DGRID)
    geom = sum(ConeCircGeom((24, 16), pos=p, fov=(0, 12)) for p in _orbit(T_DYN))
    op = Operator(grid, geom, dynamic=True, device=gpu)
    meas = op(_rand(DGRID, F64, 5, gpu)).detach()
    model = FullyDenseModel(grid)
    c0 = 0.5 + _rand(DGRID, F64, 6, gpu)
    calls = []
    direct = retrieval._gd_direct
    monkeypatch.setattr(retrieval, '_gd_direct', lambda *a, **k: calls.append(1) or direct(*a, **k))
    fid, sm = SquareLoss(), 0.5 * _reg(kind, delta, time_weight=2.0)
    c, yh, hist = retrieval.gd(op, meas.clone(), model, coeffs=c0.clone(), lr=1e-1,
                               num_iterations=15, loss_fns=[fid, sm], progress_bar=False)
    assert not calls and c.shape == DGRID
    total = [a + b for a, b in zip(hist[fid], hist[sm])]
    assert len(total) == 15 and all(math.isfinite(v) for v in total) and total[-1] < total[0]
    assert bool(c.detach().isfinite().all())
    # the first value is the formula's with the time edges, more than without them
    first = float(0.5 * sm.formula(c0, True))
    assert abs(hist[sm][0] - first) <= 1e-13 * first
    assert first > float(0.5 * _reg(kind, delta).formula(c0, True))
