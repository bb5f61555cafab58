"""The ray-side launch of retrieval.chambolle_pock (csrc/loss.hip: sphrt_cp_ray_dual_f64, declared
in include/sphrt_cp.h) against its op-by-op restatement in torch on the same device
(cp_cases.ray_dual_ref, shown sound on the CPU by test_cp_cpu.py), bit for bit:

  sizes     1, 255, 256, 257 elements, 262145 (one past 1024 workgroups x 256: the grid-stride
            loop's second pass) and 524291, every kind, with `order` null and a random
            permutation: p, p_adj and both rows of partial sums (cg_cases.block_partials, the
            documented workgroup order, over the restatement's terms);
  specials  s = 0 gives +0.0; NaN, +-inf, signed zeros and denormals in every operand; a float32
            y promoted exactly; an argument exactly on each clamp bound stores the bound's bits;
  refusals  on the host: nothing is launched, the outputs keep their fill.

The build compiles division and sqrt as the correctly rounded IEEE operations (no fast-math
flag; -ffp-contract=off), so the Poisson kind is held bit for bit like the others.
Every buffer a launch writes sits between 64-element NaN guards."""
import ctypes

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import cp_cases as cp
import loop_cases as lc
from test_gpu_fista_kernels import _Buf, _same

pytestmark = pytest.mark.gpu
F64 = tr.float64
SIZES = [1, 255, 256, 257, 262145, 524291]
SIGMA = 0.37


def _inputs(kind, n, seed):
    """z_new, z_old, y, s, w, p as float64 numpy vectors: both sides of every clamp occur."""
    rng = np.random.default_rng(seed)
    z_new, z_old = np.abs(rng.standard_normal(n)) + 0.1, np.abs(rng.standard_normal(n)) + 0.1
    y = 10.0 ** rng.uniform(-2, 1, n) if kind == 'poisson' else rng.standard_normal(n)
    s = 10.0 ** rng.uniform(-2, 0, n)
    s[rng.random(n) < 0.05] = 0.0
    w = rng.random(n) + 0.25
    p = rng.uniform(-1, 1, n) * s * (cp.HUBER_DELTA if kind == 'huber' else 1.0)
    if kind == 'huber':
        # the clamp is narrow (delta = 0.05): place t = a - sigma y at -2.5 .. 2.5 times the
        # argument that lands on the bound, so that the inside and both sides all occur
        on_bound = cp.HUBER_DELTA * (s + SIGMA)
        y = (2 * z_new - z_old) + (p - rng.uniform(-2.5, 2.5, n) * on_bound) / SIGMA
    return z_new, z_old, y, s, w, p


def _launch(gpu, kind, z_new, z_old, y, s, w, p, sigma=SIGMA, order=None, y32=False):
    """-> (p, p_adj or None, part_pp, part_fid) as numpy, guards and inputs checked."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    n = len(p)
    bz, bo, bs, bw, bp = (_Buf(v, gpu) for v in (z_new, z_old, s, w, p))
    yt = tr.from_numpy(np.ascontiguousarray(y)).to(gpu)
    yt = yt.float() if y32 else yt
    sg = _Buf(np.array([sigma]), gpu)
    g = lc.grid_of(n)
    assert lib.sphrt_loss_partials(n) == g
    pp, fid = _Buf(g, gpu), _Buf(g, gpu)
    padj = _Buf(n, gpu) if order is not None else None
    ot = tr.from_numpy(order.astype(np.int32)).to(gpu) if order is not None else None
    _lib.check(lib.sphrt_cp_ray_dual_f64(
        bz.ptr(), bo.ptr(), _lib.ptr(yt), int(not y32), n, cp.KIND_ID[kind], cp.par_of(kind),
        bs.ptr(), bw.ptr(), sg.ptr(), _lib.ptr(ot), bp.ptr(), padj.ptr() if padj else None,
        pp.ptr(), fid.ptr(), _lib.stream_of(gpu)), 'sphrt_cp_ray_dual_f64')
    tr.cuda.synchronize(gpu)
    assert all(b.guards_ok() for b in (bz, bo, bs, bw, bp, sg, pp, fid) + ((padj,) if padj else ()))
    assert _same(bz.host(), z_new) and _same(bo.host(), z_old) and _same(bs.host(), s)
    assert _same(bw.host(), w) and _same(sg.host(), [sigma])
    return bp.host(), padj.host() if padj else None, pp.host(), fid.host()


def _reference(gpu, kind, z_new, z_old, y, s, w, p, sigma=SIGMA, order=None, exact=False):
    dev = [tr.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in (z_new, z_old, y, s, w, p)]
    ot = tr.from_numpy(order.astype(np.int64)).to(gpu) if order is not None else None
    pn, padj, tpp, tfid = cp.ray_dual_ref(kind, *dev[:5], sigma, dev[5], order=ot,
                                          fma=cp.fma_exact if exact else cp.fma_eft)
    with np.errstate(all='ignore'):
        return (pn.cpu().numpy(), padj.cpu().numpy() if padj is not None else None,
                cc.block_partials(tpp.cpu().numpy()), cc.block_partials(tfid.cpu().numpy()))


def _compare(got, want, what):
    for name, a, b in zip(('p', 'p_adj', 'part_pp', 'part_fid'), got, want):
        if b is None:
            assert a is None
            continue
        bad = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))
        assert _same(a, b), (what, name, len(bad), bad[:4], a[bad[:4]], b[bad[:4]])


@pytest.mark.parametrize('perm', [False, True], ids=['plain', 'order'])
@pytest.mark.parametrize('kind', cp.KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_bitwise_against_the_restatement(n, kind, perm, gpu):
    args = _inputs(kind, n, seed=n + cp.KIND_ID[kind])
    order = np.random.default_rng(n).permutation(n) if perm else None
    got = _launch(gpu, kind, *args, order=order)
    want = _reference(gpu, kind, *args, order=order, exact=n <= 600)
    _compare(got, want, (n, kind, perm))
    s, p_new = args[3], got[0]
    assert not np.isnan(p_new).any()
    zero = s == 0
    assert not p_new[zero].any() and not np.signbit(p_new[zero]).any()
    if perm:
        assert _same(got[1], p_new[order])
    if n >= 255:                     # every branch of the kind's clamp occurs
        b = {'abs': s, 'huber': s * cp.HUBER_DELTA, 'poisson': s}.get(kind)
        if b is not None:
            live = ~zero
            assert np.all(p_new <= b) and (p_new[live] < b[live]).sum() > n / 50
            if kind != 'poisson':        # (the Poisson root reaches s by rounding alone)
                assert (p_new[live] == b[live]).sum() > n / 50
                assert (p_new[live] == -b[live]).sum() > n / 50 and np.all(p_new >= -b)
                inside = np.abs(p_new[live]) < b[live]
                assert inside.sum() > n / 50


SPECIALS = [0.0, -0.0, 5e-324, -5e-324, 2.2e-308, 1e-160, -1e160, 1e308, -1e308, np.inf, -np.inf,
            np.nan]


@pytest.mark.parametrize('kind', cp.KINDS)
def test_special_values_follow_the_documented_sequence(kind, gpu):
    """Each operand in turn takes every special value at positions spread over two workgroups,
    the others staying ordinary; the restatement's fmas are rounded once through rationals."""
    n = 315
    base = _inputs(kind, n, seed=9)
    rng = np.random.default_rng(5)
    for k in range(6):
        args = [v.copy() for v in base]
        where = rng.permutation(n)[:5 * len(SPECIALS)]
        args[k][where] = np.tile(SPECIALS, 5)
        for sigma in (SIGMA, 0.0):
            got = _launch(gpu, kind, *args, sigma=sigma)
            want = _reference(gpu, kind, *args, sigma=sigma, exact=True)
            _compare(got, want, (kind, k, sigma))
            zero = args[3] == 0
            assert not got[0][zero].any() and not np.signbit(got[0][zero]).any()
        assert np.isnan(got[0]).any() or k in (3, 4)       # (a NaN stays NaN through the clamps)
    assert where.min() < 256 <= where.max()


@pytest.mark.parametrize('kind', cp.KINDS)
def test_float32_measurements_are_promoted_exactly(kind, gpu):
    args = list(_inputs(kind, 257, seed=3))
    args[2] = args[2].astype(np.float32).astype(np.float64)
    order = np.random.default_rng(1).permutation(257)
    _compare(_launch(gpu, kind, *args, order=order, y32=True),
             _launch(gpu, kind, *args, order=order), kind)


def test_an_argument_on_a_clamp_bound_stores_the_bound(gpu):
    n = 6
    zero = np.zeros(n)
    s = np.array([0.3, 0.3, 0.7, 0.7, 1e-3, 1e-3])
    side = np.array([1.0, -1.0] * 3)
    # abs: z = y = 0, so t = p: p = +-s stays, bit for bit
    p, _, _, _ = _launch(gpu, 'abs', zero, zero, zero, s, np.ones(n), side * s)
    assert _same(p, side * s)
    # huber: sigma = s makes the divisor 2, t = +-2 (s delta) lands on the bound exactly
    for k in range(n):
        b = s[k] * cp.HUBER_DELTA
        p, _, _, _ = _launch(gpu, 'huber', zero[:1], zero[:1], zero[:1], s[k:k + 1], np.ones(1),
                             np.array([side[k] * 2 * b]), sigma=float(s[k]))
        assert _same(p, [side[k] * b])
    # poisson: a far above s runs into the upper clamp and stores s
    p, _, _, _ = _launch(gpu, 'poisson', zero + 1.0, zero + 1.0, zero + 2.0, s, np.ones(n),
                         s * 0 + 1e6)
    assert np.all(p <= s) and not np.isnan(p).any()
    # sigma = 0 and p = 3 s: d = 2 s and e = 4 s exactly, v = s: the bound itself
    p, _, _, _ = _launch(gpu, 'poisson', zero + 1.0, zero + 1.0, zero, s, np.ones(n), 3 * s,
                         sigma=0.0)
    assert _same(p, s)


def test_refusals_leave_every_buffer_untouched(gpu):
    from sph_raytracer_amd import _lib
    lib, st = _lib.load(), _lib.stream_of(gpu)
    n = 300
    zv, ov, yv, sv, wv, pv = _inputs('huber', n, seed=1)
    z, o, y, s, w, p = (_Buf(v, gpu) for v in (zv, ov, yv, sv, wv, pv))
    sg, pp, fid, padj = _Buf(np.array([SIGMA]), gpu), _Buf(2, gpu), _Buf(2, gpu), _Buf(n, gpu)
    order = tr.randperm(n, device=gpu).int()
    nan, inf = float('nan'), float('inf')

    def call(z=z.ptr(), o=o.ptr(), y=y.ptr(), n=n, kind=2, par=0.5, s=s.ptr(), w=w.ptr(),
             sg=sg.ptr(), order=_lib.ptr(order), p=p.ptr(), padj=padj.ptr(), pp=pp.ptr(),
             fid=fid.ptr()):
        return lib.sphrt_cp_ray_dual_f64(z, o, y, 1, n, kind, par, s, w, sg, order, p, padj, pp,
                                         fid, st)

    cases = [(dict(n=0), b'empty'), (dict(n=-5), b'empty'), (dict(kind=-1), b'kind'),
             (dict(kind=4), b'kind')]
    cases += [({k: None}, b'null') for k in ('z', 'o', 'y', 's', 'w', 'sg', 'p', 'pp', 'fid',
                                              'order', 'padj')]
    cases += [(dict(kind=k, par=v), word) for k, word in ((2, b'delta'), (3, b'eps'))
              for v in (nan, 0.0, -1.0, inf, -inf)]
    cases += [(dict(padj=p.ptr()), b'alias'),
              (dict(padj=ctypes.c_void_p(p.ptr().value + 8 * (n - 1))), b'alias'),
              (dict(p=z.ptr()), b'alias'), (dict(pp=fid.ptr()), b'alias'),
              (dict(fid=sg.ptr()), b'alias'), (dict(padj=y.ptr()), b'alias')]
    for i, (kw, word) in enumerate(cases):
        assert call(**kw) != 0, (i, kw)
        assert word in lib.sphrt_last_error(), (i, kw, lib.sphrt_last_error())
    tr.cuda.synchronize(gpu)
    assert all(bool(tr.isnan(b.view).all()) for b in (padj, pp, fid)) and _same(p.host(), pv)
    # the same arguments unchanged are accepted, and so is the pair of nulls
    assert call() == 0 and call(order=None, padj=None) == 0
    assert call(kind=0, par=nan) == 0 and call(kind=1, par=-1.0) == 0     # (ignored there)
    tr.cuda.synchronize(gpu)
