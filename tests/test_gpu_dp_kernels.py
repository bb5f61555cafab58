"""The three entries of include/sphrt_dp.h (csrc/loss.hip: sphrt_dp_primal_f64,
sphrt_dp_ray_dual_f64, sphrt_dp_steps_f64) against their op-by-op restatements in dp_cases, bit for
bit throughout:

  sizes     1, 255, 256, 257 and 1024 * 256 + 257 elements (past one element per thread): every
            element and every workgroup's partial sum; the fmas of the restatement rounded once
            through rationals up to 600 elements, by error-free transformations above;
  volumes   1x1x1, 1x1x2 with the ring, 2x1x1, 3x2x2 with the ring, 5x4x7 open and closed, with
            every has_* mask: the primal step and the steps launch (deg from a brute-force edge
            list);
  ray dual  `order` null and a random permutation, all four kinds, per-ray steps with zeros among
            them; s = 0, sigma = 0, NaN, +-inf, signed zeros and denormals in every operand;
  against   with tau (sigma) filled with one value the primal (ray-dual) entry gives the bits of
  shipped   sphrt_pd_primal_f64 (sphrt_cp_ray_dual_f64) reading that value as its scalar;
  refusals  on the host: nothing is launched, the outputs keep their fill.
Every buffer a launch writes sits between 64-element NaN guards."""
import ctypes
import math

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import cp_cases as cp
import dp_cases as dc
import loop_cases as lc
from test_gpu_cp_kernels import SPECIALS, _inputs
from test_gpu_fista_kernels import _Buf, _same

pytestmark = pytest.mark.gpu
F64 = tr.float64
VOLUME_CASES = dc.volume_cases()
VOLUME_IDS = [dc.volume_id(c) for c in VOLUME_CASES]
LOWER, UPPER, C_DAMP = -0.61, 0.67, 0.3


def _L(gpu):
    from sph_raytracer_amd import _lib
    return _lib, _lib.load(), _lib.stream_of(gpu)


def _dev(v, gpu):
    return tr.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(gpu)


# ---- the primal step -----------------------------------------------------------------------------------
def _primal_inputs(shape, seed):
    """x, g (n), q (3, n), tau (n): steps over two decades with zeros among them, so that each
    clamp branch and the step that stays put all occur."""
    rng, n = np.random.default_rng(seed), math.prod(shape)
    x, g, q = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal((3, n))
    tau = 10.0 ** rng.uniform(-2, 0, n)
    tau[rng.random(n) < 0.1] = 0.0
    return x, g, q, tau


def _primal(gpu, entry, shape, wrap, has, x, g, q, tau, c_damp=C_DAMP, lower=LOWER, upper=UPPER):
    """-> (x_new, part_mm); tau an array (the dp entry) or one value (the pd entry)."""
    L, lib, st = _L(gpu)
    n = math.prod(shape)
    bx, bg, bq = _Buf(x, gpu), _Buf(g, gpu), _Buf(q.reshape(-1), gpu)
    bt = _Buf(np.atleast_1d(np.asarray(tau, dtype=np.float64)), gpu)
    bn, mm = _Buf(n, gpu), _Buf(lc.grid_of(n), gpu)
    L.check(getattr(lib, entry)(bx.ptr(), bg.ptr(), bq.ptr(), bn.ptr(), *shape, int(wrap), *has,
                                c_damp, bt.ptr(), lower, upper, mm.ptr(), st), entry)
    tr.cuda.synchronize(gpu)
    assert all(b.guards_ok() for b in (bx, bg, bq, bt, bn, mm))
    assert _same(bx.host(), x) and _same(bg.host(), g) and _same(bq.host(), q.reshape(-1))
    assert _same(bt.host(), np.atleast_1d(tau))
    return bn.host(), mm.host()


def _primal_want(gpu, shape, wrap, has, x, g, q, tau, exact, **kw):
    xn, terms = dc.primal_ref(_dev(x, gpu), _dev(g, gpu), _dev(q, gpu), _dev(tau, gpu), shape, wrap,
                              has, kw.get('c_damp', C_DAMP), kw.get('lower', LOWER),
                              kw.get('upper', UPPER), fma=cp.fma_exact if exact else cp.fma_eft)
    with np.errstate(all='ignore'):
        return xn.cpu().numpy(), cc.block_partials(terms.cpu().numpy())


@pytest.mark.parametrize('wrap', [False, True], ids=['open', 'ring'])
@pytest.mark.parametrize('n', dc.SIZES)
def test_primal_sizes_bitwise(n, wrap, gpu):
    shape, has = dc.SIZE_VOLUMES[n], (1, 1, 1)
    x, g, q, tau = _primal_inputs(shape, seed=n)
    got = _primal(gpu, 'sphrt_dp_primal_f64', shape, wrap, has, x, g, q, tau)
    want = _primal_want(gpu, shape, wrap, has, x, g, q, tau, exact=n <= 600)
    assert _same(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:4]
    assert _same(got[1], want[1])
    still = tau == 0
    assert _same(got[0][still], np.clip(x[still], LOWER, UPPER))
    if n >= 255:
        assert (got[0] == LOWER).any() and (got[0] == UPPER).any()
        assert ((got[0] > LOWER) & (got[0] < UPPER)).any()


@pytest.mark.parametrize('shape,wrap,has', VOLUME_CASES, ids=VOLUME_IDS)
def test_primal_volumes_bitwise(shape, wrap, has, gpu):
    x, g, q, tau = _primal_inputs(shape, seed=7 + sum(has))
    n = len(x)
    for k, val in enumerate([np.nan, np.inf, 5e-324, -0.0, -0.25][:n]):     # (not special-cased)
        tau[(3 * k) % n] = val
    for c_damp, bounds in ((C_DAMP, (LOWER, UPPER)), (0.0, (-np.inf, np.inf))):
        kw = dict(c_damp=c_damp, lower=bounds[0], upper=bounds[1])
        got = _primal(gpu, 'sphrt_dp_primal_f64', shape, wrap, has, x, g, q, tau, **kw)
        want = _primal_want(gpu, shape, wrap, has, x, g, q, tau, exact=True, **kw)
        assert _same(got[0], want[0]) and _same(got[1], want[1]), (c_damp, got[0], want[0])


@pytest.mark.parametrize('shape,wrap', [((5, 4, 7), False), ((5, 4, 7), True), ((3, 2, 2), True),
                                        (dc.SIZE_VOLUMES[dc.SIZES[-1]], True)])
def test_primal_with_one_step_is_the_scalar_entry(shape, wrap, gpu):
    x, g, q, _ = _primal_inputs(shape, seed=3)
    for has in dc.HAS[:4]:
        for tau in (0.37, 0.0):
            a = _primal(gpu, 'sphrt_dp_primal_f64', shape, wrap, has, x, g, q,
                        np.full(len(x), tau))
            b = _primal(gpu, 'sphrt_pd_primal_f64', shape, wrap, has, x, g, q, tau)
            assert _same(a[0], b[0]) and _same(a[1], b[1]), (has, tau)


# ---- the ray dual --------------------------------------------------------------------------------------
def _sigmas(n, seed):
    rng = np.random.default_rng(seed)
    sg = 0.37 * 10.0 ** rng.uniform(-0.5, 0.5, n)
    sg[rng.random(n) < 0.05] = 0.0
    return sg


def _ray(gpu, entry, kind, z_new, z_old, y, s, w, p, sigma, order=None, y32=False):
    """-> (p, p_adj or None, part_pp, part_fid); sigma an array (dp) or one value (cp)."""
    L, lib, st = _L(gpu)
    n = len(p)
    bz, bo, bs, bw, bp = (_Buf(v, gpu) for v in (z_new, z_old, s, w, p))
    yt = _dev(y, gpu)
    yt = yt.float() if y32 else yt
    sg = _Buf(np.atleast_1d(np.asarray(sigma, dtype=np.float64)), gpu)
    g = lc.grid_of(n)
    pp, fid = _Buf(g, gpu), _Buf(g, gpu)
    padj = _Buf(n, gpu) if order is not None else None
    ot = tr.from_numpy(order.astype(np.int32)).to(gpu) if order is not None else None
    L.check(getattr(lib, entry)(
        bz.ptr(), bo.ptr(), L.ptr(yt), int(not y32), n, cp.KIND_ID[kind], cp.par_of(kind), bs.ptr(),
        bw.ptr(), sg.ptr(), L.ptr(ot), bp.ptr(), padj.ptr() if padj else None, pp.ptr(), fid.ptr(),
        st), entry)
    tr.cuda.synchronize(gpu)
    assert all(b.guards_ok() for b in (bz, bo, bs, bw, bp, sg, pp, fid) + ((padj,) if padj else ()))
    assert _same(bz.host(), z_new) and _same(bo.host(), z_old) and _same(bs.host(), s)
    assert _same(bw.host(), w) and _same(sg.host(), np.atleast_1d(sigma))
    return bp.host(), padj.host() if padj else None, pp.host(), fid.host()


def _ray_want(gpu, kind, z_new, z_old, y, s, w, p, sigma, order=None, exact=False):
    dev = [_dev(v, gpu) for v in (z_new, z_old, y, s, w, sigma, p)]
    ot = tr.from_numpy(order.astype(np.int64)).to(gpu) if order is not None else None
    pn, padj, tpp, tfid = dc.ray_dual_ref(kind, *dev, order=ot,
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
@pytest.mark.parametrize('n', dc.SIZES)
def test_ray_dual_bitwise(n, kind, perm, gpu):
    args = _inputs(kind, n, seed=n + cp.KIND_ID[kind])
    sigma = _sigmas(n, seed=n)
    order = np.random.default_rng(n).permutation(n) if perm else None
    got = _ray(gpu, 'sphrt_dp_ray_dual_f64', kind, *args, sigma, order=order)
    want = _ray_want(gpu, kind, *args, sigma, order=order, exact=n <= 600)
    _compare(got, want, (n, kind, perm))
    s, p0, p_new = args[3], args[5], got[0]
    assert not np.isnan(p_new).any()
    zero = s == 0
    assert not p_new[zero].any() and not np.signbit(p_new[zero]).any()
    if perm:
        assert _same(got[1], p_new[order])
    if n >= 255:
        assert zero.any() and (sigma == 0).any() and (p_new != p0).any()
        b = {'abs': s, 'huber': s * cp.HUBER_DELTA, 'poisson': s}.get(kind)
        assert b is None or np.all(p_new <= b)


@pytest.mark.parametrize('kind', cp.KINDS)
def test_ray_dual_special_values_follow_the_documented_sequence(kind, gpu):
    """Each operand in turn — the per-ray step among them — takes every special value at
    positions spread over two workgroups, the others staying ordinary; the restatement's fmas
    are rounded once through rationals."""
    n = 315
    base = list(_inputs(kind, n, seed=9)) + [_sigmas(n, seed=2)]
    rng = np.random.default_rng(5)
    for k in range(7):
        args = [v.copy() for v in base]
        where = rng.permutation(n)[:5 * len(SPECIALS)]
        args[k][where] = np.tile(SPECIALS, 5)
        got = _ray(gpu, 'sphrt_dp_ray_dual_f64', kind, *args)
        want = _ray_want(gpu, kind, *args, exact=True)
        _compare(got, want, (kind, k))
        zero = args[3] == 0
        assert not got[0][zero].any() and not np.signbit(got[0][zero]).any()
        assert np.isnan(got[0]).any() or k in (3, 4)       # (a NaN stays NaN through the clamps)
    assert where.min() < 256 <= where.max()


@pytest.mark.parametrize('kind', cp.KINDS)
def test_ray_dual_with_one_step_is_the_scalar_entry(kind, gpu):
    for n in (257, dc.SIZES[-1]):
        args = list(_inputs(kind, n, seed=3))
        order = np.random.default_rng(1).permutation(n)
        for y32 in (False, True):
            if y32:
                args[2] = args[2].astype(np.float32).astype(np.float64)
            for sigma in (0.37, 0.0):
                for o in (None, order):
                    a = _ray(gpu, 'sphrt_dp_ray_dual_f64', kind, *args, np.full(n, sigma), order=o,
                             y32=y32)
                    b = _ray(gpu, 'sphrt_cp_ray_dual_f64', kind, *args, sigma, order=o, y32=y32)
                    _compare(a, b, (kind, n, y32, sigma, o is not None))


# ---- the steps -----------------------------------------------------------------------------------------
def _steps(gpu, col, row, shape, wrap, has, rho, c, order=None):
    L, lib, st = _L(gpu)
    bc, br = _Buf(col, gpu), _Buf(row, gpu)
    bt, bs = _Buf(len(col), gpu), _Buf(len(row), gpu)
    ot = tr.from_numpy(order.astype(np.int32)).to(gpu) if order is not None else None
    L.check(lib.sphrt_dp_steps_f64(bc.ptr(), br.ptr(), len(row), *shape, int(wrap), *has, rho, c,
                                   L.ptr(ot), bt.ptr(), bs.ptr(), st), 'sphrt_dp_steps_f64')
    tr.cuda.synchronize(gpu)
    assert all(b.guards_ok() for b in (bc, br, bt, bs))
    assert _same(bc.host(), col) and _same(br.host(), row)
    return bt.host(), bs.host()


def _check_steps(gpu, shape, wrap, has, n_ray, rho, c, perm):
    n_vox = math.prod(shape)
    col, row = dc.steps_inputs(n_vox, n_ray, seed=n_vox + n_ray)
    order = np.random.default_rng(n_ray).permutation(n_ray) if perm else None
    tau, sigma = _steps(gpu, col, row, shape, wrap, has, rho, c, order)
    want_tau, want_sigma = dc.steps_ref(col, row, shape, wrap, has, rho, c, order)
    assert _same(tau, want_tau), (np.flatnonzero(tau != want_tau)[:4], tau[:8], want_tau[:8])
    assert _same(sigma, want_sigma)
    # the guards: +0.0 wherever a denominator is not > 0 (NaN included), never a negative zero
    r = row[order] if perm else row
    with np.errstate(all='ignore'):
        dead = ~(r > 0)
    assert not sigma[dead].any() and not np.signbit(sigma[dead]).any()
    assert not np.isnan(tau).any() and not np.isnan(sigma).any() and not np.signbit(tau).any()
    return tau, sigma, col


@pytest.mark.parametrize('shape,wrap,has', VOLUME_CASES, ids=VOLUME_IDS)
def test_steps_volumes_bitwise(shape, wrap, has, gpu):
    for n_ray, perm in ((1, False), (300, True)):
        for rho, c in ((1.5 / 72, 0.0), (0.3, 1e-3)):
            tau, _, col = _check_steps(gpu, shape, wrap, has, n_ray, rho, c, perm)
            if c == 0:          # no ray, no edge, no damping: the voxel's step is +0.0
                lone = (dc.degree(shape, wrap, has) == 0) & (col == 0)
                assert not tau[lone].any()


@pytest.mark.parametrize('n', dc.SIZES)
def test_steps_sizes_bitwise(n, gpu):
    """n voxels against 257 rays and 140 voxels against n rays: either side the longer one."""
    _check_steps(gpu, dc.SIZE_VOLUMES[n], True, (1, 1, 1), 257, 0.0208, 1e-3, True)
    _check_steps(gpu, (5, 4, 7), True, (1, 1, 1), n, 0.0208, 0.0, True)
    _check_steps(gpu, (5, 4, 7), False, (1, 0, 1), n, 0.0208, 0.0, False)


# ---- refusals ------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_untouched(gpu):
    L, lib, st = _L(gpu)
    shape, n, m = (5, 4, 7), 140, 300
    xv, gv, qv, tv = _primal_inputs(shape, seed=1)
    x, g, q, tau = _Buf(xv, gpu), _Buf(gv, gpu), _Buf(qv.reshape(-1), gpu), _Buf(tv, gpu)
    xn, mm = _Buf(n, gpu), _Buf(1, gpu)
    zv, ov, yv, sv, wv, pv = _inputs('huber', m, seed=1)
    z, o, y, s, w, p = (_Buf(v, gpu) for v in (zv, ov, yv, sv, wv, pv))
    sg, pp, fid, padj = _Buf(_sigmas(m, 1), gpu), _Buf(2, gpu), _Buf(2, gpu), _Buf(m, gpu)
    order = tr.randperm(m, device=gpu).int()
    col, row = (_Buf(v, gpu) for v in dc.steps_inputs(n, m, seed=2))
    t_out, s_out = _Buf(n, gpu), _Buf(m, gpu)
    nan, inf = float('nan'), float('inf')
    VP = ctypes.c_void_p

    def primal(x=x.ptr(), g=g.ptr(), q=q.ptr(), xn=xn.ptr(), shape=shape, tau=tau.ptr(), lower=0.0,
               upper=1.0, mm=mm.ptr()):
        return lib.sphrt_dp_primal_f64(x, g, q, xn, *shape, 1, 1, 1, 1, 0.5, tau, lower, upper, mm, st)

    def ray(z=z.ptr(), o=o.ptr(), y=y.ptr(), n=m, kind=2, par=0.5, s=s.ptr(), w=w.ptr(),
            sg=sg.ptr(), order=L.ptr(order), p=p.ptr(), padj=padj.ptr(), pp=pp.ptr(), fid=fid.ptr()):
        return lib.sphrt_dp_ray_dual_f64(z, o, y, 1, n, kind, par, s, w, sg, order, p, padj, pp, fid,
                                         st)

    def steps(col=col.ptr(), row=row.ptr(), n_ray=m, shape=shape, rho=0.5, c=0.0,
              order=L.ptr(order), tau=t_out.ptr(), sigma=s_out.ptr()):
        return lib.sphrt_dp_steps_f64(col, row, n_ray, *shape, 1, 1, 1, 1, rho, c, order, tau,
                                      sigma, st)

    cases = []
    for fn in (primal, steps):
        cases += [(fn, dict(shape=v), b'axis') for v in ((0, 4, 7), (5, -1, 7), (5, 4, 0))]
        cases += [(fn, dict(shape=(2 ** 11, 2 ** 10, 2 ** 10)), b'2^31')]
    cases += [(primal, {k: None}, b'null') for k in ('x', 'g', 'q', 'xn', 'tau', 'mm')]
    cases += [(primal, dict(xn=x.ptr()), b'alias'), (primal, dict(xn=q.ptr()), b'alias'),
              (primal, dict(xn=tau.ptr()), b'alias'),
              (primal, dict(xn=VP(tau.ptr().value + 8 * (n - 1))), b'alias'),
              (primal, dict(mm=VP(tau.ptr().value + 8 * (n - 1))), b'alias'),
              (primal, dict(lower=nan), b'bound'), (primal, dict(lower=1.0), b'bound'),
              (primal, dict(lower=inf, upper=inf), b'bound')]
    cases += [(ray, dict(n=0), b'empty'), (ray, dict(n=-5), b'empty'), (ray, dict(kind=-1), b'kind'),
              (ray, dict(kind=4), b'kind')]
    cases += [(ray, {k: None}, b'null') for k in ('z', 'o', 'y', 's', 'w', 'sg', 'p', 'pp', 'fid',
                                                   'order', 'padj')]
    cases += [(ray, dict(kind=k, par=v), word) for k, word in ((2, b'delta'), (3, b'eps'))
              for v in (nan, 0.0, -1.0, inf, -inf)]
    cases += [(ray, dict(padj=p.ptr()), b'alias'), (ray, dict(p=z.ptr()), b'alias'),
              (ray, dict(pp=fid.ptr()), b'alias'), (ray, dict(p=sg.ptr()), b'alias'),
              (ray, dict(padj=VP(sg.ptr().value + 8 * (m - 1))), b'alias'),
              (ray, dict(fid=VP(sg.ptr().value + 8 * (m - 1))), b'alias')]
    cases += [(steps, {k: None}, b'null') for k in ('col', 'row', 'tau', 'sigma')]
    cases += [(steps, dict(n_ray=v), b'n_ray') for v in (0, -1, 2 ** 31)]
    cases += [(steps, dict(rho=v), b'rho') for v in (0.0, -1.0, nan, inf)]
    cases += [(steps, dict(c=v), b'c must') for v in (-1e-9, nan, inf)]
    cases += [(steps, dict(tau=col.ptr()), b'alias'), (steps, dict(sigma=row.ptr()), b'alias'),
              (steps, dict(sigma=t_out.ptr()), b'alias'),
              (steps, dict(tau=VP(col.ptr().value + 8 * (n - 1))), b'alias'),
              (steps, dict(sigma=L.ptr(order)), b'alias')]
    for i, (fn, kw, word) in enumerate(cases):
        assert fn(**kw) != 0, (i, fn.__name__, kw)
        assert word in lib.sphrt_last_error(), (i, fn.__name__, kw, lib.sphrt_last_error())
    tr.cuda.synchronize(gpu)
    assert all(bool(tr.isnan(b.view).all()) for b in (xn, mm, padj, pp, fid, t_out, s_out))
    assert _same(p.host(), pv)
    # the same arguments unchanged are accepted, and so are the optional nulls
    assert primal() == 0 and ray() == 0 and steps() == 0
    assert ray(order=None, padj=None) == 0 and steps(order=None) == 0
    assert primal(lower=-inf, upper=inf) == 0 and steps(c=0.25) == 0
    tr.cuda.synchronize(gpu)
