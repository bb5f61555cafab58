"""The two primal-dual kernels (csrc/loss.hip: sphrt_pd_primal_f64, sphrt_pd_dual_f64, declared in
include/sphrt_pd.h) against the cases of tests/pd_cases.py (shown sound on the CPU by
test_pd_cpu.py), bit for bit throughout:

  exact     every shape of pd_cases.kernel_cases — one voxel, one axis, the double edge of a ring
            of two, edges across a workgroup boundary, the grid-stride loop's second element —
            with the wrap on and off and each axis off in turn: every element and every
            workgroup's partial sum against integer arithmetic;
  random    the element sequences against exact rationals rounded once per operation (every
            element of the small shapes, a sample of the largest), the partial sums against the
            documented workgroup order;
  specials  signed zeros, denormals, infinities and NaN in each operand, infinite bounds;
  refusals  on the host: nothing is launched, the outputs keep their fill.
Every buffer a launch writes sits between 64-element NaN guards; dual slots without an edge keep
the bits they had."""
import ctypes
import math

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import loop_cases as lc
import pd_cases as pc
from test_gpu_fista_kernels import _Buf, _same

pytestmark = pytest.mark.gpu
CASES = pc.kernel_cases()
IDS = [f'{"x".join(map(str, s))}-{"ring" if w else "open"}-{"".join(map(str, h))}' for s, w, h in CASES]


def _lib(gpu):
    from sph_raytracer_amd import _lib
    return _lib, _lib.load(), _lib.stream_of(gpu)


def _primal(gpu, shape, wrap, has, x, g, q, c_damp, tau, lower, upper):
    L, lib, st = _lib(gpu)
    n = math.prod(shape)
    bx, bg, bq = _Buf(x, gpu), _Buf(g, gpu), _Buf(q.reshape(-1), gpu)
    bn, mm, bt = _Buf(n, gpu), _Buf(lc.grid_of(n), gpu), _Buf(np.array([tau]), gpu)
    assert lib.sphrt_loss_partials(n) == lc.grid_of(n)
    L.check(lib.sphrt_pd_primal_f64(bx.ptr(), bg.ptr(), bq.ptr(), bn.ptr(), *shape, int(wrap), *has,
                                    c_damp, bt.ptr(), lower, upper, mm.ptr(), st), 'primal')
    assert all(b.guards_ok() for b in (bx, bg, bq, bn, mm, bt))
    assert _same(bx.host(), x) and _same(bg.host(), g) and _same(bq.host(), q.reshape(-1))
    assert _same(bt.host(), [tau])
    return bn.host(), mm.host()


def _dual(gpu, shape, wrap, has, x_new, x_old, q, sigma, cax):
    L, lib, st = _lib(gpu)
    n = math.prod(shape)
    bn, bo, bq = _Buf(x_new, gpu), _Buf(x_old, gpu), _Buf(q.reshape(-1), gpu)
    qq, bs = _Buf(lc.grid_of(n), gpu), _Buf(np.array([sigma]), gpu)
    L.check(lib.sphrt_pd_dual_f64(bn.ptr(), bo.ptr(), bq.ptr(), *shape, int(wrap), *has, *cax,
                                  bs.ptr(), qq.ptr(), st), 'dual')
    assert all(b.guards_ok() for b in (bn, bo, bq, qq, bs))
    assert _same(bn.host(), x_new) and _same(bo.host(), x_old) and _same(bs.host(), [sigma])
    return bq.host().reshape(3, n), qq.host()


def _indices(n, seed):
    return np.arange(n) if n <= 600 else cc.sample(n, seed)


# ---- exact cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,wrap,has', CASES, ids=IDS)
def test_exact_cases(shape, wrap, has, gpu):
    n = math.prod(shape)
    lo, up = pc.neighbours(shape, wrap, has)
    x, g, q, xn, xo = pc.exact_vectors(shape, seed=7 * n)
    for case in pc.EXACT_PRIMAL:
        want, want_mm, _ = pc.exact_primal(x, g, q, lo, up, *case)
        got, mm = _primal(gpu, shape, wrap, has, x, g, q, *(a / b for a, b in case))
        assert _same(got, want), (case, np.flatnonzero(got != want)[:4])
        assert _same(mm, want_mm), (case, np.flatnonzero(mm != want_mm)[:4])
    for case in pc.EXACT_DUAL:
        want, want_qq, _ = pc.exact_dual(xn, xo, q, up, case[0], case[1:])
        got, qq = _dual(gpu, shape, wrap, has, xn, xo, q, case[0][0] / case[0][1],
                        [a / b for a, b in case[1:]])
        assert _same(got, want), (case, np.argwhere(got != want)[:4])
        assert _same(qq, want_qq), (case, np.flatnonzero(qq != want_qq)[:4])


# ---- random cases --------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,wrap,has', CASES, ids=IDS)
def test_random_cases(shape, wrap, has, gpu):
    n = math.prod(shape)
    lo, up = pc.neighbours(shape, wrap, has)
    x, g, q, xn, xo = pc.random_vectors(shape, seed=n)
    tau, lower, upper, sigma, cax = pc.random_scalars(n)
    idx = _indices(n, seed=n)
    s = pc.adjoint_sum(q, lo, up)
    for c_damp in pc.RANDOM_C_DAMP:
        got, mm = _primal(gpu, shape, wrap, has, x, g, q, c_damp, tau, lower, upper)
        want = [pc.primal_ref(i, x, g, q, lo, up, c_damp, tau, lower, upper)[0] for i in idx]
        assert _same(got[idx], want), c_damp
        # elsewhere: the same step at every voxel (within the two forms' distance of numpy's)
        plain = np.clip(x - tau * ((c_damp * x + g) + s), lower, upper)
        assert np.all(np.abs(got - plain) <= 4 * np.spacing(np.abs(x) + tau * (np.abs(g) + np.abs(s) + 1)))
        assert _same(mm, cc.block_partials((got - x) ** 2)), c_damp
    got, qq = _dual(gpu, shape, wrap, has, xn, xo, q, sigma, cax)
    for i in idx:
        want, _ = pc.dual_ref(i, xn, xo, q, up, sigma, cax)
        for ax in range(3):
            assert lc.same_or_both_nan(got[ax][i], q[ax][i] if want[ax] is None else want[ax]), (i, ax)
    xb = 2 * xn - xo
    for ax in range(3):
        m = up[ax] >= 0
        assert _same(got[ax][~m], q[ax][~m])                  # (no edge: untouched)
        plain = np.clip(q[ax][m] + sigma * (xb[up[ax][m]] - xb[m]), -cax[ax], cax[ax])
        assert np.all(np.abs(got[ax][m] - plain) <= 4 * np.spacing(np.abs(q[ax][m]) + 4.0))
    assert _same(qq, cc.block_partials(pc.dual_terms(got, q, up)))


# ---- special values ------------------------------------------------------------------------------------
@pytest.mark.parametrize('lower,upper', pc.SPECIAL_BOUNDS)
def test_special_elements_follow_the_documented_sequence(lower, upper, gpu):
    shape, has, n = pc.SPECIAL_SHAPE, (1, 1, 1), 315
    (x, g, q, xn, xo), where = pc.special_vectors(seed=9)
    for wrap in (False, True):
        lo, up = pc.neighbours(shape, wrap, has)
        for c_damp, tau in ((0.375, 0.3), (0.0, 0.3), (0.25, 0.0)):
            got, mm = _primal(gpu, shape, wrap, has, x, g, q, c_damp, tau, lower, upper)
            want = [pc.primal_ref(i, x, g, q, lo, up, c_damp, tau, lower, upper) for i in range(n)]
            assert _same(got, [w[0] for w in want]), (wrap, c_damp, tau)
            with np.errstate(all='ignore'):
                assert _same(mm, cc.block_partials([w[1] for w in want])), (wrap, c_damp, tau)
            assert np.isnan(got[where]).any()             # (a NaN stays NaN through the clamp)
            ok = ~np.isnan(got)
            assert np.all((got[ok] >= lower) & (got[ok] <= upper))
        for cax in pc.SPECIAL_C:
            for sigma in (0.3, 0.0):
                got, qq = _dual(gpu, shape, wrap, has, xn, xo, q, sigma, cax)
                want = [pc.dual_ref(i, xn, xo, q, up, sigma, cax) for i in range(n)]
                for ax in range(3):
                    col = [q[ax][i] if w[0][ax] is None else w[0][ax] for i, w in enumerate(want)]
                    assert _same(got[ax], col), (wrap, cax, sigma, ax)
                with np.errstate(all='ignore'):
                    assert _same(qq, cc.block_partials([w[1] for w in want])), (wrap, cax, sigma)
                assert np.isnan(got).any()
                for ax in range(3):
                    v = got[ax][(up[ax] >= 0) & ~np.isnan(got[ax])]
                    assert np.all(np.abs(v) <= cax[ax])


# ---- refusals ------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_untouched(gpu):
    """Each refusal returns non-zero with its word in sphrt_last_error and launches nothing: the
    outputs keep their NaN fill and q its values."""
    L, lib, st = _lib(gpu)
    shape, n = (5, 7, 9), 315
    xv, gv, qv, _, xov = pc.exact_vectors(shape, seed=1)
    x, g, xo, q = _Buf(xv, gpu), _Buf(gv, gpu), _Buf(xov, gpu), _Buf(qv.reshape(-1), gpu)
    xn, mm, qq = _Buf(n, gpu), _Buf(2, gpu), _Buf(2, gpu)
    tau = _Buf(np.array([0.25]), gpu)
    nan, inf = float('nan'), float('inf')

    def primal(x=x.ptr(), g=g.ptr(), q=q.ptr(), xn=xn.ptr(), shape=shape, tau=tau.ptr(), lower=0.0,
               upper=1.0, mm=mm.ptr()):
        return lib.sphrt_pd_primal_f64(x, g, q, xn, *shape, 1, 1, 1, 1, 0.5, tau, lower, upper, mm, st)

    def dual(a=x.ptr(), b=xo.ptr(), q=q.ptr(), shape=shape, cs=(1.0, 0.0, 2.0), sigma=tau.ptr(),
             qq=qq.ptr()):
        return lib.sphrt_pd_dual_f64(a, b, q, *shape, 1, 1, 1, 1, *cs, sigma, qq, st)

    cases = []
    for fn in (primal, dual):
        cases += [(fn, dict(shape=s), b'axis') for s in ((0, 7, 9), (5, -1, 9), (5, 7, 0))]
        cases += [(fn, dict(shape=(2 ** 11, 2 ** 10, 2 ** 10)), b'2^31')]
    cases += [(primal, {k: None}, b'null') for k in ('x', 'g', 'q', 'xn', 'tau', 'mm')]
    cases += [(dual, {k: None}, b'null') for k in ('a', 'b', 'q', 'sigma', 'qq')]
    cases += [(primal, dict(xn=x.ptr()), b'alias'), (primal, dict(xn=g.ptr()), b'alias'),
              (primal, dict(xn=q.ptr()), b'alias'), (primal, dict(g=x.ptr()), b'alias'),
              (primal, dict(xn=ctypes.c_void_p(q.ptr().value + 8 * (3 * n - 1))), b'alias'),
              (primal, dict(mm=tau.ptr()), b'alias'),
              (dual, dict(q=x.ptr()), b'alias'), (dual, dict(b=x.ptr()), b'alias'),
              (dual, dict(a=ctypes.c_void_p(q.ptr().value + 8 * 2 * n)), b'alias'),
              (dual, dict(qq=q.ptr()), b'alias'),
              (primal, dict(lower=nan), b'bound'), (primal, dict(upper=nan), b'bound'),
              (primal, dict(lower=1.0), b'bound'), (primal, dict(lower=2.0), b'bound'),
              (primal, dict(lower=inf, upper=inf), b'bound'),
              (primal, dict(lower=-inf, upper=-inf), b'bound')]
    cases += [(dual, dict(cs=cs), b'c_ax') for cs in ((nan, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, inf))]
    for i, (fn, kw, word) in enumerate(cases):
        assert fn(**kw) != 0, (i, fn.__name__, kw)
        assert word in lib.sphrt_last_error(), (i, fn.__name__, kw, lib.sphrt_last_error())
    tr.cuda.synchronize(gpu)
    assert all(bool(tr.isnan(b.view).all()) for b in (xn, mm, qq)) and _same(q.host(), qv.reshape(-1))
    # and the same arguments unchanged are accepted
    assert primal() == 0 and dual() == 0
    assert primal(lower=-inf, upper=inf) == 0 and primal(lower=0.0, upper=inf) == 0
    tr.cuda.synchronize(gpu)
