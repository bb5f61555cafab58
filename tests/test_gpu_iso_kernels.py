"""The two launches of include/sphrt_iso.h (csrc/loss.hip: sphrt_iso_primal_f64,
sphrt_iso_dual_f64) against the cases of tests/iso_cases.py (shown sound on the CPU by
test_iso_cpu.py), bit for bit throughout:

  shapes    pd_cases.SHAPES — one voxel, one axis, the double edge of a ring of two, edges across a
            workgroup boundary, 274 365 voxels (the grid-stride loop's second pass) — ring open
            and closed, each weight 0 in turn;
  primal    every element (a sample of the largest shape) against the header's sequence in exact
            rationals rounded once per operation, the whole volume against an op-by-op torch
            restatement on the device, and with weights (1, 1, 1) against sphrt_pd_primal_f64 on
            the same buffers;
  dual      the same two references; on exact data (Pythagorean triples scaled by powers of two,
            both sides of nrm > radius and the tie) against Fractions; the ball
            sum q^2 <= radius^2 (1 + 12 u) in Fractions on random data;
  specials  signed zeros, denormals, infinities and NaN in each operand: NaN stays NaN, radius 0
            stores +-0.
Every buffer a launch writes sits between 64-element NaN guards; dual slots without an edge keep
the bits they had; partial sums follow cg_cases.block_partials (`_kernel_sum`'s order)."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import cp_cases as cp
import iso_cases as ic
import loop_cases as lc
import pd_cases as pc
from test_gpu_fista_kernels import _Buf, _same

pytestmark = pytest.mark.gpu
CASES = ic.kernel_cases()
IDS = [f'{"x".join(map(str, s))}-{"ring" if w else "open"}-{"".join(str(int(v > 0)) for v in wt)}'
       for s, w, wt in CASES]


def _lib(gpu):
    from sph_raytracer_amd import _lib
    return _lib, _lib.load(), _lib.stream_of(gpu)


def _primal(gpu, shape, wrap, weights, x, g, q, c_damp, tau, lower, upper, pd_has=None):
    """sphrt_iso_primal_f64 (or, with pd_has, sphrt_pd_primal_f64) -> (x_new, part_mm)."""
    L, lib, st = _lib(gpu)
    n = math.prod(shape)
    bx, bg, bq = _Buf(x, gpu), _Buf(g, gpu), _Buf(q.reshape(-1), gpu)
    bn, mm, bt = _Buf(n, gpu), _Buf(lc.grid_of(n), gpu), _Buf(np.array([tau]), gpu)
    assert lib.sphrt_loss_partials(n) == lc.grid_of(n)
    if pd_has is None:
        L.check(lib.sphrt_iso_primal_f64(bx.ptr(), bg.ptr(), bq.ptr(), bn.ptr(), *shape, int(wrap),
                                         *weights, c_damp, bt.ptr(), lower, upper, mm.ptr(), st),
                'iso primal')
    else:
        L.check(lib.sphrt_pd_primal_f64(bx.ptr(), bg.ptr(), bq.ptr(), bn.ptr(), *shape, int(wrap),
                                        *pd_has, c_damp, bt.ptr(), lower, upper, mm.ptr(), st),
                'pd primal')
    assert all(b.guards_ok() for b in (bx, bg, bq, bn, mm, bt))
    assert _same(bx.host(), x) and _same(bg.host(), g) and _same(bq.host(), q.reshape(-1))
    assert _same(bt.host(), [tau])
    return bn.host(), mm.host()


def _dual(gpu, shape, wrap, weights, x_new, x_old, q, radius, sigma):
    L, lib, st = _lib(gpu)
    n = math.prod(shape)
    bn, bo, bq = _Buf(x_new, gpu), _Buf(x_old, gpu), _Buf(q.reshape(-1), gpu)
    qq, bs = _Buf(lc.grid_of(n), gpu), _Buf(np.array([sigma]), gpu)
    L.check(lib.sphrt_iso_dual_f64(bn.ptr(), bo.ptr(), bq.ptr(), *shape, int(wrap), *weights,
                                   radius, bs.ptr(), qq.ptr(), st), 'iso dual')
    assert all(b.guards_ok() for b in (bn, bo, bq, qq, bs))
    assert _same(bn.host(), x_new) and _same(bo.host(), x_old) and _same(bs.host(), [sigma])
    return bq.host().reshape(3, n), qq.host()


def _indices(n, seed):
    return np.arange(n) if n <= 600 else cc.sample(n, seed)


def _dev(v, gpu):
    return tr.from_numpy(np.ascontiguousarray(v)).to(gpu)


def _torch_primal(gpu, x, g, q, lo, up, weights, c_damp, tau, lower, upper):
    """The primal launch op by op in torch on the device (cp_cases.fma_eft for every fma)."""
    xd, gd, qd = _dev(x, gpu), _dev(g, gpu), _dev(q, gpu)
    full = lambda v: tr.full_like(xd, float(v))          # noqa: E731
    gp = cp.fma_eft(full(c_damp), xd, gd)
    s = tr.zeros_like(xd)
    for ax in range(3):
        m = _dev(lo[ax] >= 0, gpu)
        if bool(m.any()):
            src = _dev(lo[ax][lo[ax] >= 0], gpu)
            s[m] = cp.fma_eft(full(weights[ax])[m], qd[ax][src], s[m])
        m = _dev(up[ax] >= 0, gpu)
        if bool(m.any()):
            s[m] = cp.fma_eft(full(-weights[ax])[m], qd[ax][m], s[m])
    u = cp.fma_eft(full(-tau), gp + s, xd)
    lo_t, hi_t = full(lower), full(upper)
    xn = tr.where(u < lo_t, lo_t, tr.where(u > hi_t, hi_t, u))
    return xn.cpu().numpy()


def _torch_dual(gpu, x_new, x_old, q, up, weights, radius, sigma):
    """The dual launch op by op in torch on the device -> (q_new (3, n), the voxels' terms)."""
    xn, xo, qd = _dev(x_new, gpu), _dev(x_old, gpu), _dev(q, gpu)
    xb = cp.fma_eft(tr.full_like(xn, 2.0), xn, -xo)
    v, n2 = qd.clone(), tr.zeros_like(xn)
    for ax in range(3):
        m = _dev(up[ax] >= 0, gpu)
        if not bool(m.any()):
            continue
        j = _dev(up[ax][up[ax] >= 0], gpu)
        e = weights[ax] * (xb[j] - xb[m])
        v[ax][m] = cp.fma_eft(tr.full_like(e, float(sigma)), e, qd[ax][m])
        n2[m] = n2[m] + v[ax][m] * v[ax][m]
    nrm = tr.sqrt(n2)
    outside = nrm > radius
    # (tensor / tensor: a Python scalar over a tensor goes through the reciprocal, two roundings)
    scale = tr.full_like(nrm, float(radius)) / nrm
    out, t = qd.clone(), tr.zeros_like(xn)
    for ax in range(3):
        m = _dev(up[ax] >= 0, gpu)
        if not bool(m.any()):
            continue
        qn = tr.where(outside[m], v[ax][m] * scale[m], v[ax][m])
        out[ax][m] = qn
        d = qn - qd[ax][m]
        t[m] = t[m] + d * d
    return out.cpu().numpy(), t.cpu().numpy()


@pytest.mark.parametrize('shape,wrap,weights', CASES, ids=IDS)
def test_primal_against_the_sequence_and_the_restatement(shape, wrap, weights, gpu):
    n = math.prod(shape)
    lo, up = pc.neighbours(shape, wrap, ic.has_of(weights, shape))
    x, g, q, _, _ = pc.random_vectors(shape, seed=n)
    tau, lower, upper, _, _ = pc.random_scalars(n)
    idx = _indices(n, seed=n)
    for c_damp in pc.RANDOM_C_DAMP:
        got, mm = _primal(gpu, shape, wrap, weights, x, g, q, c_damp, tau, lower, upper)
        want = [ic.primal_ref(i, x, g, q, lo, up, weights, c_damp, tau, lower, upper)[0] for i in idx]
        assert _same(got[idx], want), c_damp
        whole = _torch_primal(gpu, x, g, q, lo, up, weights, c_damp, tau, lower, upper)
        assert _same(got, whole), (c_damp, np.flatnonzero(got != whole)[:4])
        assert _same(mm, cc.block_partials((got - x) ** 2)), c_damp


@pytest.mark.parametrize('shape,wrap', [(s, w) for s, ws in pc.SHAPES for w in ws],
                         ids=[f'{"x".join(map(str, s))}-{"ring" if w else "open"}'
                              for s, ws in pc.SHAPES for w in ws])
def test_primal_with_unit_weights_is_the_pd_entry_bit_for_bit(shape, wrap, gpu):
    n = math.prod(shape)
    x, g, q, _, _ = pc.random_vectors(shape, seed=n + 1)
    tau, lower, upper, _, _ = pc.random_scalars(n)
    for c_damp, lo_b, hi_b in ((0.3, lower, upper), (0.0, -math.inf, math.inf)):
        a, mm_a = _primal(gpu, shape, wrap, (1.0, 1.0, 1.0), x, g, q, c_damp, tau, lo_b, hi_b)
        b, mm_b = _primal(gpu, shape, wrap, None, x, g, q, c_damp, tau, lo_b, hi_b, pd_has=(1, 1, 1))
        assert _same(a, b) and _same(mm_a, mm_b)


@pytest.mark.parametrize('shape,wrap,weights', CASES, ids=IDS)
def test_dual_against_the_sequence_the_restatement_and_the_ball(shape, wrap, weights, gpu):
    n = math.prod(shape)
    _, up = pc.neighbours(shape, wrap, ic.has_of(weights, shape))
    _, _, q, xn, xo = pc.random_vectors(shape, seed=n)
    sigma = pc.random_scalars(n)[3]
    idx = _indices(n, seed=n)
    sides = set()
    for radius in (1.3, 0.4, 0.0):
        got, qq = _dual(gpu, shape, wrap, weights, xn, xo, q, radius, sigma)
        for i in idx:
            want, _ = ic.dual_ref(i, xn, xo, q, up, weights, radius, sigma)
            for ax in range(3):
                assert lc.same_or_both_nan(got[ax][i], q[ax][i] if want[ax] is None else want[ax]), \
                    (radius, i, ax)
        whole, terms = _torch_dual(gpu, xn, xo, q, up, weights, radius, sigma)
        assert _same(got, whole), (radius, np.argwhere(got != whole)[:4])
        for ax in range(3):
            m = up[ax] >= 0
            assert _same(got[ax][~m], q[ax][~m])                  # (no edge: untouched)
        assert _same(qq, cc.block_partials(terms)), radius
        assert _same(qq, cc.block_partials(pc.dual_terms(got, q, up))), radius
        if radius == 0.0:
            assert not got[up >= 0].any()                         # +-0
            continue
        # the ball, in Fractions (every voxel of the small shapes, a sample of the largest)
        sub = np.asarray(idx)
        excess = ic.ball_excess(got[:, sub], up[:, sub], radius)
        print(f'{shape} {wrap} {weights} radius {radius}: sum q^2 / r^2 - 1 = '
              f'{float((excess - 1) * 2 ** 53):.3g} u')
        assert excess <= ic.BALL
        nrm = np.sqrt(sum(np.where(up[ax] >= 0, got[ax], 0.0) ** 2 for ax in range(3)))
        sides |= {bool(v) for v in (nrm < 0.999 * radius)[(up >= 0).any(axis=0)]}
    if n >= 63:
        assert sides == {False, True}                             # (both branches taken)


@pytest.mark.parametrize('shape,wrap,weights', [c for c in CASES if math.prod(c[0]) <= 600], ids=[
    i for i, c in zip(IDS, CASES) if math.prod(c[0]) <= 600])
def test_dual_on_exact_data(shape, wrap, weights, gpu):
    n = math.prod(shape)
    _, up = pc.neighbours(shape, wrap, ic.has_of(weights, shape))
    seen = set()
    for seed in range(4):
        xn, xo, q, sigma, radius, want, side = ic.exact_dual_case(shape, wrap, weights, seed)
        got, qq = _dual(gpu, shape, wrap, weights, xn, xo, q, radius, sigma)
        assert _same(got, want), (seed, np.argwhere(got != want)[:4])
        assert _same(qq, cc.block_partials(pc.dual_terms(want, q, up)))
        assert ic.ball_excess(got, up, radius) <= 1                # exactly feasible here
        seen |= set(side[(up >= 0).any(axis=0)].tolist())
    assert n < 63 or seen == {-1, 0, 1}


def test_special_values(gpu):
    shape, weights, n = pc.SPECIAL_SHAPE, (1.0, 0.5, 2.0), 315
    (x, g, q, xn, xo), where = pc.special_vectors(seed=9)
    for wrap in (False, True):
        lo, up = pc.neighbours(shape, wrap, (1, 1, 1))
        for lower, upper in pc.SPECIAL_BOUNDS:
            got, mm = _primal(gpu, shape, wrap, weights, x, g, q, 0.375, 0.3, lower, upper)
            want = [ic.primal_ref(i, x, g, q, lo, up, weights, 0.375, 0.3, lower, upper)
                    for i in range(n)]
            assert _same(got, [w[0] for w in want]), (wrap, lower, upper)
            with np.errstate(all='ignore'):
                assert _same(mm, cc.block_partials([w[1] for w in want]))
            assert np.isnan(got[where]).any()
        for radius in (0.9, 0.0, 1e308, 5e-324):
            for sigma in (0.3, 0.0):
                got, qq = _dual(gpu, shape, wrap, weights, xn, xo, q, radius, sigma)
                want = [ic.dual_ref(i, xn, xo, q, up, weights, radius, sigma) for i in range(n)]
                for ax in range(3):
                    col = [q[ax][i] if w[0][ax] is None else w[0][ax] for i, w in enumerate(want)]
                    assert _same(got[ax], col), (wrap, radius, sigma, ax)
                with np.errstate(all='ignore'):
                    assert _same(qq, cc.block_partials([w[1] for w in want]))
                assert np.isnan(got).any()                         # (a NaN stays NaN)
                if radius == 0.0:
                    # +-0 at every voxel whose triple holds no NaN (a NaN norm fails the
                    # compare, and the voxel's other slots then store v)
                    clean = ~(np.isnan(got) & (up >= 0)).any(axis=0)
                    assert not got[:, clean][up[:, clean] >= 0].any() and clean.sum() > 200


def test_refusals_leave_every_buffer_untouched(gpu):
    L, lib, st = _lib(gpu)
    shape, n = (5, 7, 9), 315
    xv, gv, qv, _, xov = pc.exact_vectors(shape, seed=1)
    x, g, xo, q = _Buf(xv, gpu), _Buf(gv, gpu), _Buf(xov, gpu), _Buf(qv.reshape(-1), gpu)
    xn, mm, qq = _Buf(n, gpu), _Buf(2, gpu), _Buf(2, gpu)
    tau = _Buf(np.array([0.25]), gpu)
    nan, inf = float('nan'), float('inf')

    def primal(x=x.ptr(), g=g.ptr(), q=q.ptr(), xn=xn.ptr(), shape=shape, ws=(1.0, 0.5, 2.0),
               tau=tau.ptr(), lower=0.0, upper=1.0, mm=mm.ptr()):
        return lib.sphrt_iso_primal_f64(x, g, q, xn, *shape, 1, *ws, 0.5, tau, lower, upper, mm, st)

    def dual(a=x.ptr(), b=xo.ptr(), q=q.ptr(), shape=shape, ws=(1.0, 0.5, 2.0), radius=1.0,
             sigma=tau.ptr(), qq=qq.ptr()):
        return lib.sphrt_iso_dual_f64(a, b, q, *shape, 1, *ws, radius, sigma, qq, st)

    cases = []
    for fn in (primal, dual):
        cases += [(fn, dict(shape=s), b'axis') for s in ((0, 7, 9), (5, -1, 9), (5, 7, 0))]
        cases += [(fn, dict(shape=(2 ** 11, 2 ** 10, 2 ** 10)), b'2^31')]
        cases += [(fn, dict(ws=ws), b'weights') for ws in ((nan, 1.0, 1.0), (1.0, -1.0, 1.0),
                                                          (1.0, 1.0, inf))]
    cases += [(primal, {k: None}, b'null') for k in ('x', 'g', 'q', 'xn', 'tau', 'mm')]
    cases += [(dual, {k: None}, b'null') for k in ('a', 'b', 'q', 'sigma', 'qq')]
    cases += [(primal, dict(xn=x.ptr()), b'alias'), (primal, dict(xn=q.ptr()), b'alias'),
              (primal, dict(mm=tau.ptr()), b'alias'), (dual, dict(q=x.ptr()), b'alias'),
              (dual, dict(b=x.ptr()), b'alias'), (dual, dict(qq=q.ptr()), b'alias'),
              (primal, dict(lower=nan), b'bound'), (primal, dict(lower=1.0), b'bound')]
    cases += [(dual, dict(radius=v), b'radius') for v in (nan, -1.0, inf)]
    for i, (fn, kw, word) in enumerate(cases):
        assert fn(**kw) != 0, (i, fn.__name__, kw)
        assert word in lib.sphrt_last_error(), (i, fn.__name__, kw, lib.sphrt_last_error())
    tr.cuda.synchronize(gpu)
    assert all(bool(tr.isnan(b.view).all()) for b in (xn, mm, qq)) and _same(q.host(), qv.reshape(-1))
    assert primal() == 0 and dual() == 0
    tr.cuda.synchronize(gpu)
