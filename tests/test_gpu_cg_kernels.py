"""The three conjugate-gradient kernels (csrc/loss.hip: sphrt_cg_curvature_f64,
sphrt_cg_update_f64, sphrt_cg_direction_f64) against the cases of tests/cg_cases.py (shown sound
on the CPU by test_cg_cpu.py), bit for bit throughout:

  exact     every length of LENGTHS (one to four elements per thread, one to 1024 partial sums),
            every element and every workgroup's partial sum against integer arithmetic, alpha and
            beta dyadic rationals from integer partial sums;
  random    alpha and beta from the documented summation order restated in numpy, a sample of
            elements against the exact-rational fma, the partial sums against the documented
            workgroup order over the launch's own output;
  guards    PHP of 0, negative and NaN, RR of 0 and NaN, a quotient that overflows, the freeze
            threshold reached, met exactly, not reached, NaN and NULL;
  specials  signed zeros, denormals, overflow, infinities and NaN through the documented
            operation sequence, with alpha and beta non-zero and zero.
Every buffer a launch writes sits between 64-element NaN guards."""
import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import loop_cases as lc

pytestmark = pytest.mark.gpu
GUARD = cc.GUARD


def _lib(gpu):
    from sph_raytracer_amd import _lib
    return _lib, _lib.load(), _lib.stream_of(gpu)


class _Buf:
    """A float64 device buffer between NaN guards."""

    def __init__(self, values, gpu):
        n = values if isinstance(values, int) else len(values)
        self.whole = tr.full((n + 2 * GUARD,), float('nan'), dtype=tr.float64, device=gpu)
        self.view = self.whole[GUARD:GUARD + n]
        if not isinstance(values, int):
            self.view.copy_(tr.from_numpy(np.ascontiguousarray(values, dtype=np.float64)))

    def ptr(self):
        from sph_raytracer_amd import _lib
        return _lib.ptr(self.view)

    def host(self):
        return self.view.cpu().numpy()

    def guards_ok(self):
        return bool(tr.isnan(self.whole[:GUARD]).all()) and bool(tr.isnan(self.whole[-GUARD:]).all())


def _same(a, b):
    """Bit for bit, NaN at the same places (payloads not compared)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(np.where(na, 0, a).view(np.int64), np.where(nb, 0, b).view(np.int64))


def _curvature(gpu, p, h, c_damp):
    L, lib, st = _lib(gpu)
    n = len(p)
    bp, bh, part = _Buf(p, gpu), _Buf(h, gpu), _Buf(lc.grid_of(n), gpu)
    assert lib.sphrt_loss_partials(n) == lc.grid_of(n)
    L.check(lib.sphrt_cg_curvature_f64(bp.ptr(), bh.ptr(), n, c_damp, part.ptr(), st), 'curvature')
    assert bh.guards_ok() and part.guards_ok() and _same(bp.host(), p)
    return bh.host(), part.host()


def _update(gpu, x, r, p, h, part_rr, part_php, rr_stop):
    L, lib, st = _lib(gpu)
    n = len(x)
    bx, br, bp, bh = (_Buf(v, gpu) for v in (x, r, p, h))
    rr, php, out = _Buf(part_rr, gpu), _Buf(part_php, gpu), _Buf(lc.grid_of(n), gpu)
    stop = _Buf(np.array([rr_stop]), gpu) if rr_stop is not None else None
    L.check(lib.sphrt_cg_update_f64(bx.ptr(), br.ptr(), bp.ptr(), bh.ptr(), n, rr.ptr(), php.ptr(),
                                    len(part_rr), stop.ptr() if stop else None, out.ptr(), st),
            'update')
    assert all(b.guards_ok() for b in (bx, br, out))
    assert _same(bp.host(), p) and _same(bh.host(), h) and _same(rr.host(), part_rr)
    return bx.host(), br.host(), out.host()


def _direction(gpu, p, r, part_new, part_old, rr_stop):
    L, lib, st = _lib(gpu)
    n = len(p)
    bp, br = _Buf(p, gpu), _Buf(r, gpu)
    new, old = _Buf(part_new, gpu), _Buf(part_old, gpu)
    stop = _Buf(np.array([rr_stop]), gpu) if rr_stop is not None else None
    L.check(lib.sphrt_cg_direction_f64(bp.ptr(), br.ptr(), n, new.ptr(), old.ptr(), len(part_new),
                                       stop.ptr() if stop else None, st), 'direction')
    assert bp.guards_ok() and _same(br.host(), r)
    return bp.host()


# ---- exact cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n', cc.LENGTHS)
def test_exact_cases(n, gpu):
    x, r, p, h = cc.exact_vectors(n, seed=7 * n)
    for num, den in cc.DYADIC:
        ctx = f'n={n} {num}/{den}'
        top, bot = cc.dyadic_partials(n, num, den, seed=n + num)
        hn, php = _curvature(gpu, p, h, num / den)
        want_h, want_php = cc.exact_curvature(p, h, num, den)
        assert _same(hn, want_h) and _same(php, want_php), ctx
        xn, rn, part = _update(gpu, x, r, p, h, top, bot, None)
        want_x, want_r, want_part = cc.exact_update(x, r, p, h, num, den)
        assert _same(xn, want_x) and _same(rn, want_r), ctx
        assert _same(part, want_part), (ctx, np.flatnonzero(part != want_part)[:4])
        assert _same(_direction(gpu, p, r, top, bot, None), cc.exact_direction(p, r, num, den)), ctx


# ---- random cases --------------------------------------------------------------------------------
@pytest.mark.parametrize('n', cc.LENGTHS)
def test_random_cases(n, gpu):
    x, r, p, h = cc.random_vectors(n, seed=n)
    rr, php = cc.random_partials(n, seed=n)
    idx = cc.sample(n, seed=n)
    alpha = cc.alpha_ref(cc.kernel_sum(rr), cc.kernel_sum(php), None)
    assert alpha > 0
    xn, rn, part = _update(gpu, x, r, p, h, rr, php, None)
    want = [cc.update_ref(x[i], r[i], p[i], h[i], alpha) for i in idx]
    assert _same(xn[idx], [w[0] for w in want]) and _same(rn[idx], [w[1] for w in want])
    assert _same(part, cc.block_partials(rn * rn))
    # elsewhere: the same alpha in every workgroup (within the two forms' distance of numpy's)
    assert np.all(np.abs(xn - (x + alpha * p)) <= np.spacing(np.abs(alpha * p)) + np.spacing(np.abs(xn)))
    assert np.all(np.abs(rn - (r - alpha * h)) <= np.spacing(np.abs(alpha * h)) + np.spacing(np.abs(rn)))
    beta = cc.beta_ref(cc.kernel_sum(rr), cc.kernel_sum(php), None)
    pn = _direction(gpu, p, r, rr, php, None)
    assert _same(pn[idx], [cc.fma(beta, p[i], r[i]) for i in idx])
    assert np.all(np.abs(pn - (beta * p + r)) <= np.spacing(np.abs(beta * p)) + np.spacing(np.abs(pn)))
    c_damp = 0.3 + 1e-3 * (n % 7)
    hn, pph = _curvature(gpu, p, h, c_damp)
    assert _same(hn[idx], [cc.fma(c_damp, p[i], h[i]) for i in idx])
    assert _same(pph, cc.block_partials(p * hn))


# ---- the scalar guards and the freeze ------------------------------------------------------------
INF, NAN = cc.INF, cc.NAN
# (RR, PHP, rr_stop): one value in the first partial, zeros in the second (n = 257: two partials)
UPDATE_GUARDS = [
    (2.0, 8.0, None), (2.0, 8.0, 1.0), (2.0, 8.0, 2.0), (2.0, 8.0, 3.0), (2.0, 8.0, NAN),
    (2.0, 8.0, 0.0), (2.0, 0.0, None), (2.0, -0.0, None), (2.0, -8.0, None), (2.0, NAN, None),
    (2.0, -INF, None), (2.0, INF, None), (0.0, 8.0, None), (0.0, 0.0, None), (0.0, 8.0, 0.0),
    (NAN, 8.0, None), (NAN, 8.0, 1.0), (INF, 8.0, None), (1e308, 1e-308, None), (5e-324, 8.0, None),
]
DIRECTION_GUARDS = [
    (1.0, 4.0, None), (1.0, 4.0, 3.0), (1.0, 4.0, 4.0), (1.0, 4.0, 5.0), (1.0, 4.0, NAN),
    (1.0, 0.0, None), (1.0, -0.0, None), (1.0, -4.0, None), (1.0, NAN, None), (0.0, 4.0, None),
    (0.0, 0.0, 0.0), (NAN, 4.0, None), (INF, 4.0, None), (1.0, INF, None), (1e308, 1e-308, None),
]


def _two(v, second_slot):
    """Two partial sums holding v: in the first slot or in the second."""
    return np.array([0.0, v]) if second_slot else np.array([v, 0.0])


@pytest.mark.parametrize('second_slot', [False, True])
def test_update_guards(second_slot, gpu):
    n = 257
    x, r, p, h = cc.exact_vectors(n, seed=5)
    for rr, php, stop in UPDATE_GUARDS:
        ctx = (rr, php, stop)
        alpha = cc.alpha_ref(cc.kernel_sum(_two(rr, second_slot)),
                             cc.kernel_sum(_two(php, not second_slot)), stop)
        xn, rn, part = _update(gpu, x, r, p, h, _two(rr, second_slot), _two(php, not second_slot),
                               stop)
        want = [cc.update_ref(x[i], r[i], p[i], h[i], alpha) for i in range(n)]
        assert _same(xn, [w[0] for w in want]) and _same(rn, [w[1] for w in want]), ctx
        assert _same(part, cc.block_partials(rn * rn)), ctx
        if alpha == 0.0:      # frozen or guarded: nothing moves
            assert _same(xn, x) and _same(rn, r), ctx
    # the cases cover both outcomes
    alphas = [cc.alpha_ref(a, b, s) for a, b, s in UPDATE_GUARDS]
    assert alphas.count(0.0) >= 12 and sum(a > 0 for a in alphas) >= 4


@pytest.mark.parametrize('second_slot', [False, True])
def test_direction_guards(second_slot, gpu):
    n = 257
    _, r, p, _ = cc.exact_vectors(n, seed=6)
    for new, old, stop in DIRECTION_GUARDS:
        beta = cc.beta_ref(cc.kernel_sum(_two(new, second_slot)),
                           cc.kernel_sum(_two(old, not second_slot)), stop)
        pn = _direction(gpu, p, r, _two(new, second_slot), _two(old, not second_slot), stop)
        assert _same(pn, [cc.fma(beta, p[i], r[i]) for i in range(n)]), (new, old, stop)
        if beta == 0.0:       # the direction restarts from the residual
            assert _same(pn, r + 0.0 * p), (new, old, stop)


# ---- special values ------------------------------------------------------------------------------
def _with_specials(n, seed):
    x, r, p, h = (v.copy() for v in cc.random_vectors(n, seed))
    where = []
    for base in (3, 250, n - len(cc.SPECIAL_ELEMENTS)):      # both workgroups, the ragged end
        for j, tup in enumerate(cc.SPECIAL_ELEMENTS):
            x[base + j], r[base + j], p[base + j], h[base + j] = tup
            where.append(base + j)
    return x, r, p, h, np.array(where)


@pytest.mark.parametrize('scalar', [0.375, 0.0, 3.0])
def test_special_values_follow_the_documented_sequence(scalar, gpu):
    n = 300
    x, r, p, h, where = _with_specials(n, seed=9)
    top = np.array([3.0, 0.0]) if scalar else np.array([0.0, 0.0])
    bot = np.array([0.0, 3.0 / scalar]) if scalar else np.array([1.0, 1.0])
    assert cc.alpha_ref(cc.kernel_sum(top), cc.kernel_sum(bot), None) == scalar
    assert cc.beta_ref(cc.kernel_sum(top), cc.kernel_sum(bot), None) == scalar
    xn, rn, part = _update(gpu, x, r, p, h, top, bot, None)
    want = [cc.update_ref(x[i], r[i], p[i], h[i], scalar) for i in range(n)]
    assert _same(xn, [w[0] for w in want]) and _same(rn, [w[1] for w in want])
    with np.errstate(all='ignore'):
        assert _same(part, cc.block_partials(rn * rn))
    assert np.isnan(part).all()                       # (a NaN in each workgroup reaches its sum)
    assert np.isnan(xn[where]).any() and np.isinf(xn[where]).any()
    assert _same(_direction(gpu, p, r, top, bot, None),
                 [cc.fma(scalar, p[i], r[i]) for i in range(n)])
    hn, php = _curvature(gpu, p, h, scalar)
    assert _same(hn, [cc.fma(scalar, p[i], h[i]) for i in range(n)])
    with np.errstate(all='ignore'):
        assert _same(php, cc.block_partials(p * hn))
    # denormals are kept (not flushed): the smallest one survives an update by itself
    assert xn[where[2]] == cc.fma(scalar, 5e-324, 5e-324) > 0
