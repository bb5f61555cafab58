"""The two projected-gradient kernels (csrc/loss.hip: sphrt_pg_step_f64, sphrt_pg_momentum_f64)
against the cases of tests/fista_cases.py (shown sound on the CPU by test_fista_cpu.py), bit for
bit throughout:

  exact     every length of LENGTHS, every element and every workgroup's partial sum against
            integer arithmetic, each clamp branch taken; integer rows for part_gd whose totals
            are > 0, < 0 and exactly 0, with *j_in at the start, inside and at the end of the table;
  random    a sample of elements against the exact-rational sequence, the partial sums against
            the documented workgroup order, GD from the documented summation order;
  specials  signed zeros, denormals, infinities and NaN in each operand and in GD, infinite
            bounds;
  refusals  on the host, with a device fault behind every pointer that would be read.
Every buffer a launch writes sits between 64-element NaN guards (the int64 slots between -1s)."""
import ctypes

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import fista_cases as fc
import loop_cases as lc

pytestmark = pytest.mark.gpu
GUARD = fc.GUARD


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


def _step(gpu, z, g, x_old, c_damp, step, lower, upper):
    L, lib, st = _lib(gpu)
    n = len(z)
    bz, bg, bo = (_Buf(v, gpu) for v in (z, g, x_old))
    bn, gd, mm = _Buf(n, gpu), _Buf(lc.grid_of(n), gpu), _Buf(lc.grid_of(n), gpu)
    bs = _Buf(np.array([step]), gpu)
    assert lib.sphrt_loss_partials(n) == lc.grid_of(n)
    L.check(lib.sphrt_pg_step_f64(bz.ptr(), bg.ptr(), bo.ptr(), bn.ptr(), n, c_damp, bs.ptr(),
                                  lower, upper, gd.ptr(), mm.ptr(), st), 'step')
    assert all(b.guards_ok() for b in (bn, gd, mm))
    assert _same(bz.host(), z) and _same(bg.host(), g) and _same(bo.host(), x_old)
    assert _same(bs.host(), [step])
    return bn.host(), gd.host(), mm.host()


def _momentum(gpu, x_new, x_old, part_gd, omega, j_in):
    """-> (z, j_out); *j_in and its neighbours are checked untouched."""
    L, lib, st = _lib(gpu)
    n = len(x_new)
    bn, bo, bz = _Buf(x_new, gpu), _Buf(x_old, gpu), _Buf(n, gpu)
    gd, om = _Buf(part_gd, gpu), _Buf(omega, gpu)
    slots = tr.full((2 * GUARD + 2,), -1, dtype=tr.int64, device=gpu)
    slots[GUARD] = j_in
    L.check(lib.sphrt_pg_momentum_f64(bz.ptr(), bn.ptr(), bo.ptr(), n, gd.ptr(), len(part_gd),
                                      om.ptr(), len(omega), L.ptr(slots[GUARD:]),
                                      L.ptr(slots[GUARD + 1:]), st), 'momentum')
    assert bz.guards_ok()
    assert _same(bn.host(), x_new) and _same(bo.host(), x_old) and _same(gd.host(), part_gd)
    s = slots.cpu().numpy()
    assert s[GUARD] == j_in and np.all(s[:GUARD] == -1) and np.all(s[GUARD + 2:] == -1)
    return bz.host(), int(s[GUARD + 1])


# ---- exact cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', fc.LENGTHS)
def test_exact_cases(n, gpu):
    z, g, x_old = fc.exact_vectors(n, seed=11 * n)
    for c_damp, step, lower, upper in fc.EXACT_STEPS:
        ctx = f'n={n} {c_damp} {step} {lower} {upper}'
        want_x, want_gd, want_mm, _ = fc.exact_step(z, g, x_old, c_damp, step, lower, upper)
        xn, gd, mm = _step(gpu, z, g, x_old, *(a / b for a, b in (c_damp, step, lower, upper)))
        assert _same(xn, want_x), (ctx, np.flatnonzero(xn != want_x)[:4])
        assert _same(gd, want_gd), (ctx, np.flatnonzero(gd != want_gd)[:4])
        assert _same(mm, want_mm), (ctx, np.flatnonzero(mm != want_mm)[:4])
    x_new = z                                            # (any two exact vectors)
    for sign in (1, -1, 0):
        part = fc.gd_partials(n, sign, seed=n + sign)
        for j_in in fc.EXACT_J_IN:
            j = fc.j_ref(cc.kernel_sum(part), j_in, len(fc.EXACT_OMEGA))
            zn, j_out = _momentum(gpu, x_new, x_old, part, fc.EXACT_OMEGA, j_in)
            assert j_out == j, (n, sign, j_in)
            assert _same(zn, fc.exact_momentum(x_new, x_old, fc.EXACT_OMEGA[j])), (n, sign, j_in)


# ---- random cases --------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', fc.LENGTHS)
def test_random_cases(n, gpu):
    z, g, x_old = fc.random_vectors(n, seed=n)
    step, lower, upper = fc.random_scalars(n)
    idx = cc.sample(n, seed=n)
    for c_damp in fc.RANDOM_C_DAMP:
        xn, gd, mm = _step(gpu, z, g, x_old, c_damp, step, lower, upper)
        want = [fc.step_ref(z[i], g[i], x_old[i], c_damp, step, lower, upper)[0] for i in idx]
        assert _same(xn[idx], want), c_damp
        # elsewhere: the same step in every workgroup (within the two forms' distance of numpy's)
        plain = np.clip(z - step * (c_damp * z + g), lower, upper)
        assert np.all(np.abs(xn - plain) <= 4 * np.spacing(np.abs(z) + step * np.abs(g))), c_damp
        assert _same(mm, cc.block_partials((z - xn) ** 2)), c_damp
        if c_damp in (0.0, 0.125):        # c z is exact: numpy's c z + g is the fma
            assert _same(gd, cc.block_partials((c_damp * z + g) * (xn - x_old))), c_damp
    x_new = xn
    omega = np.random.default_rng(n).random(9)
    for sign in (1, -1):
        part = fc.random_partials(n, seed=n, sign=sign)
        j = fc.j_ref(cc.kernel_sum(part), 4, len(omega))
        assert j == (1 if sign > 0 else 5)
        zn, j_out = _momentum(gpu, x_new, x_old, part, omega, 4)
        assert j_out == j
        assert _same(zn[idx], [fc.momentum_ref(x_new[i], x_old[i], omega[j]) for i in idx])
        plain = x_new + omega[j] * (x_new - x_old)
        assert np.all(np.abs(zn - plain) <= 2 * np.spacing(np.abs(plain)) + np.spacing(np.abs(x_new)))


# ---- special values ------------------------------------------------------------------------------------
@pytest.mark.parametrize('lower,upper', fc.SPECIAL_BOUNDS)
def test_special_elements_follow_the_documented_sequence(lower, upper, gpu):
    n = 300
    z, g, x_old, where = fc.special_vectors(n, seed=9)
    for c_damp, step in ((0.375, 0.3), (0.0, 0.3), (0.25, 0.0)):
        xn, gd, mm = _step(gpu, z, g, x_old, c_damp, step, lower, upper)
        want = [fc.step_ref(z[i], g[i], x_old[i], c_damp, step, lower, upper) for i in range(n)]
        assert _same(xn, [w[0] for w in want]), (c_damp, step)
        with np.errstate(all='ignore'):
            assert _same(gd, cc.block_partials([w[1] for w in want])), (c_damp, step)
            assert _same(mm, cc.block_partials([w[2] for w in want])), (c_damp, step)
        assert np.isnan(xn[where]).any()              # (a NaN stays NaN through the clamp)
        ok = ~np.isnan(xn)
        assert np.all((xn[ok] >= lower) & (xn[ok] <= upper))
    zn, j_out = _momentum(gpu, z, x_old, np.array([-1.0, 0.0]), [0.0, 0.0, 0.375, 0.5], 1)
    assert j_out == 2
    assert _same(zn, [fc.momentum_ref(z[i], x_old[i], 0.375) for i in range(n)])


@pytest.mark.parametrize('second_slot', [False, True])
def test_special_gd(second_slot, gpu):
    n = 257
    x_new, x_old, _ = fc.exact_vectors(n, seed=5)
    omega = [0.0, 0.5, 0.25, 0.375, 0.125]
    for (a, b), restart in fc.SPECIAL_GD:
        part = np.array([b, a]) if second_slot else np.array([a, b])
        for j_in in (0, 2, 4):
            j = fc.j_ref(cc.kernel_sum(part), j_in, len(omega))
            assert (j == 1) == restart or (j_in == 0 and j == 1)
            zn, j_out = _momentum(gpu, x_new, x_old, part, omega, j_in)
            assert j_out == j, (a, b, j_in)
            assert _same(zn, fc.exact_momentum(x_new, x_old, omega[j])), (a, b, j_in)


# ---- refusals ------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_untouched(gpu):
    """Each refusal returns non-zero with its word in sphrt_last_error and launches nothing: the
    outputs keep their NaN fill."""
    L, lib, st = _lib(gpu)
    n = 300
    z, g, xo = (_Buf(v, gpu) for v in fc.exact_vectors(n, seed=1))
    xn, gd, mm = _Buf(n, gpu), _Buf(2, gpu), _Buf(2, gpu)
    step = _Buf(np.array([0.25]), gpu)
    omega = _Buf(np.array([0.0, 0.0, 0.5]), gpu)
    slots = tr.zeros(2, dtype=tr.int64, device=gpu)
    nan, inf = float('nan'), float('inf')

    def do_step(z=z.ptr(), g=g.ptr(), xo=xo.ptr(), xn=xn.ptr(), n=n, step=step.ptr(), lower=0.0,
                upper=1.0, gd=gd.ptr(), mm=mm.ptr()):
        return lib.sphrt_pg_step_f64(z, g, xo, xn, n, 0.5, step, lower, upper, gd, mm, st)

    def do_momentum(zz=xn.ptr(), a=z.ptr(), b=xo.ptr(), n=n, gd=gd.ptr(), n_part=2,
                    om=omega.ptr(), n_omega=3, j_in=L.ptr(slots), j_out=L.ptr(slots[1:])):
        return lib.sphrt_pg_momentum_f64(zz, a, b, n, gd, n_part, om, n_omega, j_in, j_out, st)

    cases = [(do_step, dict(n=0), b'empty'), (do_step, dict(n=-3), b'empty')]
    cases += [(do_step, {k: None}, b'null') for k in ('z', 'g', 'xo', 'xn', 'step', 'gd', 'mm')]
    cases += [(do_step, dict(xn=z.ptr()), b'alias'), (do_step, dict(xn=g.ptr()), b'alias'),
              (do_step, dict(xn=xo.ptr()), b'alias'), (do_step, dict(g=z.ptr()), b'alias'),
              (do_step, dict(xn=ctypes.c_void_p(z.ptr().value + 8 * (n - 1))), b'alias'),
              (do_step, dict(mm=gd.ptr()), b'alias'),
              (do_step, dict(lower=nan), b'bound'), (do_step, dict(upper=nan), b'bound'),
              (do_step, dict(lower=1.0), b'bound'), (do_step, dict(lower=2.0), b'bound'),
              (do_step, dict(lower=inf, upper=inf), b'bound'),
              (do_step, dict(lower=-inf, upper=-inf), b'bound')]
    cases += [(do_momentum, dict(n=0), b'empty')]
    cases += [(do_momentum, {k: None}, b'null')
              for k in ('zz', 'a', 'b', 'gd', 'om', 'j_in', 'j_out')]
    cases += [(do_momentum, dict(n_part=k), b'n_part') for k in (0, 1, 3, 1024)]
    cases += [(do_momentum, dict(n_omega=k), b'n_omega') for k in (1, 0, -4)]
    cases += [(do_momentum, dict(zz=z.ptr()), b'alias'), (do_momentum, dict(zz=xo.ptr()), b'alias'),
              (do_momentum, dict(a=xo.ptr()), b'alias'),
              (do_momentum, dict(j_out=L.ptr(slots)), b'alias')]
    for i, (fn, kw, word) in enumerate(cases):
        assert fn(**kw) != 0, (i, fn.__name__, kw)
        assert word in lib.sphrt_last_error(), (i, fn.__name__, kw, lib.sphrt_last_error())
    tr.cuda.synchronize(gpu)
    assert all(bool(tr.isnan(b.view).all()) for b in (xn, gd, mm)) and not bool(slots.any())
    # and the same arguments unchanged are accepted
    assert do_step() == 0 and do_momentum() == 0
    assert do_step(lower=-inf, upper=inf) == 0 and do_step(lower=0.0, upper=inf) == 0
