"""The retrieval loop's elementwise kernels (csrc/loss.hip) past one element per thread and on
values that are not benign, against the cases of tests/loop_cases.py (shown sound on the CPU by
test_loop_cases_cpu.py).  Every comparison is bitwise or against an exact integer sum; the one
bound (the regulariser's total on random values) is the derived n * 2^-53 * sum|terms|.

  Adam       both arithmetics of adam_neg_kernel against torch's own step on the same GPU, at
             every length of LENGTHS (one, two, three and four elements per thread), parameters
             and both moments as int64 views (so -0.0 != +0.0; NaN at the same indices, payloads
             not compared), signed zeros, denormals, g * g under- and overflow, infinities and
             NaN planted in every stride; the FOREACH step also against the exact-rational
             restatement of its documented operation sequence.
  partials   neg_reg_kernel's, the Adam launch's and sq_residual_kernel's per-workgroup sums on
             the exact value set, each workgroup's against an integer reference (not in sum).
  stage      the Adam launch's brick-stage write at every voxel of a 70 x 65 x 66 grid (more
             than one element per thread, padding columns in every dimension).
Every output buffer sits between 64-element NaN guards.

Mutations of the library (each built once, run once against this file; not committed):
  1. the Adam loop reads param[i0] for param[i] on later iterations: both Adam tests fail at
     n = 262145 and 786433 in every configuration (24 cases) and pass at every shorter length;
     the Adam launch's exact partials fail at the same two lengths.
  2. the stage write only when `first`: test_adam_stage_write_every_voxel fails, nothing else.
  3. block_partial sums three of the four wave totals: the regulariser's and the residual's
     per-workgroup partials fail at every n >= 255 (35 cases); n <= 65 passes, as it must: the
     fourth wave owns no element there.  The Adam tests pass: they compare the Adam launch's
     partials with neg_reg_kernel's, both through the same block_partial; the exact partials of
     test_neg_reg_gradient_and_partials are what holds the Adam launch.
  (4 to 6 change csrc/fixed.*: nothing here fails; see test_gpu_fixed_kernels.py.)
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch as tr

import loop_cases as lc
from gpu_helpers import _stage_col

pytestmark = pytest.mark.gpu
GUARD = lc.GUARD
HYPER = {'lr': 0.01, 'beta2': 0.999, 'eps': 1e-8}


@functools.lru_cache(maxsize=None)
def _inputs(n):
    return lc.adam_inputs(n, seed=n)


@functools.lru_cache(maxsize=None)
def _sample(n):
    return lc.sample_indices(n, _inputs(n)['special'], seed=n)


def _lib(gpu):
    from sph_raytracer_amd import _lib
    return _lib, _lib.load(), _lib.stream_of(gpu)


def _guarded(values, gpu, dtype=tr.float64):
    """(whole, view): the values (a numpy array, or a length: NaN) between NaN guards."""
    n = values if isinstance(values, int) else len(values)
    whole = tr.full((n + 2 * GUARD,), float('nan'), dtype=dtype, device=gpu)
    view = whole[GUARD:GUARD + n]
    if not isinstance(values, int):
        view.copy_(tr.from_numpy(np.ascontiguousarray(values)))
    return whole, view


def _guards_nan(*wholes):
    return all(bool(tr.isnan(w[:GUARD]).all()) and bool(tr.isnan(w[-GUARD:]).all()) for w in wholes)


def _same_bits(name, want, got, ctx):
    """NaN at the same indices, every other element equal as int64 (so -0.0 != +0.0)."""
    wn, gn = tr.isnan(want), tr.isnan(got)
    a = tr.where(wn, 0, want.view(tr.int64))
    b = tr.where(gn, 0, got.view(tr.int64))
    if not (tr.equal(wn, gn) and tr.equal(a, b)):
        bad = ((wn != gn) | (a != b)).nonzero().reshape(-1)
        k = int(bad[0])
        pytest.fail(f'{ctx}: {name} differs at {len(bad)} of {want.numel()} elements, first {k}: '
                    f'{want[k].item()!r} (torch) vs {got[k].item()!r}')


def _bitwise(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64),
                          np.asarray(b, dtype=np.float64).view(np.int64))


# ---- B1: Adam against torch -----------------------------------------------------------------------
def _adam_case(n, gpu, foreach, wd, c_neg, beta1):
    L, lib, st = _lib(gpu)
    inp = _inputs(n)
    hyper = dict(HYPER, beta1=beta1, wd=wd)
    pa, ma, va = (tr.from_numpy(inp[k]).to(gpu) for k in ('p', 'm', 'v'))      # torch's
    (wp, pb), (wm, mb), (wv, vb) = (_guarded(inp[k], gpu) for k in ('p', 'm', 'v'))
    n_part = lib.sphrt_loss_partials(n)
    assert n_part == lc.grid_of(n)
    samp = tr.from_numpy(_sample(n)).to(gpu)
    if foreach:
        opt = tr.optim.Adam([pa], lr=hyper['lr'], betas=(beta1, hyper['beta2']), eps=hyper['eps'],
                            weight_decay=wd, foreach=True)
        opt.state[pa] = {'step': tr.tensor(0.0), 'exp_avg': ma, 'exp_avg_sq': va}
    else:
        steps = [tr.zeros((), dtype=tr.float32, device=gpu)]
    n_steps = lc.steps_of(n)
    for it in range(n_steps):
        ctx = f'n={n} step {it}'
        g = tr.from_numpy(inp['g'][it]).to(gpu)
        ga = g.clone()
        part_a = tr.empty(n_part, dtype=tr.float64, device=gpu)
        wpart, part_b = _guarded(n_part, gpu)
        if c_neg is not None:
            L.check(lib.sphrt_neg_reg_f64(L.ptr(pa), n, c_neg, L.ptr(ga), L.ptr(part_a), st), 'neg')
        emulate = foreach and it in (0, 1, 2, n_steps - 1)
        if emulate:
            before = [t[samp].cpu().tolist() for t in (pb, g, mb, vb)]
        if foreach:
            pa.grad = ga
            opt.step()
            step_size, bc2s = lc.bias_corrections(hyper, it + 1)
            L.check(lib.sphrt_adam_foreach_neg_f64(
                L.ptr(pb), L.ptr(g), L.ptr(mb), L.ptr(vb), n, step_size, beta1, hyper['beta2'],
                hyper['eps'], wd, bc2s, c_neg or 0.0, L.ptr(part_b if c_neg is not None else None),
                None, st), 'adam_foreach')
        else:
            tr._foreach_add_(steps, 1)
            tr._fused_adam_([pa], [ga], [ma], [va], [], steps, amsgrad=False, lr=hyper['lr'],
                            beta1=beta1, beta2=hyper['beta2'], weight_decay=wd, eps=hyper['eps'],
                            maximize=False, grad_scale=None, found_inf=None)
            L.check(lib.sphrt_adam_neg_f64(
                L.ptr(pb), L.ptr(g), L.ptr(mb), L.ptr(vb), n, hyper['lr'], beta1, hyper['beta2'],
                hyper['eps'], wd, float(it + 1), c_neg or 0.0,
                L.ptr(part_b if c_neg is not None else None), None, st), 'adam_neg')
        for name, a, b in (('param', pa, pb), ('exp_avg', ma, mb), ('exp_avg_sq', va, vb)):
            _same_bits(name, a, b, ctx)
        assert _guards_nan(wp, wm, wv, wpart), ctx
        if c_neg is not None:
            _same_bits('partials', part_a, part_b, ctx)
        else:
            assert bool(tr.isnan(part_b).all()), ctx               # no partials asked, none written
        if emulate:
            after = [t[samp].cpu().tolist() for t in (pb, mb, vb)]
            for j, i in enumerate(_sample(n).tolist()):
                want = lc.foreach_step_ref(*(col[j] for col in before), hyper, it + 1, c_neg)
                have = tuple(col[j] for col in after)
                assert all(map(lc.same_or_both_nan, want, have)), \
                    (ctx, i, [col[j] for col in before], want, have)


@pytest.mark.parametrize('n', lc.LENGTHS)
@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('c_neg', [None, 0.3])
@pytest.mark.parametrize('beta1', [0.9, 0.3])
def test_adam_foreach_every_length_and_value(beta1, c_neg, wd, n, gpu):
    """sphrt_adam_foreach_neg_f64 against torch.optim.Adam(foreach=True) and, on the sample,
    against foreach_step_ref."""
    _adam_case(n, gpu, True, wd, c_neg, beta1)


@pytest.mark.parametrize('n', lc.LENGTHS)
@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('c_neg', [None, 0.3])
def test_adam_fused_every_length_and_value(c_neg, wd, n, gpu):
    """sphrt_adam_neg_f64 against torch._fused_adam_ (its bias corrections are the device's pow:
    held to torch only)."""
    _adam_case(n, gpu, False, wd, c_neg, 0.9)


# ---- B2: regulariser ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', lc.LENGTHS)
def test_neg_reg_gradient_and_partials(n, gpu):
    L, lib, st = _lib(gpu)
    c_neg = 0.3
    n_part = lib.sphrt_loss_partials(n)
    inp = _inputs(n)
    # special + random values: the gradient is torch's g - c * (d < 0), bit for bit
    d = tr.from_numpy(inp['p']).to(gpu)
    wg, g = _guarded(inp['g'][0], gpu)
    want = g.sub(d.lt(0).to(tr.float64), alpha=c_neg)
    wpart, part = _guarded(n_part, gpu)
    L.check(lib.sphrt_neg_reg_f64(L.ptr(d), n, c_neg, L.ptr(g), L.ptr(part), st), 'neg_reg')
    _same_bits('gradient', want, g, f'n={n}')
    assert _guards_nan(wg, wpart)
    # exact values: every workgroup's partial is its integer sum
    dx, gx = lc.exact_values(n, seed=n), lc.exact_values(n, seed=n + 1)
    ref = lc.neg_partials_ref(dx, n)
    d = tr.from_numpy(dx).to(gpu)
    wg, g = _guarded(gx, gpu)
    wpart, part = _guarded(n_part, gpu)
    L.check(lib.sphrt_neg_reg_f64(L.ptr(d), n, c_neg, L.ptr(g), L.ptr(part), st), 'neg_reg')
    assert _bitwise(part.cpu().numpy(), ref), np.flatnonzero(part.cpu().numpy() != ref)[:8]
    assert _guards_nan(wg, wpart)
    # ... and so is each of the Adam launch's, in both arithmetics
    for foreach in (True, False):
        (wp, p), (wm, m), (wv, v) = (_guarded(a, gpu) for a in (dx, np.zeros(n), np.zeros(n)))
        wpart, part = _guarded(n_part, gpu)
        g = tr.from_numpy(gx).to(gpu)
        if foreach:
            step_size, bc2s = lc.bias_corrections(dict(HYPER, beta1=0.9), 1)
            L.check(lib.sphrt_adam_foreach_neg_f64(
                L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, step_size, 0.9, 0.999, 1e-8, 0.0, bc2s,
                c_neg, L.ptr(part), None, st), 'adam_foreach')
        else:
            L.check(lib.sphrt_adam_neg_f64(
                L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, 0.01, 0.9, 0.999, 1e-8, 0.0, 1.0,
                c_neg, L.ptr(part), None, st), 'adam_neg')
        assert _bitwise(part.cpu().numpy(), ref), (foreach, np.flatnonzero(part.cpu().numpy() != ref)[:8])
        assert _guards_nan(wp, wm, wv, wpart)
    # random values: the total within the recursive-summation bound of the exact sum
    dr = np.random.default_rng(n).standard_normal(n)
    d = tr.from_numpy(dr).to(gpu)
    g = tr.zeros(n, dtype=tr.float64, device=gpu)
    wpart, part = _guarded(n_part, gpu)
    L.check(lib.sphrt_neg_reg_f64(L.ptr(d), n, c_neg, L.ptr(g), L.ptr(part), st), 'neg_reg')
    terms = np.abs(np.minimum(dr, 0.0))
    exact = math.fsum(terms)
    total = math.fsum(part.cpu().tolist())
    assert abs(total - exact) <= n * 2.0 ** -53 * exact, (total, exact)
    assert _guards_nan(wpart)


# ---- B3: residual ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n', lc.LENGTHS)
@pytest.mark.parametrize('ydt', [tr.float64, tr.float32])
@pytest.mark.parametrize('ordered', [False, True])
def test_sq_residual_partials_per_workgroup(ordered, ydt, n, gpu):
    """sphrt_sq_residual_f64 on the exact value set: each workgroup's partial is the integer sum
    of the squared residuals of the outputs it owns (through the ray map: of rays order[j]), and
    the scaled residual is torch's, bit for bit."""
    L, lib, st = _lib(gpu)
    yh, y = lc.residual_inputs(n)
    order = np.random.default_rng(n).permutation(n).astype(np.int32) if ordered else None
    ref = lc.sq_partials_ref(yh[order], y[order], n) if ordered else lc.sq_partials_ref(yh, y, n)
    yhat, yy = tr.from_numpy(yh).to(gpu), tr.from_numpy(y).to(ydt).to(gpu)
    od = tr.from_numpy(order).to(gpu) if ordered else None
    n_part = lib.sphrt_loss_partials(n)
    assert n_part == len(ref)
    wout, out = _guarded(n, gpu)
    wpart, part = _guarded(n_part, gpu)
    scale = 0.37
    L.check(lib.sphrt_sq_residual_f64(L.ptr(yhat), L.ptr(yy), int(ydt == tr.float64), n, scale,
                                      L.ptr(od), L.ptr(out), L.ptr(part), st), 'sq_residual')
    r = yhat - yy.to(tr.float64)
    if ordered:
        r = r[od.long()]
    _same_bits('r_scaled', r * scale, out, f'n={n}')
    got = part.cpu().numpy()
    assert _bitwise(got, ref), np.flatnonzero(got != ref)[:8]
    assert _guards_nan(wout, wpart)


# ---- B4: stage write ------------------------------------------------------------------------------
def test_adam_stage_write_every_voxel(gpu, monkeypatch):
    """On a 70 x 65 x 66 grid (300300 voxels: a second element for 38156 threads; no extent a
    multiple of the 4 x 2 x 4 brick: padding columns in every dimension), after each of 3 Adam
    launches of each arithmetic with stage_of: the stage holds param[v] at _stage_col(v) for
    every voxel, every padding column is untouched, and a forward through the stage (no pack)
    is op(param) bit for bit.  A stage_of of another size or with too small a buffer is refused
    with nothing written."""
    from sph_raytracer_amd import ConeCircGeom, Operator, SphericalGrid
    L, lib, st = _lib(gpu)
    shape, brick = (70, 65, 66), (4, 2, 4)
    n = math.prod(shape)
    assert n == 300300 > lc.STRIDE and all(s % b for s, b in zip(shape, brick))
    monkeypatch.setenv('SPHRT_BRICK', ','.join(map(str, brick)))
    grid = SphericalGrid(shape=shape)
    geom = sum(ConeCircGeom(shape=(8, 16), pos=(5 * math.cos(th), 5 * math.sin(th), 1), fov=(0, 45))
               for th in (0.0, 2.0))
    op = Operator(grid, geom, device=gpu)
    desc = op._csr['desc']
    assert desc.stage_shape[0] > 0 and tuple(desc.stage_brick) == brick
    sd, buf = op._stage_for_loop(tr.float64)
    cols = sd.stage_cols
    assert cols == 72 * 66 * 68 and buf.numel() == 8 * cols == sd.stage_bytes
    col_of = _stage_col(np.arange(n, dtype=np.int64), shape, brick)
    assert len(np.unique(col_of)) == n and col_of.max() < cols
    pad = np.setdiff1d(np.arange(cols, dtype=np.int64), col_of)
    assert len(pad) == cols - n
    col_of, pad = tr.from_numpy(col_of).to(gpu), tr.from_numpy(pad).to(gpu)
    stage = buf.view(tr.float64)[:cols]
    rng = np.random.default_rng(70)
    p0 = rng.standard_normal(n)
    n_rays = op._csr['n']
    for foreach in (True, False):
        (wp, p), (wm, m), (wv, v) = (_guarded(a, gpu) for a in (p0, np.zeros(n), np.zeros(n)))
        sd.stage_packed = 0
        buf.fill_(0x5a)
        out = tr.empty(n_rays, dtype=tr.float64, device=gpu)
        op._forward_staged(p, out, sd)                       # packs p0
        sd.stage_packed = 1
        snapshot = stage.view(tr.int64).clone()
        assert tr.equal(stage[col_of].view(tr.int64), p.view(tr.int64))
        # refusals first: nothing may be written
        state = [t.clone() for t in (wp, wm, wv)]
        g = tr.from_numpy(rng.standard_normal(n)).to(gpu)
        small = L.CSR.from_buffer_copy(sd)
        small.stage_bytes = 8 * cols - 1
        for bad, count, word in ((sd, n - 1, b'voxels, the CSR has'), (small, n, b'too small')):
            if foreach:
                rc = lib.sphrt_adam_foreach_neg_f64(
                    L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), count, -0.1, 0.9, 0.999, 1e-8, 0.0,
                    0.03, 0.0, None, ctypes.byref(bad), st)
            else:
                rc = lib.sphrt_adam_neg_f64(
                    L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), count, 0.01, 0.9, 0.999, 1e-8, 0.0,
                    1.0, 0.0, None, ctypes.byref(bad), st)
            assert rc != 0 and word in lib.sphrt_last_error(), lib.sphrt_last_error()
        assert all(tr.equal(a.view(tr.int64), b.view(tr.int64)) for a, b in zip(state, (wp, wm, wv)))
        assert tr.equal(stage.view(tr.int64), snapshot)
        for it in range(3):
            g = tr.from_numpy(rng.standard_normal(n) * 10.0 ** (it % 4 - 2)).to(gpu)
            before = p.clone()
            if foreach:
                step_size, bc2s = lc.bias_corrections(dict(HYPER, beta1=0.9), it + 1)
                L.check(lib.sphrt_adam_foreach_neg_f64(
                    L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, step_size, 0.9, 0.999, 1e-8, 0.0,
                    bc2s, 0.0, None, ctypes.byref(sd), st), 'adam_foreach')
            else:
                L.check(lib.sphrt_adam_neg_f64(
                    L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, 0.01, 0.9, 0.999, 1e-8, 0.0,
                    float(it + 1), 0.0, None, ctypes.byref(sd), st), 'adam_neg')
            ctx = f'foreach={foreach} launch {it}'
            assert int((p != before).sum()) > n - 16, ctx          # the step moved the parameters
            _same_bits('stage', p, stage[col_of], ctx)
            assert tr.equal(stage.view(tr.int64)[pad], snapshot[pad]), ctx
            assert _guards_nan(wp, wm, wv), ctx
            op._forward_staged(p, out, sd)                   # stage_packed = 1: reads the stage
            assert sd.stage_packed == 1
            assert tr.equal(out.view(geom.shape), op(p.view(shape))), ctx
