"""The deterministic matrix-free adjoint on the GPU: MatrixFreeOperator(deterministic=True) and
back_project(deterministic=True) — the trace's fixed-point scatter (sphrt_fixed_scale_f64,
sphrt_trace_backproject_fixed_f64 / sphrt_trace_normal_fixed_f64, sphrt_fixed_finalize_f64) —
through every path a ray can take to its emit code, and gd()'s loop over it.

What is asserted bitwise: the result against a prediction made of Python integers (§1: the terms
from the float64-atomic back-projection of one-hot channels, which involves no sum; quantised
with Fractions; converted with float(int)), and results against each other (§2: two calls, a
permutation of the rays, a batch split over two calls, two backward passes; every path of §4;
two gd runs of §7).

Tolerances (the project's own): against the oracle float64 within 1e-10 x max|reference|,
float32 within 1e-5 x; against the float64-atomic mode rtol 1e-12 and atol 1e-12 x max.  The
quantisation error, at most n_adds x 2^-62 x the bound of a term, is far inside them.

Which path a case is on is asserted as in test_gpu_matrix_free_gradient.py §3."""
import ctypes
import gc as _gc
import math
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch as tr

import golden_cases as gc
from gpu_helpers import exact_stats
from test_gpu_adjoint_paths import (DGRID, F32, F64, SGRID, T_DYN, TOL, _assert_close,
                                    _check_coverage, _orbit, _rand, _Ref, _static_geom)
from test_gpu_matrix_free_gradient import (SCALE, _assert_gd_pins, _exact_waves, _gd_circ16,
                                           _ref_forward, _ref_gradient)

pytestmark = pytest.mark.gpu


def _agree(got, ref):
    assert tr.allclose(got, ref, rtol=1e-12, atol=1e-12 * float(ref.abs().max()))


def _op(grid, geom, gpu, **kw):
    from sph_raytracer_amd import MatrixFreeOperator
    return MatrixFreeOperator(grid, geom, device=gpu, deterministic=True, **kw)


def _atomic(op, fn):
    """fn() with the operator in its float64-atomic mode."""
    op.deterministic = False
    try:
        return fn()
    finally:
        op.deterministic = True


def _signed(shape, seed, gpu):
    return (_rand(shape, F64, seed, gpu) - 0.5) * 2


# ---- 1. exact bits, predicted independently of the code under test -------------------------------
N_EXACT = 64


def _exact_case():
    """A (1, 2, 4) grid of radius 1 — eight octants, L = 2 — and 64 rays none of which visits a
    voxel twice: 40 near the (1, 1, 1) diagonal (long chords through two opposite octants, so
    many large terms of one sign meet in a voxel) and 24 scattered ones (the other octants), all
    chosen with the oracle.  y: magnitudes in [0.9, 0.99], max exactly 0.99, the diagonal group
    positive and the others negative."""
    from sph_raytracer_amd import SphericalGrid
    grid = SphericalGrid(shape=(1, 2, 4), size_r=(0, 1))
    g = np.random.default_rng(11)
    n = 300
    d = g.normal(size=(n, 3))
    d[:150] = np.array([1.0, 1.0, 1.0]) + 0.12 * d[:150]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    through = g.uniform(-0.3, 0.3, size=(n, 3))
    through[:150] = 0.05 * g.normal(size=(150, 3)) + 0.02
    xs = through - 3.0 * d
    cand = _Ref(grid, gc.FixtureGeom(dict(xs=xs, rays=d, ray_shape=np.array([n]))))
    once = [i for i in range(n)
            if cand.ptr[i + 1] > cand.ptr[i] and
            np.unique(cand.vox[cand.ptr[i]:cand.ptr[i + 1]]).size == cand.ptr[i + 1] - cand.ptr[i]]
    keep = [i for i in once if i < 150][:40] + [i for i in once if i >= 150][:24]
    assert len(keep) == N_EXACT
    xs, d = np.ascontiguousarray(xs[keep]), np.ascontiguousarray(d[keep])
    geom = gc.FixtureGeom(dict(xs=xs, rays=d, ray_shape=np.array([N_EXACT])))
    ref = _Ref(grid, geom)
    # asserted from the reference's trace: no ray visits a voxel twice, >= 32 rays, >= half the
    # voxels hit
    for i in range(ref.n):
        v = ref.vox[ref.ptr[i]:ref.ptr[i + 1]]
        assert v.size and np.unique(v).size == v.size, i
    assert ref.n >= 32 and np.unique(ref.vox).size >= 0.5 * ref.vol
    mag = 0.9 + 0.09 * g.random(N_EXACT)
    mag[0] = 0.99
    y = np.where(np.arange(N_EXACT) < 40, mag, -mag)
    return grid, geom, ref, y


def _bits(a):
    return [struct.pack('<d', float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def _predict(lib, terms, bound):
    """terms (n_terms, vol) float64, each an exact product with no sum in it -> (the values the
    fixed-point sum must give, the integers V): E from the bound by the host mirror, every term
    quantised as a Fraction (round half to even), summed as Python integers, float(int), ldexp."""
    E, flags = ctypes.c_int32(), ctypes.c_int32()
    assert lib.sphrt_fixed_exponent_host(bound, E, flags) == 0 and flags.value == 0
    E = E.value
    q = Fraction(2) ** (E - 61)
    V = [0] * terms.shape[1]
    for row in terms:
        for v in np.flatnonzero(row):
            V[v] += round(Fraction(float(row[v])) / q)
    return np.array([math.ldexp(float(k), E - 61) for k in V]), V


def _one_hot_terms(op, r):
    """Every ray's terms r_i * len exactly: the float64-atomic back-projection of the one-hot
    channels diag(r) in one call — a voxel receives at most one non-zero add per channel."""
    n = r.numel()
    return _atomic(op, lambda: op.T(tr.diag(r))).reshape(n, -1).cpu().numpy()


def test_exact_bits_back_projection(gpu):
    from sph_raytracer_amd import _lib, back_project
    grid, geom, ref, y = _exact_case()
    op = _op(grid, geom, gpu)
    yt = tr.from_numpy(y).to(gpu)
    terms = _one_hot_terms(op, yt)
    assert terms.shape == (N_EXACT, ref.vol)
    for i in range(ref.n):                       # the terms sit where the reference's trace does
        assert set(np.flatnonzero(terms[i])) == set(ref.vox[ref.ptr[i]:ref.ptr[i + 1]])
    L = 2.0 * float(grid.r_b[-1])
    want, V = _predict(_lib.load(), terms, L * float(np.abs(y).max()))
    print(f'back-projection: max |V| = 2^{math.log2(max(abs(k) for k in V)):.2f}, '
          f'{sum(k < 0 for k in V)} negative totals of {len(V)}')
    assert max(abs(k) for k in V) > 2 ** 64 and min(V) < 0
    got = op.T(yt)
    assert got.shape == tuple(grid.shape) and got.dtype == F64
    assert _bits(got.cpu()) == _bits(want)
    assert _bits(back_project(grid, geom, yt, deterministic=True).cpu()) == _bits(want)


def test_exact_bits_residual_gradient(gpu):
    from sph_raytracer_amd import _lib
    grid, geom, ref, y = _exact_case()
    op = _op(grid, geom, gpu)
    x = _signed(grid.shape, 12, gpu)
    m = tr.from_numpy(y).to(gpu) * 0.7
    yhat = op(x)
    r = (yhat - m) * SCALE                      # the kernel's two roundings, formed in torch
    terms = _one_hot_terms(op, r)
    L = 2.0 * float(grid.r_b[-1])
    bound = (SCALE * L * L) * float(x.abs().max()) + (SCALE * L) * float(m.abs().max())
    want, V = _predict(_lib.load(), terms, bound)
    assert min(V) < 0 < max(V)
    yh, grad = op.residual_gradient(x, m, SCALE)
    assert tr.equal(yh, yhat)
    assert _bits(grad.cpu()) == _bits(want)


# ---- 2. order independence, bitwise ---------------------------------------------------------------
@pytest.fixture(scope='module')
def static_cases():
    """name -> (grid, geom, reference, deterministic MatrixFreeOperator), built once."""
    cache = {}

    def get(name, gpu):
        if name not in cache:
            from sph_raytracer_amd import SphericalGrid
            grid, geom = SphericalGrid(shape=SGRID), _static_geom(name)
            ref = _Ref(grid, geom)
            _check_coverage(ref)
            cache[name] = (grid, geom, ref, _op(grid, geom, gpu))
        return cache[name]

    return get


def _flat_geom(geom, order=None):
    rays = geom.rays.reshape(-1, 3)
    xs = geom.ray_starts.broadcast_to(geom.rays.shape).reshape(-1, 3)
    order = np.arange(len(rays)) if order is None else order
    return gc.FixtureGeom(dict(xs=xs.numpy()[order].copy(), rays=rays.numpy()[order].copy(),
                               ray_shape=np.array([len(order)])))


def test_two_calls_and_a_permutation_are_equal(gpu, static_cases):
    grid, geom, ref, op = static_cases('S3', gpu)
    y = _signed(geom.shape, 21, gpu)
    x, m = _rand(SGRID, F64, 22, gpu), _rand(geom.shape, F64, 23, gpu)
    a, (yh, g) = op.T(y), op.residual_gradient(x, m, SCALE)
    assert tr.equal(a, op.T(y))
    yh2, g2 = op.residual_gradient(x, m, SCALE)
    assert tr.equal(yh, yh2) and tr.equal(g, g2)
    perm = np.random.default_rng(24).permutation(ref.n)
    pop = _op(grid, _flat_geom(geom, perm), gpu)
    pt = tr.from_numpy(perm).to(gpu)
    assert tr.equal(pop.T(y.reshape(-1)[pt]), a)
    yhp, gp = pop.residual_gradient(x, m.reshape(-1)[pt], SCALE)
    assert tr.equal(yhp, yh.reshape(-1)[pt]) and tr.equal(gp, g)


def test_split_batch_through_the_c_abi(gpu, static_cases):
    """The first and the second half of the rays added into one accumulator under one record,
    then finalized: bitwise the whole batch."""
    from sph_raytracer_amd import _lib
    grid, geom, ref, op = static_cases('S1', gpu)
    lib, vol, n = _lib.load(), math.prod(SGRID), ref.n
    y = _signed((n,), 25, gpu)
    x, m = _rand(SGRID, F64, 26, gpu).reshape(-1), _rand((n,), F64, 27, gpu)
    whole_t = op.T(y.reshape(geom.shape))
    whole_y, whole_g = op.residual_gradient(x.reshape(SGRID), m.reshape(geom.shape), SCALE)
    halves = [_op(grid, _flat_geom(geom, np.arange(lo, hi)), gpu)
              for lo, hi in ((0, n // 2), (n // 2, n))]
    st = _lib.stream_of(gpu)
    L = 2.0 * float(grid.r_b[-1])
    rec = tr.zeros(2, dtype=tr.int64, device=gpu)
    out = tr.empty(vol, dtype=F64, device=gpu)
    # back-projection
    acc = tr.zeros(2 * vol, dtype=tr.int64, device=gpu)
    _lib.check(lib.sphrt_fixed_scale_f64(_lib.ptr(y), n, L, None, 0, 0.0, _lib.ptr(rec), st), 's')
    for h, (lo, hi) in zip(halves, ((0, n // 2), (n // 2, n))):
        plan, batch, ws = h._parts
        yy = y[lo:hi].contiguous()
        _lib.check(lib.sphrt_trace_backproject_fixed_f64(
            plan.handle, batch.desc, _lib.ptr(yy), 1, hi - lo, 0, _lib.ptr(acc), vol,
            _lib.ptr(rec), _lib.ptr(ws), ws.numel(), st), 'b')
    _lib.check(lib.sphrt_fixed_finalize_f64(_lib.ptr(acc), vol, _lib.ptr(rec), _lib.ptr(out), st), 'f')
    assert tr.equal(out.reshape(SGRID), whole_t)
    # gradient
    acc.zero_()
    yhat = tr.empty(n, dtype=F64, device=gpu)
    _lib.check(lib.sphrt_fixed_scale_f64(_lib.ptr(x), vol, SCALE * L * L, _lib.ptr(m), n, SCALE * L,
                                         _lib.ptr(rec), st), 's')
    for h, (lo, hi) in zip(halves, ((0, n // 2), (n // 2, n))):
        plan, batch, ws = h._parts
        mm, yy = m[lo:hi].contiguous(), yhat[lo:hi]
        _lib.check(lib.sphrt_trace_normal_fixed_f64(
            plan.handle, batch.desc, _lib.ptr(x), _lib.ptr(mm), SCALE, 1, vol, 0, _lib.ptr(yy),
            hi - lo, _lib.ptr(acc), _lib.ptr(rec), _lib.ptr(ws), ws.numel(), st), 'n')
    _lib.check(lib.sphrt_fixed_finalize_f64(_lib.ptr(acc), vol, _lib.ptr(rec), _lib.ptr(out), st), 'f')
    assert tr.equal(yhat.reshape(geom.shape), whole_y) and tr.equal(out.reshape(SGRID), whole_g)


def test_two_backward_passes_are_equal(gpu, static_cases):
    grid, geom, ref, op = static_cases('S2', gpu)
    w = _signed(geom.shape, 28, gpu)
    grads = []
    for _ in range(2):
        x = _rand(SGRID, F64, 29, gpu).requires_grad_()
        (op(x) * w).sum().backward()
        grads.append(x.grad)
    assert tr.equal(grads[0], grads[1]) and tr.equal(grads[0], op.T(w))
    _assert_close(grads[0], ref.adjoint(w), TOL[F64])


# ---- 3. accuracy, 5. layouts ----------------------------------------------------------------------
@pytest.mark.parametrize('lead', [(), (3,), (2, 2)], ids=['1ch', '3ch', '2x2ch'])
@pytest.mark.parametrize('name', ['S1', 'S4'])
def test_static_accuracy_and_channels(name, lead, gpu, static_cases):
    """1, 3 and (2, 2) channels: T and residual_gradient against the oracle's adjoint and against
    the float64-atomic mode; float32 in, float32 out."""
    grid, geom, ref, op = static_cases(name, gpu)
    n_chan = math.prod(lead)
    y = _signed(lead + tuple(geom.shape), 31, gpu)
    x = _rand(lead + SGRID, F64, 32, gpu)
    m = _rand(lead + tuple(geom.shape), F64, 33, gpu)
    t = op.T(y)
    assert t.shape == x.shape and t.dtype == F64 and t.device == gpu
    _assert_close(t, ref.adjoint(y, n_chan=n_chan), TOL[F64])
    _agree(t, _atomic(op, lambda: op.T(y)))
    yhat, grad = op.residual_gradient(x, m, SCALE)
    assert grad.shape == x.shape and grad.dtype == F64 and grad.device == gpu
    assert tr.equal(yhat, op(x))
    fwd = _ref_forward(ref, x, n_chan)
    _assert_close(grad, _ref_gradient(ref, fwd, m, SCALE, n_chan=n_chan), TOL[F64])
    _agree(grad, _atomic(op, lambda: op.residual_gradient(x, m, SCALE))[1])
    t32 = op.T(y.float())
    assert t32.dtype == F32 and t32.shape == x.shape
    _assert_close(t32, ref.adjoint(y.float(), n_chan=n_chan), TOL[F32])
    y32, g32 = op.residual_gradient(x.float(), m.float(), SCALE)
    assert y32.dtype == F32 and g32.dtype == F32 and g32.shape == x.shape
    fwd32 = _ref_forward(ref, x.float(), n_chan)
    _assert_close(g32, _ref_gradient(ref, fwd32, m.float(), SCALE, n_chan=n_chan), TOL[F32])


def test_host_tensors_in_host_tensors_out(gpu, static_cases):
    from sph_raytracer_amd import back_project
    grid, geom, ref, op = static_cases('S1', gpu)
    y, x = _signed(geom.shape, 34, 'cpu'), _rand(SGRID, F64, 35, 'cpu')
    t = back_project(grid, geom, y, deterministic=True)
    assert t.device.type == 'cpu' and tr.equal(t, op.T(y.to(gpu)).cpu())
    _assert_close(t, ref.adjoint(y), TOL[F64])
    yhat, grad = op.residual_gradient(x, y)
    assert yhat.device.type == 'cpu' and grad.device.type == 'cpu'
    _assert_close(grad, _ref_gradient(ref, _ref_forward(ref, x, 1), y, 1.0), TOL[F64])


@pytest.fixture(scope='module')
def dyn():
    from sph_raytracer_amd import ConeCircGeom, SphericalGrid
    grid = SphericalGrid(shape=DGRID)
    geoms = [ConeCircGeom((24, 16), pos=p, fov=(0, 12)) for p in _orbit(T_DYN)]
    geom = sum(geoms)
    return grid, geom, geoms[0], _Ref(grid, geom), _Ref(grid, geoms[0])


def test_dynamic_view_time_pairing(dyn, gpu):
    grid, geom, _, ref, _ = dyn
    div = ref.n // T_DYN
    op = _op(grid, geom, gpu, dynamic=True)
    y, x, m = _signed(geom.shape, 36, gpu), _rand(DGRID, F64, 37, gpu), _rand(geom.shape, F64, 38, gpu)
    t = op.T(y, time_slices=True)
    assert t.shape == DGRID and tr.equal(t, op.T(y, time_slices=True))
    _assert_close(t, ref.adjoint(y, div=div, n_t=T_DYN), TOL[F64])
    _agree(t, _atomic(op, lambda: op.T(y, time_slices=True)))
    with pytest.raises(NotImplementedError):
        op.T(y)
    yhat, grad = op.residual_gradient(x, m, SCALE)
    assert tr.equal(yhat, op(x)) and tr.equal(grad, op.residual_gradient(x, m, SCALE)[1])
    fwd = ref.forward(x, div=div)
    _assert_close(grad, _ref_gradient(ref, fwd, m, SCALE, div=div, n_t=T_DYN), TOL[F64])


def test_dynamic_single_detector(dyn, gpu):
    grid, _, single, _, ref1 = dyn
    op = _op(grid, single, gpu)
    yshape = (T_DYN,) + tuple(single.shape)
    y, x, m = _signed(yshape, 39, gpu), _rand(DGRID, F64, 40, gpu), _rand(yshape, F64, 41, gpu)
    t = op.T(y, time_slices=True)
    assert t.shape == DGRID and tr.equal(t, op.T(y, time_slices=True))
    _assert_close(t, ref1.adjoint(y, n_chan=T_DYN), TOL[F64])
    yhat, grad = op.residual_gradient(x, m, SCALE)
    assert tr.equal(yhat, op(x)) and tr.equal(grad, op.residual_gradient(x, m, SCALE)[1])
    _assert_close(grad, _ref_gradient(ref1, _ref_forward(ref1, x, T_DYN), m, SCALE, n_chan=T_DYN),
                  TOL[F64])


# ---- 4. every emit path ---------------------------------------------------------------------------
def _path_check(grid, geom, gpu, seed, ref=None, lead=()):
    """T and residual_gradient on one geometry: against the oracle, against the float64-atomic
    mode, and two calls bitwise equal -> the reference."""
    ref = ref or _Ref(grid, geom)
    n_chan = math.prod(lead)
    op = _op(grid, geom, gpu)
    y = _signed(lead + tuple(geom.shape), seed, gpu)
    x = _rand(lead + tuple(grid.shape), F64, seed + 100, gpu)
    m = _rand(lead + tuple(geom.shape), F64, seed + 200, gpu)
    t = op.T(y)
    assert t.shape == x.shape and tr.equal(t, op.T(y))
    _assert_close(t, ref.adjoint(y, n_chan=n_chan), TOL[F64])
    _agree(t, _atomic(op, lambda: op.T(y)))
    yhat, grad = op.residual_gradient(x, m, SCALE)
    yhat2, grad2 = op.residual_gradient(x, m, SCALE)
    assert tr.equal(yhat, op(x)) and tr.equal(yhat, yhat2) and tr.equal(grad, grad2)
    fwd = _ref_forward(ref, x, n_chan)
    _assert_close(yhat, fwd, TOL[F64])
    _assert_close(grad, _ref_gradient(ref, fwd, m, SCALE, n_chan=n_chan), TOL[F64])
    _agree(grad, _atomic(op, lambda: op.residual_gradient(x, m, SCALE))[1])
    return ref


def test_head_segments(gpu):
    case = gc.load('inside_starts')
    grid, geom = gc.make_grid(case), gc.FixtureGeom(case)
    st, shape = case['starts'], case['shape']
    inside = np.all((st >= 0) & (st < shape[:, None]), axis=0)
    assert inside.mean() >= 0.5
    ref = _path_check(grid, geom, gpu, 47)
    first = ref.vox[ref.ptr[:-1][inside]]
    svox = (st[0] * shape[1] + st[1]) * shape[2] + st[2]
    assert np.mean(first == svox[inside]) >= 0.9


@pytest.mark.parametrize('name', gc.LATTICE_CASES)
def test_lattice_tie_rays(name, gpu):
    from sph_raytracer_amd.raytracer import _Plan
    case = gc.load(name)
    grid = gc.make_grid(case)
    geom = gc.FixtureGeom(dict(case, xs=case['xs'].copy(), rays=case['rays'].copy()))
    assert len(case['xs']) == 8918
    assert _exact_waves(int(_Plan(grid, gpu).K)) == 4
    deferred = exact_stats(grid, geom, gpu)[0]
    ref = _Ref(grid, geom)
    hit = int((np.diff(ref.ptr) > 0).sum())
    assert 0 < deferred < hit, (deferred, hit)
    _path_check(grid, geom, gpu, 48, ref=ref)


def test_lds_list_path(gpu):
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    grid = SphericalGrid(shape=(300, 2, 2))
    geom = ConeRectGeom((4, 5), pos=(3, 0.01, 0.02), fov=(2, 2))
    ref = _Ref(grid, geom)
    assert int((np.diff(ref.ptr) > 512).sum()) >= 8
    assert np.unique(ref.vox).size >= 0.5 * ref.vol
    _path_check(grid, geom, gpu, 49, ref=ref)


def _lattice_subset(nr, gpu):
    from sph_raytracer_amd import SphericalGrid
    case = gc.load('lattice_full')
    grid = SphericalGrid(shape=(nr, 4, 4), size_r=(0, 2))
    xs, rays = case['xs'][::7].copy(), case['rays'][::7].copy()
    geom = gc.FixtureGeom(dict(xs=xs, rays=rays, ray_shape=np.array([len(xs)])))
    return grid, geom


@pytest.mark.parametrize('nr,waves', [(880, 1), (1000, 0)], ids=['one_wave', 'serial'])
def test_exact_path_large_lists(nr, waves, gpu):
    from sph_raytracer_amd.raytracer import _Plan
    grid, geom = _lattice_subset(nr, gpu)
    K = int(_Plan(grid, gpu).K)
    assert K == 2 * (nr + 1) + 2 * 5 + 5 + 1 and _exact_waves(K) == waves
    assert waves == 1 or K > 1815
    deferred = exact_stats(grid, geom, gpu)[0]
    ref = _Ref(grid, geom)
    assert 0 < deferred <= int((np.diff(ref.ptr) > 0).sum())
    _path_check(grid, geom, gpu, 50, ref=ref)


def test_large_k_route(gpu):
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    from sph_raytracer_amd.raytracer import _Plan
    grid = SphericalGrid(shape=(7000, 3, 5))
    geom = ConeRectGeom((6, 8), pos=(3, 0, 0.5), fov=(40, 40))
    K = int(_Plan(grid, gpu).K)
    assert K == 14017 and K > 13653 and _exact_waves(K) == 0
    ref = _Ref(grid, geom)
    hit = int((np.diff(ref.ptr) > 0).sum())
    assert ref.n == 48 and hit >= 24
    assert exact_stats(grid, geom, gpu)[0] == hit
    _path_check(grid, geom, gpu, 51, ref=ref)


def test_serial_walk_with_channels(gpu):
    grid, geom = _lattice_subset(1000, gpu)
    assert exact_stats(grid, geom, gpu)[0] > 0
    _path_check(grid, geom, gpu, 52, lead=(3,))


# ---- 6. degenerate inputs -------------------------------------------------------------------------
def _all_positive_zero(t):
    return t.numel() > 0 and bool((t.view(tr.int64) == 0).all())


def test_zero_residual_gives_exactly_zero(gpu, static_cases):
    grid, geom, ref, op = static_cases('S3', gpu)
    x = _rand((3,) + SGRID, F64, 61, gpu)
    m0 = op(x)
    y0, g0 = op.residual_gradient(x, m0, SCALE)
    assert tr.equal(y0, m0) and g0.shape == x.shape and _all_positive_zero(g0)


def test_all_rays_miss(gpu):
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    grid = SphericalGrid(shape=SGRID)
    geom = ConeRectGeom((9, 7), pos=(5, 0, 0), lookdir=(1, 0, 0), fov=(20, 20))
    assert _Ref(grid, geom).ptr[-1] == 0
    op = _op(grid, geom, gpu)
    for lead in ((), (3,)):
        x = _rand(lead + SGRID, F64, 62, gpu)
        m = _rand(lead + tuple(geom.shape), F64, 63, gpu)
        yhat, grad = op.residual_gradient(x, m, SCALE)
        assert yhat.shape == m.shape and grad.shape == x.shape
        assert _all_positive_zero(yhat) and _all_positive_zero(grad)
        assert _all_positive_zero(op.T(m))


def test_zero_and_non_finite_inputs(gpu, static_cases):
    """y = 0: the bound is zero, flag bit 0, +0.0 everywhere.  One inf (or NaN) in y: the bound
    is not finite, flag bit 1, NaN everywhere.  Plain flag branches: no adds are made."""
    grid, geom, ref, op = static_cases('S1', gpu)
    z = tr.zeros(geom.shape, dtype=F64, device=gpu)
    t = op.T(z)
    assert t.shape == SGRID and _all_positive_zero(t)
    assert _all_positive_zero(op.T(-z))
    for bad in (float('inf'), -float('inf'), float('nan')):
        y = _signed(geom.shape, 64, gpu)
        y.view(-1)[ref.n // 3] = bad
        assert bool(op.T(y).isnan().all())
    x, m = _rand(SGRID, F64, 65, gpu), _rand(geom.shape, F64, 66, gpu)
    m.view(-1)[5] = float('inf')
    yhat, grad = op.residual_gradient(x, m, SCALE)
    assert tr.equal(yhat, op(x)) and bool(grad.isnan().all())
    y0, g0 = op.residual_gradient(tr.zeros_like(x), tr.zeros_like(m), SCALE)
    assert _all_positive_zero(y0) and _all_positive_zero(g0)


# ---- 7. gd ----------------------------------------------------------------------------------------
def test_gd_is_bitwise_reproducible(gpu, monkeypatch):
    """gd() over a deterministic operator, twice: coefficients, y_result and both loss histories
    bitwise equal; the gd_circ16 fixture's pins; _normal_into once per iteration."""
    from sph_raytracer_amd import retrieval
    case, op, meas, model, sq, neg = _gd_circ16(gpu)
    op.deterministic = True
    coeffs0 = tr.ones(model.coeffs_shape, dtype=F64, device=gpu)
    assert retrieval._fused_plan(op, meas, model, coeffs0, [sq, neg], [coeffs0]) == (sq, neg)
    calls = {'normal': 0, 'fixed': set()}
    normal = op._normal_into

    def normal_into(*a):
        calls['normal'] += 1
        assert len(a) == 6                       # the loop hands over its own buffers ...
        calls['fixed'].add((a[5][0].data_ptr(), a[5][1].data_ptr()))
        return normal(*a)

    monkeypatch.setattr(op, '_normal_into', normal_into)
    runs = []
    for _ in range(2):
        calls['fixed'].clear()
        coeffs, y_res, losses = retrieval.gd(op, meas.clone(), model, lr=0.1,
                                             num_iterations=int(case['iterations']),
                                             loss_fns=[sq, neg], progress_bar=False)
        assert len(calls['fixed']) == 1          # ... the same pair in every iteration
        runs.append((coeffs.detach().clone(), y_res.detach().clone(),
                     list(losses[sq]), list(losses[neg])))
    assert calls['normal'] == 2 * int(case['iterations'])
    a, b = runs
    assert tr.equal(a[0], b[0]) and tr.equal(a[1], b[1])
    assert _bits(a[2]) == _bits(b[2]) and _bits(a[3]) == _bits(b[3])
    _assert_gd_pins(case, coeffs, y_res, losses, sq, neg, 'deterministic fused loop')


# ---- 8. memory ------------------------------------------------------------------------------------
def test_call_holds_nothing_per_segment(gpu, static_cases):
    """As test_gpu_matrix_free_gradient.py's: the call's peak exceeds what the operator holds by
    no more than yhat, the result, the integer accumulator (16 B per density element) and the
    16-byte record, each rounded up to the allocator's 512-byte blocks — far below one entry per
    segment — and nothing is left held after the call."""
    from sph_raytracer_amd import _lib
    grid, geom, ref, _ = static_cases('S3', gpu)
    lib = _lib.load()
    x, m = _rand(SGRID, F64, 71, gpu), _rand(geom.shape, F64, 72, gpu)
    _gc.collect()
    tr.cuda.synchronize(gpu)
    base = tr.cuda.memory_allocated(gpu)
    op = _op(grid, geom, gpu)
    op.residual_gradient(x, m, SCALE)
    _gc.collect()
    tr.cuda.synchronize(gpu)
    held = tr.cuda.memory_allocated(gpu) - base
    plan, batch, ws = op._parts
    ws_bytes = lib.sphrt_trace_workspace_bytes(plan.handle, batch.n)
    assert 0 < held <= 48 * batch.n + ws_bytes + lib.sphrt_plan_table_bytes(plan._desc)
    tr.cuda.reset_peak_memory_stats(gpu)
    yhat, grad = op.residual_gradient(x, m, SCALE)
    tr.cuda.synchronize(gpu)
    peak = tr.cuda.max_memory_allocated(gpu) - base - held
    allowed = (2 * (8 * x.numel() + 512) + 2 * (8 * m.numel() + 512)
               + 16 * x.numel() + 512 + 512)
    print(f'deterministic residual_gradient peak {peak} B over the operator, allowed {allowed} B, '
          f'{len(ref.seg)} segments ({12 * len(ref.seg)} B as a CSR)')
    assert 12 * len(ref.seg) > allowed
    assert 0 < peak <= allowed
    del yhat, grad
    _gc.collect()
    tr.cuda.synchronize(gpu)
    assert tr.cuda.memory_allocated(gpu) - base == held
