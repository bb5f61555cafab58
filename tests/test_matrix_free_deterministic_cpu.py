"""Host side of the deterministic matrix-free adjoint (csrc/fixed.hpp; sphrt_fixed_scale_f64,
sphrt_trace_backproject_fixed_f64, sphrt_trace_normal_fixed_f64, sphrt_fixed_finalize_f64,
sphrt_fixed_accumulate_f64 and the three host mirrors): the entries are declared, exported and bound; their refusals fire on the
host, before any device call; the fixed-point arithmetic equals Python's integers and
float(int) bit for bit; the Python layer has the ``deterministic`` switches and still raises
layout errors before it looks for a device.  (No compute call: no GPU here.)"""
import ctypes
import math
import os
import re
import struct
from fractions import Fraction

import pytest
import torch as tr

from fixed_cases import EXPONENTS, _pairs, _terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {                                   # name -> argument count
    'sphrt_fixed_scale_f64': 8,
    'sphrt_trace_backproject_fixed_f64': 12,
    'sphrt_trace_normal_fixed_f64': 15,
    'sphrt_fixed_finalize_f64': 5,
    'sphrt_fixed_accumulate_f64': 6,
    'sphrt_fixed_exponent_host': 3,
    'sphrt_fixed_quantise_host': 3,
    'sphrt_fixed_value_host': 4,
}


def _bits(v):
    return struct.pack('<d', v)


def _lib():
    from sph_raytracer_amd import _lib, build
    build.build()
    return _lib.load()


# ---- 1. entries -----------------------------------------------------------------------------------
def test_entries_declared_exported_and_bound():
    from sph_raytracer_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, 'include', 'sphrt.h')).read()
    normal = re.search(r'int\s+sphrt_trace_normal_f64\s*\(', hdr)
    assert normal
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    last = normal.start()
    for name, n_args in ENTRIES.items():
        m = re.search(r'(?:int|void|double)\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr)
        assert m, f'{name} is not declared in include/sphrt.h'
        assert m.start() > last, f'{name} is not declared after its predecessor'
        last = m.start()
        assert len(m.group(1).split(',')) == n_args, name
        assert name in _lib.EXPORTED and hasattr(raw, name)
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert lib.sphrt_fixed_value_host.restype is ctypes.c_double
    assert lib.sphrt_fixed_quantise_host.restype is None
    assert lib.sphrt_trace_normal_fixed_f64.argtypes[4] is ctypes.c_double      # scale, by value
    assert lib.sphrt_fixed_scale_f64.argtypes[2] is ctypes.c_double
    # each comment names what the entry replaces and states the contract
    comment = hdr[normal.start():]
    for word in ('sphrt_trace_backproject_f64', 'sphrt_trace_normal_f64', 'llrint', 'ldexp',
                 '2^31', '2^29', 'ties to even', 'flags bit 0', 'flags bit 1', 'carry'):
        assert word in comment, word


# ---- 2. host refusals -----------------------------------------------------------------------------
def _host_plan(grid):
    """A plan over host 'tables' (as tests/test_matrix_free_gradient_cpu.py): enough for the
    checks that read the plan's grid, no device needed."""
    from sph_raytracer_amd import raytracer as rt
    stg = rt._Staging()
    plan = rt._Plan(grid, tr.device('cuda', 0), staging=stg)
    stg.upload('cpu')
    plan.attach(stg)
    return plan, stg


def _rays(n):
    from sph_raytracer_amd import _lib
    rays = _lib.RayBatch()
    rays.ndim = 1
    rays.shape[0] = n
    rays.xs_stride[0] = rays.rays_stride[0] = 3
    rays.xs = rays.rays = rays.start = 16     # never dereferenced: every call fails its checks
    return rays


def _check(lib, cases):
    for i, (run, word) in enumerate(cases):
        assert run() != 0, i
        assert word in lib.sphrt_last_error(), (i, word, lib.sphrt_last_error())


def test_trace_refusals_on_the_host():
    """The atomic siblings' refusals, a null scale record and the 2^29 cap, each with its word in
    sphrt_last_error, before the library asks for a device."""
    from sph_raytracer_amd import SphericalGrid
    lib = _lib()
    grid = SphericalGrid(shape=(4, 5, 6))
    plan, _keep = _host_plan(grid)
    vol, n = 4 * 5 * 6, 10
    rays, p, h = _rays(n), ctypes.c_void_p(16), plan.handle
    need = lib.sphrt_trace_workspace_bytes(h, n)
    assert need > 0
    huge = ctypes.c_size_t(-1).value

    def normal(plan=h, rays=rays, d=p, m=p, scale=0.5, n_chan=1, cs=vol, div=0, yhat=p, ycs=n,
               acc=p, rec=p, ws=p, ws_size=need):
        return lib.sphrt_trace_normal_fixed_f64(
            plan, ctypes.byref(rays) if rays is not None else None, d, m, scale, n_chan, cs, div,
            yhat, ycs, acc, rec, ws, ws_size, None)

    def back(plan=h, rays=rays, y=p, n_chan=1, ycs=n, div=0, acc=p, cs=vol, rec=p, ws=p,
             ws_size=need):
        return lib.sphrt_trace_backproject_fixed_f64(
            plan, ctypes.byref(rays) if rays is not None else None, y, n_chan, ycs, div, acc, cs,
            rec, ws, ws_size, None)

    shared = lambda call: [                                          # noqa: E731
        (lambda: call(plan=None), b'null plan'),
        (lambda: call(rays=None), b'null ray batch'),
        (lambda: call(acc=None), b'null'),
        (lambda: call(rec=None), b'scale record'),
        (lambda: call(n_chan=0), b'n_chan'),
        (lambda: call(n_chan=-2), b'n_chan'),
        (lambda: call(n_chan=3, div=5), b'ray_chan_div'),
        (lambda: call(cs=vol - 1), b'chan_stride'),
        (lambda: call(n_chan=2, ycs=n - 1), b'y_chan_stride'),
        (lambda: call(ws_size=need - 1), b'workspace too small'),
        (lambda: call(ws_size=0), b'workspace too small'),
        (lambda: call(ws=None), b'workspace too small'),
        # the cap: n_rays * max(n_chan, 1) >= 2^29, whatever the workspace
        (lambda: call(rays=_rays(2 ** 29), ws_size=huge), b'capacity'),
        (lambda: call(rays=_rays(2 ** 40), ws_size=huge), b'capacity'),
        (lambda: call(rays=_rays(2 ** 27), n_chan=4, ycs=2 ** 27, ws_size=huge), b'capacity'),
        (lambda: call(n_chan=2 ** 29, ycs=n), b'capacity'),
    ]
    _check(lib, shared(normal) + [(lambda: normal(d=None), b'density, m, yhat or acc'),
                                  (lambda: normal(m=None), b'density, m, yhat or acc'),
                                  (lambda: normal(yhat=None), b'density, m, yhat or acc')])
    _check(lib, shared(back) + [(lambda: back(y=None), b'y or acc')])
    # one ray below the cap passes it (and is refused for its workspace instead)
    _check(lib, [(lambda: normal(rays=_rays(2 ** 29 - 1)), b'workspace too small'),
                 (lambda: back(rays=_rays(2 ** 29 - 1)), b'workspace too small')])


def test_scale_and_finalize_refusals_on_the_host():
    lib = _lib()
    p = ctypes.c_void_p(16)
    scale, fin = lib.sphrt_fixed_scale_f64, lib.sphrt_fixed_finalize_f64
    add = lib.sphrt_fixed_accumulate_f64
    _check(lib, [
        (lambda: scale(p, 4, 1.0, None, 0, 0.0, None, None), b'scale record'),
        (lambda: scale(p, -1, 1.0, None, 0, 0.0, p, None), b'negative scale length'),
        (lambda: scale(p, 4, 1.0, p, -1, 1.0, p, None), b'negative scale length'),
        (lambda: scale(None, 4, 1.0, None, 0, 0.0, p, None), b'null scale input'),
        (lambda: scale(p, 4, 1.0, None, 3, 1.0, p, None), b'null scale input'),
        (lambda: scale(p, 4, -1.0, None, 0, 0.0, p, None), b'scale factor'),
        (lambda: scale(p, 4, float('nan'), None, 0, 0.0, p, None), b'scale factor'),
        (lambda: scale(p, 4, 1.0, p, 4, -2.0, p, None), b'scale factor'),
        (lambda: fin(p, 4, None, p, None), b'scale record'),
        (lambda: fin(p, -1, p, p, None), b'negative finalize length'),
        (lambda: fin(None, 4, p, p, None), b'acc or out'),
        (lambda: fin(p, 4, p, None, None), b'acc or out'),
        (lambda: add(p, p, 4, None, p, None), b'scale record'),
        (lambda: add(p, p, -1, p, p, None), b'negative accumulate length'),
        (lambda: add(None, p, 4, p, p, None), b'terms, index or acc'),
        (lambda: add(p, None, 4, p, p, None), b'terms, index or acc'),
        (lambda: add(p, p, 4, p, None, None), b'terms, index or acc'),
    ])
    E, flags = ctypes.c_int32(), ctypes.c_int32()
    _check(lib, [(lambda: lib.sphrt_fixed_exponent_host(-1.0, E, flags), b'negative bound'),
                 (lambda: lib.sphrt_fixed_exponent_host(1.0, None, flags), b'null'),
                 (lambda: lib.sphrt_fixed_exponent_host(1.0, E, None), b'null')])


# ---- 3. arithmetic against Python integers --------------------------------------------------------
def _exponent(lib, bound):
    E, flags = ctypes.c_int32(7), ctypes.c_int32(7)
    assert lib.sphrt_fixed_exponent_host(bound, E, flags) == 0
    return E.value, flags.value


def _quantise(lib, term, E):
    out = (ctypes.c_int64 * 2)()
    lib.sphrt_fixed_quantise_host(term, E, out)
    return out[0], out[1]


def _round_half_even(q):
    """A Fraction to the nearest integer, ties to even (what Python's round does on one)."""
    return round(q)


def test_exponent_is_frexp():
    lib = _lib()
    for E in EXPONENTS:
        for f in (0.5, 0.75, 1 - 2.0 ** -53):
            if E - 53 < -1074 and f != 0.5 and f != 0.75:
                continue                              # (not representable that far down)
            B = math.ldexp(f, E)
            assert math.frexp(B) == (f, E)
            assert _exponent(lib, B) == (E, 0)
    assert _exponent(lib, 5e-324) == (-1073, 0)
    assert _exponent(lib, 1.7976931348623157e308) == (1024, 0)
    for B in (3.0, 1e-300, 6.02e23, 0.1):
        assert _exponent(lib, B) == (math.frexp(B)[1], 0)


def test_flags():
    """Bit 0: a zero bound — every value is +0.0.  Bit 1: a bound that is not finite — every
    value is NaN.  Whatever the accumulator holds."""
    lib = _lib()
    assert _exponent(lib, 0.0)[1] == 1
    assert _exponent(lib, float('inf'))[1] == 2
    assert _exponent(lib, float('nan'))[1] == 2
    for lo, hi in ((0, 0), (123, -7), (2 ** 62, 2 ** 59)):
        z = lib.sphrt_fixed_value_host(lo, hi, 0, 1)
        assert _bits(z) == _bits(0.0)
        assert math.isnan(lib.sphrt_fixed_value_host(lo, hi, 0, 2))
        assert math.isnan(lib.sphrt_fixed_value_host(lo, hi, 0, 3))


@pytest.mark.parametrize('E', EXPONENTS)
def test_quantise_equals_python_integers(E):
    lib = _lib()
    terms = _terms(E)
    q = Fraction(2) ** (E - 61)
    ties = 0
    for term in terms:
        want = _round_half_even(Fraction(term) / q)
        assert abs(want) <= 2 ** 61
        ties += (Fraction(term) / q).denominator == 2
        lo, hi = _quantise(lib, term, E)
        assert (lo, hi) == (want & 0xffffffff, want >> 32), (E, term, want)
        assert 0 <= lo < 2 ** 32 and hi * 2 ** 32 + lo == want
    if E - 61 - 1 >= -1074:                            # (half quanta exist as doubles)
        assert ties >= 8, ties
        assert any(t != 0 and _quantise(lib, t, E) == (0, 0) for t in terms)   # below q / 2
    else:
        assert min(abs(t) for t in terms if t) >= q    # (every double is a whole quantum here)
    assert sum(t != 0 and abs(t) < 2.2250738585072014e-308 for t in terms) >= 2   # subnormals


@pytest.mark.parametrize('E', EXPONENTS)
def test_terms_above_the_bound_stay_exact(E):
    """A head segment may be many diameters long: a term up to 2^32 times the bound is split
    exactly all the same (hi beyond 2^29), and the pair's value is the term's, correctly
    rounded."""
    lib = _lib()
    q = Fraction(2) ** (E - 61)
    for mult in (1.5, 7.0, 26846.59, 2.0 ** 20 + 0.3, 2.0 ** 31):
        for sign in (1, -1):
            term = sign * math.ldexp(0.7, E) * mult
            if math.isinf(term):
                continue
            want = round(Fraction(term) / q)
            lo, hi = _quantise(lib, term, E)
            assert 0 <= lo < 2 ** 32 and hi * 2 ** 32 + lo == want, (E, mult, sign)
            got = lib.sphrt_fixed_value_host(lo, hi, E, 0)
            assert _bits(got) == _bits(math.ldexp(float(want), E - 61))


@pytest.mark.parametrize('E', EXPONENTS)
def test_value_equals_float_of_int(E):
    lib = _lib()
    seen = {'big': 0, 'neg': 0, 'wide': 0}
    for lo, hi in _pairs():
        V = hi * 2 ** 32 + lo
        seen['big'] += abs(V) > 2 ** 64
        seen['neg'] += V < 0
        seen['wide'] += abs(V).bit_length() - (abs(V) & -abs(V)).bit_length() + 1 > 53 if V else 0
        want = math.ldexp(float(V), E - 61)
        got = lib.sphrt_fixed_value_host(lo, hi, E, 0)
        assert _bits(got) == _bits(want), (E, lo, hi, got, want)
    assert min(seen.values()) >= 8, seen


def test_quantise_then_value_round_trips_a_sum():
    """A few thousand mixed-sign terms summed as the accumulator sums them (lo and hi
    separately, no carry between them): the value is the correctly rounded exact sum of the
    quantised terms."""
    import random
    lib = _lib()
    rng = random.Random(5)
    terms = [rng.uniform(-1, 1) * 3.7 for _ in range(4000)]
    E, flags = _exponent(lib, 3.7)
    assert flags == 0
    lo = hi = total = 0
    for term in terms:
        a, b = _quantise(lib, term, E)
        lo, hi = lo + a, hi + b
        total += round(Fraction(term) / Fraction(2) ** (E - 61))
    assert hi * 2 ** 32 + lo == total and lo < 2 ** 63
    got = lib.sphrt_fixed_value_host(lo, hi, E, 0)
    assert _bits(got) == _bits(math.ldexp(float(total), E - 61))
    assert abs(got - math.fsum(terms)) <= len(terms) * 2.0 ** -62 * 3.7 + 2.0 ** -52 * abs(got)


# ---- 4. the Python layer --------------------------------------------------------------------------
def _operator(grid, geom):
    """A MatrixFreeOperator as far as the host goes (tests/test_matrix_free_gradient_cpu.py)."""
    from sph_raytracer_amd import MatrixFreeOperator
    op = object.__new__(MatrixFreeOperator)
    op.grid, op.geom, op._ray_shape = grid, geom, tuple(geom.shape)
    return op


def test_deterministic_switches_exist():
    import inspect
    from sph_raytracer_amd import MatrixFreeOperator, back_project
    assert inspect.signature(back_project).parameters['deterministic'].default is False
    par = inspect.signature(MatrixFreeOperator.__init__).parameters['deterministic']
    assert par.default is False
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    op = _operator(SphericalGrid((4, 4, 4)), ConeRectGeom((4, 5), (5, 0, 0)))
    assert op.deterministic is False
    op.deterministic = True
    assert op.deterministic is True
    for doc in (MatrixFreeOperator.__doc__, back_project.__doc__):
        assert 'not bitwise reproducible' not in doc
        assert 'deterministic' in doc and '16 more bytes' in doc and 'two integer atomics' in doc


def test_layout_errors_before_any_device(monkeypatch):
    """With the deterministic mode on, layout errors are still raised before the device is
    looked for (the monkeypatch of test_matrix_free_gradient_cpu.py)."""
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid, _lib, back_project

    def never(*a, **k):
        raise AssertionError('a layout error must come before the device')

    monkeypatch.setattr(_lib, 'require_gpu', never)
    grid, geom = SphericalGrid((4, 4, 4)), ConeRectGeom((4, 5), (5, 0, 0))
    op = _operator(grid, geom)
    op.deterministic = True
    x = tr.ones(4, 4, 4)
    with pytest.raises(ValueError, match='ray shape'):
        op.residual_gradient(x, tr.ones(4, 6))
    with pytest.raises(ValueError, match='density of shape'):
        op.residual_gradient(x, tr.ones(3, 4, 5))
    with pytest.raises(ValueError, match='ray shape'):
        op.T(tr.ones(4, 6))
    with pytest.raises(ValueError, match='ray shape'):
        back_project(grid, geom, tr.ones(5), deterministic=True)
    dyn = SphericalGrid((5, 4, 4, 4))
    coll = sum(ConeRectGeom((4, 5), (5, 0, k)) for k in range(5))
    dop = _operator(dyn, coll)
    dop.deterministic = True
    with pytest.raises(ValueError, match='cannot pair'):
        dop.residual_gradient(tr.ones(3, 4, 4, 4), tr.ones(3, 4, 5))
    with pytest.raises(NotImplementedError):
        dop.T(tr.ones(5, 4, 5))                         # (the time_slices rule)
    with pytest.raises(NotImplementedError):
        back_project(dyn, coll, tr.ones(5, 4, 5), time_slices=False, deterministic=True)
    with pytest.raises(ValueError, match='cannot pair'):
        back_project(dyn, coll, tr.ones(3, 4, 5), deterministic=True)
