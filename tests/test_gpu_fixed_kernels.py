"""The device compilations of the fixed-point accumulator's arithmetic (csrc/fixed.hpp through
csrc/fixed.hip) on the adversarial inputs of tests/fixed_cases.py, which
test_matrix_free_deterministic_cpu.py holds the host mirrors to: the device's clz, u64 -> f64
conversion, ldexp, rint and floor (subnormal results at E = -1070 included) against Python
integers and float(int), bit for bit.

  finalize    sphrt_fixed_finalize_f64 on every accumulator pair of _pairs() under every
              exponent, the flagged records, lengths round a workgroup, guards round `out`.
  scale       sphrt_fixed_scale_f64 (fixed_max_kernel, fixed_record_kernel) against the bound
              in Python floats and sphrt_fixed_exponent_host: the maximum at wave, workgroup and
              array edges and past eight values per thread, carried by a negative value, -0.0,
              a bound that rounds to zero, inf and NaN of either sign, the second input absent,
              empty, zero and dominant.
  accumulate  sphrt_fixed_accumulate_f64 (the trace's own device add, fixed_accumulate) on the
              tie, subnormal and above-the-bound terms, one element each, and 4000 terms into
              one element in two orders.

Mutations of the library (each built once, run once against this file; not committed):
  4. fixed_value drops the sticky bit: test_finalize_equals_float_of_int fails on the tie pairs
     at every exponent but -1070, and test_finalize_lengths_and_flags from 255 elements up (the
     first tie pair is past element 1).  At E = -1070 it passes: every result is subnormal
     there, rounded again at far fewer bits, and the sticky bit's half ulp of 2^-53 is lost in
     that second rounding whichever way it went.
  5. fixed_max_kernel without the sign mask: test_scale_finds_the_maximum_wherever_it_is fails
     at every length above 1 (any negative value's pattern outranks the maximum's; at n = 1
     the lone negative maximum gives a negative bound, whose frexp exponent is the same), all
     of test_scale_zero_and_non_finite_bounds (-0.0 beside 0.75 wins the maximum) and three of
     the four test_scale_second_input cases.
  6. fixed_quantise truncates instead of rounding to nearest even: both accumulate tests fail
     (half-quantum terms, the 4000-term sum) at every exponent but -1070, where no term has a
     fraction of a quantum.
  (1 to 3 change csrc/loss.hip: nothing here fails; see test_gpu_loop_kernels.py.)
"""
import ctypes
import math
import random
import struct
from fractions import Fraction

import pytest
import torch as tr

import fixed_cases as fc

pytestmark = pytest.mark.gpu
GUARD = 64
# bit patterns of the non-finite values, as int64: +inf, -inf, NaN, NaN with the sign bit set
NON_FINITE = (0x7ff0000000000000, 0x7ff0000000000000 - 2 ** 63, 0x7ff8000000000000,
              0x7ff8000000000000 - 2 ** 63)


def _bits(v):
    return struct.pack('<d', v)


def _lib(gpu):
    from sph_raytracer_amd import _lib
    return _lib, _lib.load(), _lib.stream_of(gpu)


def _record(E, flags, gpu):
    return tr.tensor([E, flags, 0, 0], dtype=tr.int32, device=gpu)


def _guarded(n, dtype, gpu, fill):
    """(whole, view): n elements between GUARD elements on either side, all `fill`."""
    whole = tr.full((n + 2 * GUARD,), fill, dtype=dtype, device=gpu)
    return whole, whole[GUARD:GUARD + n]


def _guards_nan(whole, n):
    return bool(tr.isnan(whole[:GUARD]).all()) and bool(tr.isnan(whole[GUARD + n:]).all())


def _exponent(lib, B):
    E, flags = ctypes.c_int32(7), ctypes.c_int32(7)
    assert lib.sphrt_fixed_exponent_host(B, E, flags) == 0
    return E.value, flags.value


# ---- finalize -----------------------------------------------------------------------------------
@pytest.mark.parametrize('E', fc.EXPONENTS)
def test_finalize_equals_float_of_int(E, gpu):
    L, lib, st = _lib(gpu)
    pairs = fc._pairs()
    acc = tr.tensor(pairs, dtype=tr.int64, device=gpu)
    whole, out = _guarded(len(pairs), tr.float64, gpu, float('nan'))
    L.check(lib.sphrt_fixed_finalize_f64(L.ptr(acc), len(pairs), L.ptr(_record(E, 0, gpu)),
                                         L.ptr(out), st), 'finalize')
    got = out.cpu().tolist()
    assert _guards_nan(whole, len(pairs))
    sub = 0
    for (lo, hi), g in zip(pairs, got):
        want = math.ldexp(float(hi * 2 ** 32 + lo), E - 61)
        sub += want != 0 and abs(want) < 2.2250738585072014e-308
        assert _bits(g) == _bits(want), (E, lo, hi, g, want)
    assert sub >= 8 if E == -1070 else sub == 0           # subnormal results where they exist


@pytest.mark.parametrize('n_elems', [1, 255, 256, 257])
def test_finalize_lengths_and_flags(n_elems, gpu):
    """Exactly n_elems outputs are written (the rest of a 257-element `out` and its guards stay
    NaN / the fill), and a flagged record gives +0.0 (bit 0) or NaN (bit 1, alone or with bit 0)
    whatever the accumulator holds."""
    L, lib, st = _lib(gpu)
    pairs = (fc._pairs() * 4)[:257]
    acc = tr.tensor(pairs, dtype=tr.int64, device=gpu)
    E = 1
    for flags in (0, 1, 2, 3):
        whole, out = _guarded(257, tr.float64, gpu, -7.0)
        whole[:GUARD] = whole[GUARD + 257:] = float('nan')
        L.check(lib.sphrt_fixed_finalize_f64(L.ptr(acc), n_elems, L.ptr(_record(E, flags, gpu)),
                                             L.ptr(out), st), 'finalize')
        got = out.cpu().tolist()
        assert _guards_nan(whole, 257) and got[n_elems:] == [-7.0] * (257 - n_elems)
        for (lo, hi), g in zip(pairs[:n_elems], got):
            if flags & 2:
                assert math.isnan(g)
            elif flags & 1:
                assert _bits(g) == _bits(0.0)
            else:
                assert _bits(g) == _bits(math.ldexp(float(hi * 2 ** 32 + lo), E - 61))


# ---- scale --------------------------------------------------------------------------------------
def _scale(gpu, a, fa, b=None, fb=0.0, nb=None):
    """The record sphrt_fixed_scale_f64 writes over 16 bytes of garbage -> (E, flags)."""
    L, lib, st = _lib(gpu)
    rec = tr.full((4 + 2 * 4,), 0x7f7f7f7f, dtype=tr.int32, device=gpu)
    nb = (b.numel() if b is not None else 0) if nb is None else nb
    L.check(lib.sphrt_fixed_scale_f64(L.ptr(a), a.numel(), fa, L.ptr(b), nb, fb, L.ptr(rec[4:8]),
                                      st), 'scale')
    r = rec.cpu().tolist()
    assert r[:4] == [0x7f7f7f7f] * 4 and r[8:] == [0x7f7f7f7f] * 4     # 16 bytes, no more
    assert r[6:8] == [0, 0], 'the second 8 bytes of the record must read 0'
    return r[4], r[5]


SCALE_LENGTHS = [1, 63, 64, 65, 2047, 2048, 2049, 2097152, 2097157]


@pytest.mark.parametrize('n', SCALE_LENGTHS)
def test_scale_finds_the_maximum_wherever_it_is(n, gpu):
    """The maximum magnitude, carried by a negative value, at the first and the last element and
    on either side of every wave, workgroup, per-thread-eight and launch edge the length has
    (2097152 = 1024 workgroups x 256 threads x 8 values: from there on a ninth value)."""
    _, lib, _ = _lib(gpu)
    g = tr.Generator(device='cpu').manual_seed(n)
    x = (tr.rand(n, generator=g, dtype=tr.float64) * 2 - 1).to(gpu)
    edges = (0, 63, 64, 255, 256, 2047, 2048, 262143, 262144, 2097151, 2097152, 2097156, n - 1)
    fa = 0.3
    base = float(x.abs().max())
    assert _scale(gpu, x, fa) == _exponent(lib, fa * base)
    for pos in sorted({p for p in edges if p < n}):
        for big in (-3.5, 2.0 ** 40 + 1):
            keep = x[pos].clone()
            x[pos] = big
            assert _scale(gpu, x, fa) == _exponent(lib, fa * abs(big)), (n, pos, big)
            x[pos] = keep
    assert _exponent(lib, fa * 3.5) != _exponent(lib, fa * base)        # (the cases can tell)


@pytest.mark.parametrize('n', [1, 65, 2049])
def test_scale_zero_and_non_finite_bounds(n, gpu):
    _, lib, _ = _lib(gpu)
    z = tr.full((n,), -0.0, dtype=tr.float64, device=gpu)
    assert bool((z.view(tr.int64) == -2 ** 63).all())
    assert _scale(gpu, z, 1.0) == (0, 1)                                # all -0.0: the zero flag
    assert _scale(gpu, tr.zeros(n, dtype=tr.float64, device=gpu), 1.0) == (0, 1)
    x = z.clone()
    x[n // 2] = 5e-324
    assert 0.25 * 5e-324 == 0.0
    assert _scale(gpu, x, 0.25) == (0, 1)                               # the bound rounds to 0
    assert _scale(gpu, x, 1.0) == _exponent(lib, 5e-324) == (-1073, 0)
    # -0.0 beside a positive value: the sign bit must not win the pattern maximum
    x = tr.full((n + 1,), 0.75, dtype=tr.float64, device=gpu)
    x[n] = -0.0
    assert int(x.view(tr.int64)[n]) == -2 ** 63
    assert _scale(gpu, x, 1.0) == _exponent(lib, 0.75)
    for bad in NON_FINITE:
        for pos in sorted({0, n // 2, n - 1}):
            x = tr.full((n,), 0.75, dtype=tr.float64, device=gpu)
            x.view(tr.int64)[pos] = bad
            assert _scale(gpu, x, 0.5) == (0, 2), (hex(bad), pos)
    # a NaN beside an infinity, and an infinite factor: non-finite all the same
    x = tr.full((max(n, 2),), float('inf'), dtype=tr.float64, device=gpu)
    x.view(tr.int64)[0] = NON_FINITE[3]
    assert _scale(gpu, x, 0.5) == (0, 2)
    assert _scale(gpu, tr.ones(n, dtype=tr.float64, device=gpu), float('inf')) == (0, 2)


@pytest.mark.parametrize('na, nb', [(65, 1), (1, 65), (2049, 257), (257, 2049)])
def test_scale_second_input(na, nb, gpu):
    """B = fa * max|a| + fb * max|b| in single IEEE operations (fixed_record_kernel's have_b
    arm): b absent, of length 0, all zero, smaller and dominant, with its maximum negative."""
    _, lib, _ = _lib(gpu)
    g = tr.Generator(device='cpu').manual_seed(na * 7 + nb)
    a = (tr.rand(na, generator=g, dtype=tr.float64) * 2 - 1).to(gpu)
    b = (tr.rand(nb, generator=g, dtype=tr.float64) * 2 - 1).to(gpu)
    a[na // 2], b[nb - 1] = -1.7, -2.9
    fa, fb = 0.3, 0.7
    only_a = _exponent(lib, fa * 1.7)
    assert _scale(gpu, a, fa) == only_a                                  # b absent
    assert _scale(gpu, a, fa, b, fb, nb=0) == only_a                     # nb = 0
    assert _scale(gpu, a, fa, tr.zeros_like(b), fb) == _exponent(lib, fa * 1.7 + fb * 0.0)
    assert _scale(gpu, a, fa, b, fb) == _exponent(lib, fa * 1.7 + fb * 2.9)
    assert _scale(gpu, a, fa, b, 2.0 ** 30) == _exponent(lib, fa * 1.7 + 2.0 ** 30 * 2.9)
    assert _exponent(lib, fa * 1.7 + 2.0 ** 30 * 2.9) != only_a != _exponent(lib, fa * 1.7 + fb * 2.9)
    assert _scale(gpu, tr.zeros_like(a), fa, b, fb) == _exponent(lib, fa * 0.0 + fb * 2.9)
    assert _scale(gpu, tr.zeros_like(a), fa, tr.zeros_like(b), fb) == (0, 1)
    b[0] = float('nan')
    assert _scale(gpu, a, fa, b, fb) == (0, 2)
    assert _scale(gpu, a, fa, b, 0.0) == (0, 2)                          # 0 * NaN is NaN


# ---- accumulate ---------------------------------------------------------------------------------
def _accumulate(gpu, terms, index, n_elems, E, flags=0):
    """The accumulator (n_elems pairs between guards, zeroed) after one
    sphrt_fixed_accumulate_f64 -> ([(lo, hi)], the device tensor)."""
    L, lib, st = _lib(gpu)
    whole, acc = _guarded(2 * n_elems, tr.int64, gpu, 0)
    whole[:GUARD] = whole[GUARD + 2 * n_elems:] = 0x5a5a5a5a
    t = tr.tensor(terms, dtype=tr.float64, device=gpu)
    ix = tr.tensor(index, dtype=tr.int64, device=gpu)
    L.check(lib.sphrt_fixed_accumulate_f64(L.ptr(t), L.ptr(ix), len(terms),
                                           L.ptr(_record(E, flags, gpu)), L.ptr(acc), st), 'add')
    w = whole.cpu().tolist()
    assert w[:GUARD] == w[GUARD + 2 * n_elems:] == [0x5a5a5a5a] * GUARD
    flat = w[GUARD:GUARD + 2 * n_elems]
    return list(zip(flat[0::2], flat[1::2])), acc


@pytest.mark.parametrize('E', fc.EXPONENTS)
def test_accumulate_equals_python_integers(E, gpu):
    """Each term of _terms(E) (ties on both parities, subnormals, below half a quantum) and each
    above-the-bound multiple into its own element: {lo, hi} is the split of the exactly rounded
    quotient.  A flagged record adds nothing."""
    terms = fc._terms(E) + fc.above_bound_terms(E)
    n = len(terms)
    got, _ = _accumulate(gpu, terms, list(range(n)), n, E)
    ties = 0
    for term, (lo, hi) in zip(terms, got):
        want = fc.quanta(term, E)
        ties += (Fraction(term) / Fraction(2) ** (E - 61)).denominator == 2
        assert (lo, hi) == (want & 0xffffffff, want >> 32), (E, term, want, lo, hi)
    assert ties >= 8 or E - 62 < -1074
    assert max(abs(fc.quanta(t, E)) for t in terms) > 2 ** 61              # above the bound
    for flags in (1, 2, 3):
        got, _ = _accumulate(gpu, terms, list(range(n)), n, E, flags)
        assert got == [(0, 0)] * n


def test_accumulate_a_sum_in_two_orders(gpu):
    """The 4000 terms of test_quantise_then_value_round_trips_a_sum into one element (every add
    contends for the same pair), in two orders: both pairs equal the Python integer sums of the
    split quanta, and the finalized value is ldexp(float(total), E - 61) bit for bit."""
    L, lib, st = _lib(gpu)
    terms = fc.sum_terms()
    E, flags = _exponent(lib, fc.SUM_BOUND)
    assert flags == 0
    ks = [fc.quanta(t, E) for t in terms]
    total, lo, hi = sum(ks), sum(k & 0xffffffff for k in ks), sum(k >> 32 for k in ks)
    assert hi * 2 ** 32 + lo == total and lo < 2 ** 63
    shuffled = terms[:]
    random.Random(11).shuffle(shuffled)
    assert shuffled != terms
    # element 1 of three: its neighbours must stay untouched
    for order in (terms, shuffled):
        got, acc = _accumulate(gpu, order, [1] * len(order), 3, E)
        assert got == [(0, 0), (lo, hi), (0, 0)]
        whole, out = _guarded(3, tr.float64, gpu, float('nan'))
        L.check(lib.sphrt_fixed_finalize_f64(L.ptr(acc), 3, L.ptr(_record(E, 0, gpu)),
                                             L.ptr(out), st), 'finalize')
        vals = out.cpu().tolist()
        assert _guards_nan(whole, 3)
        assert [_bits(v) for v in vals] == [_bits(0.0), _bits(math.ldexp(float(total), E - 61)),
                                            _bits(0.0)]
