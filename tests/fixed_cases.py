"""Adversarial inputs of the fixed-point accumulator (csrc/fixed.hpp), shared by the host test
(test_matrix_free_deterministic_cpu.py: the sphrt_fixed_*_host mirrors) and the device test
(test_gpu_fixed_kernels.py: the device compilations of the same functions).  No GPU dependency and
no library call: the references are Python integers, Fractions and float(int)."""
import math
import random
from fractions import Fraction

EXPONENTS = (-1070, -60, 0, 1, 61, 900)
ABOVE_BOUND = (1.5, 7.0, 26846.59, 2.0 ** 20 + 0.3, 2.0 ** 31)   # multiples of 0.7 * 2^E
SUM_BOUND = 3.7


def _terms(E):
    """Terms under a bound B = 2^E (1 - 2^-53)-ish: zero, the bound's neighbours, exact
    half-quantum ties on both parities, subnormals and values below half a quantum."""
    q = Fraction(2) ** (E - 61)
    out = [0.0, -0.0]
    top = math.ldexp(1 - 2.0 ** -53, E) if E - 53 >= -1074 else math.ldexp(0.75, E)
    out += [top, -top, math.ldexp(0.5, E), -math.ldexp(0.5, E)]
    for k in (0, 1, 2, 3, 4, 5, 2 ** 20, 2 ** 20 + 1, 2 ** 40 + 2, 2 ** 40 + 3, 2 ** 51, 2 ** 51 + 1):
        tie = (k + Fraction(1, 2)) * q                 # k even: rounds to k; odd: to k + 1
        for v in (tie, tie + q / 8, tie - q / 8, k * q, q / 2, q / 4, q * 3 / 8, q / 2 ** 30):
            f = float(v)
            if Fraction(f) == v and abs(f) <= top:     # (exactly representable ones only)
                out += [f, -f]
    out += [5e-324, -5e-324, 2.2250738585072014e-308 / 4, 2.2250738585072014e-308]
    return [t for t in out if abs(t) <= top]


def _pairs():
    """(lo, hi) pairs of a carry-save accumulator: |V| > 2^64, negative V, more than 53
    significant bits, ties and sticky cases of the 64-bit normalisation, lo near 2^62."""
    out = [(0, 0), (1, 0), (0, 1), (0, -1), (5, -1), (2 ** 32 - 1, 0), (2 ** 32 - 1, -1),
           (2 ** 62, 0), (2 ** 62 + 1, 2 ** 30), (2 ** 62 - 1, -(2 ** 59)),
           (2 ** 63 - 1, 2 ** 60 - 1), (2 ** 63 - 1, -(2 ** 60))]
    for v in (2 ** 53 + 1, 2 ** 54 + 2, 2 ** 54 + 6, 2 ** 64 + 2 ** 11, 2 ** 64 + 3 * 2 ** 11,
              2 ** 64 + 2 ** 11 + 1, 2 ** 64 + 2 ** 11 - 1, 2 ** 80 + 2 ** 27, 2 ** 80 + 2 ** 27 + 1,
              2 ** 80 + 3 * 2 ** 27, 2 ** 91 + 2 ** 38 + 2 ** 3, 2 ** 91 - 1, 2 ** 64, 2 ** 64 - 1,
              2 ** 65 + 2 ** 12, 2 ** 65 + 2 ** 12 + 1, 3 * 2 ** 63 + 2 ** 11 * 3, 2 ** 63,
              (2 ** 53 + 1) * 2 ** 30 + 1, (2 ** 53 + 3) * 2 ** 38 - 1):
        for sign in (1, -1):
            V = sign * v
            hi = V >> 32                               # the canonical split ...
            out.append((V - hi * 2 ** 32, hi))
            hi2 = hi - 2 ** 29                         # ... and one with a large lo
            lo2 = V - hi2 * 2 ** 32
            if 0 <= lo2 < 2 ** 63 and -(2 ** 63) <= hi2:
                out.append((lo2, hi2))
    return out


def above_bound_terms(E):
    """The finite terms of test_terms_above_the_bound_stay_exact: up to 2^32 times the bound."""
    out = [sign * math.ldexp(0.7, E) * mult for mult in ABOVE_BOUND for sign in (1, -1)]
    return [t for t in out if not math.isinf(t)]


def sum_terms():
    """The 4000 mixed-sign terms of test_quantise_then_value_round_trips_a_sum (bound 3.7)."""
    rng = random.Random(5)
    return [rng.uniform(-1, 1) * SUM_BOUND for _ in range(4000)]


def quanta(term, E):
    """The term in quanta of 2^(E - 61), rounded half to even: the exact integer the split holds."""
    return round(Fraction(term) / Fraction(2) ** (E - 61))
