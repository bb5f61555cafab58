"""tests/loop_cases.py holds what it claims, on references alone (no GPU, no library call): the
lengths reach one, two and three-or-four elements per thread; the exact value set's sums are
exact whatever their order; the special tuples sit in every stride of the longest case; and the
exact-rational FOREACH step gives a hand-computed result and tells the documented operation
sequence from its two nearest neighbours."""
import math
import os
import re
import struct
from fractions import Fraction

import numpy as np
import pytest

import loop_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = {'lr': 0.01, 'beta1': 0.9, 'beta2': 0.999, 'eps': 1e-8, 'wd': 0.0}


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, 'sph_raytracer_amd', 'csrc', 'loss.hip')).read()
    assert int(re.search(r'kLossThreads = (\d+);', src).group(1)) == lc.THREADS
    assert int(re.search(r'kLossMaxBlocks = (\d+);', src).group(1)) == lc.MAX_BLOCKS
    assert lc.STRIDE == 262144 == 64 ** 3


def test_lengths_reach_every_class():
    """sphrt_loss_partials' formula restated: one element per thread up to 262144, exactly two
    for exactly one thread at 262145, three for every thread and four for thread 0 of workgroup
    0 alone at 786433; the short lengths sit on both sides of a wave and a workgroup."""
    assert lc.LENGTHS == [1, 63, 64, 65, 255, 256, 257, 262143, 262144, 262145, 786433]
    for n in lc.LENGTHS:
        e = lc.elems_per_thread(n)
        assert e.sum() == n and len(e) == 256 * lc.grid_of(n)
        if n <= 262144:
            assert e.max() == 1
            assert lc.grid_of(n) == -(-n // 256)
        else:
            assert lc.grid_of(n) == 1024
    assert [lc.grid_of(n) for n in (1, 63, 64, 65, 255, 256, 257)] == [1, 1, 1, 1, 1, 1, 2]
    assert lc.grid_of(262143) == lc.grid_of(262144) == 1024 and lc.elems_per_thread(262143)[-1] == 0
    e = lc.elems_per_thread(262145)
    assert e[0] == 2 and (e[1:] == 1).all()
    e = lc.elems_per_thread(786433)
    assert e[0] == 4 and (e[1:] == 3).all()
    assert 786433 == 3 * lc.STRIDE + 1
    assert [lc.steps_of(n) for n in (257, 262143)] == [20, 3]


def test_exact_set_sums_are_exact_in_any_order():
    n = max(lc.LENGTHS)
    assert n * 64 ** 2 < 2 ** 50                 # |value| <= 64: every sum of squares of values
    assert n * 128 ** 2 * 64 < 2 ** 53           # and of squared differences, in 64ths, fits
    for m in lc.LENGTHS:
        d = lc.exact_values(m, seed=m)
        k = d * 8
        assert np.array_equal(k, np.round(k)) and np.abs(d).max() <= 64
        assert (d < 0).sum() * 4 >= m and (m < 4 or (d > 0).sum() * 4 >= m)
        assert np.array_equal(d.astype(np.float32).astype(np.float64), d)     # float32 y holds it
        yh, y = lc.residual_inputs(m)
        assert d[-1] < 0 and yh[-1] != y[-1]         # the ragged last element is in both sums
    d, y = lc.residual_inputs(n)
    assert d[-1] < 0
    neg, sq = lc.neg_partials_ref(d, n), lc.sq_partials_ref(d, y, n)
    assert len(neg) == len(sq) == 1024
    # against Fractions on a few workgroups, in the owner rule's own words
    for b in (0, 1, 511, 1023):
        own = [i for i in range(n) if (i // 256) % 1024 == b]
        assert len(own) == (256 * 3 + 1 if b == 0 else 256 * 3)
        assert Fraction(neg[b]) == sum(Fraction(-d[i]) for i in own if d[i] < 0)
        assert Fraction(sq[b]) == sum((Fraction(d[i]) - Fraction(y[i])) ** 2 for i in own)
    # float64 sums in three different orders give the same bits
    terms = np.abs(np.minimum(d, 0.0))
    perm = np.random.default_rng(0).permutation(n)
    assert float(np.sum(terms)) == float(np.sum(terms[perm])) == math.fsum(terms) == neg.sum()
    s = 0.0
    for x in terms[::-1][:5000]:
        s += x
    assert s == math.fsum(terms[::-1][:5000])
    # a dropped wave total, or a partial of the wrong stride, is a different number
    b0 = [i for i in range(n) if (i // 256) % 1024 == 0]
    assert neg[0] != math.fsum(terms[i] for i in b0 if i % 256 < 192)
    assert neg[0] != math.fsum(terms[i] for i in b0[:-1])
    assert sq[0] != math.fsum((d[i] - y[i]) ** 2 for i in b0[:-1])
    # short lengths: one workgroup owns everything
    d = lc.exact_values(255, seed=3)
    assert lc.neg_partials_ref(d, 255).tolist() == [math.fsum(-x for x in d if x < 0)]
    assert len(lc.neg_partials_ref(lc.exact_values(257, 4), 257)) == 2


def test_special_set_and_its_placement():
    tuples = lc.special_tuples()
    bits = lambda x: struct.pack('<d', x)                         # noqa: E731
    want = {bits(s) for s in lc.SPECIALS if not math.isnan(s)}
    assert len(lc.SPECIALS) == 13 and len(want) == 12
    for slot in (0, 1):
        have = {bits(t[slot]) for t in tuples if not math.isnan(t[slot])}
        assert want <= have and any(math.isnan(t[slot]) for t in tuples)
    assert {0.0, 5e-324, 1e300} <= {t[3] for t in tuples}
    assert all(t[3] >= 0 for t in tuples)                          # a second moment is a square
    n = 786433
    place = lc.special_placement(n)
    idx = [i for i, _ in place]
    assert len(set(idx)) == len(idx) == 3 * len(tuples) + 1 <= 512
    assert place[-1] == (n - 1, lc.LAST_TUPLE)
    for lo, hi in ((0, 262144), (262144, 524288), (524288, 786432)):
        here = [tup for i, tup in place if lo <= i < hi]
        assert len(here) == len(tuples) and all(map(_same_tuple, here, tuples))
    # a copy straddles the first wave edge; every shorter length keeps its last element
    assert {63, 64} <= set(idx)
    for m in lc.LENGTHS:
        pl = lc.special_placement(m)
        assert pl[-1][0] == m - 1 and all(0 <= i < m for i, _ in pl)
        assert len({i for i, _ in pl}) == len(pl)
    assert len(lc.special_placement(63)) == 42 + 1 and len(lc.special_placement(255)) == len(tuples) + 1
    # plant + sample: every special index is in the sample, which stays within 512
    inp = lc.adam_inputs(65, seed=5)
    samp = lc.sample_indices(65, inp['special'], seed=1)
    assert len(samp) == 65 and set(inp['special']) <= set(samp)
    big = lc.sample_indices(n, np.asarray(idx), seed=1)
    assert len(big) == 512 and set(idx) <= set(big.tolist())
    assert all(_same_tuple((inp['p'][i], g[i], inp['m'][i], inp['v'][i]), tup)
               for g in inp['g'][:1] for i, tup in lc.special_placement(65))
    assert all(lc.same_or_both_nan(g[i], tup[1]) for g in inp['g'] for i, tup in lc.special_placement(65))


def _same_tuple(a, b):
    return all(lc.same_or_both_nan(float(x), float(y)) for x, y in zip(a, b))


def test_fma_is_one_rounding_with_ieee_edges():
    assert lc.fma(2.0 ** -30, 2.0 ** -30, 1.0) == 1.0
    a = 1 + 2.0 ** -30
    assert lc.fma(a, a, -1.0) == 2.0 ** -29 + 2.0 ** -60 != a * a - 1.0
    assert math.isnan(lc.fma(lc.INF, 0.0, 1.0)) and math.isnan(lc.fma(lc.INF, 1.0, -lc.INF))
    assert lc.fma(lc.INF, -1.0, 5.0) == -lc.INF and lc.fma(2.0, 3.0, lc.INF) == lc.INF
    assert lc.fma(1e200, 1e200, 0.0) == lc.INF and lc.fma(-1e200, 1e200, 1e300) == -lc.INF
    z = lambda x: math.copysign(1.0, x)                            # noqa: E731
    assert z(lc.fma(0.0, -1.0, 0.0)) == 1 and z(lc.fma(0.0, -1.0, -0.0)) == -1
    assert z(lc.fma(-0.0, 5.0, -0.0)) == -1 and lc.fma(2.0, 3.0, -6.0) == 0 and z(lc.fma(2.0, 3.0, -6.0)) == 1
    tiny = lc.fma(-5e-324, 0.25, 0.0)
    assert tiny == 0 and z(tiny) == -1                             # underflow keeps the sign
    assert lc.fma(5e-324, 0.75, 0.0) == 5e-324


def test_foreach_step_by_hand():
    """Dyadic inputs, every operation exact, worked out by hand.
    lr .5, beta1 .25 (weight .75: the large lerp form), beta2 .75, eps 2, t = 1, p 1, g 2:
      m = g - (g - 0) * (1 - .75) = 1.5;  v = .25 * 4 + 0 = 1;  bc2s = sqrt(.25) = .5;
      den = 1 / .5 + 2 = 4;  step = -(.5 / .75) (one rounding);  p' = fma(step, .375, 1).
    beta1 .75 (weight .25: the small form): m = 0 + .25 * 2 = .5; step = -(.5 / .25) = -2;
      p' = 1 - 2 * (.5 / 4) = .75.
    With p = -1, c_neg = .5, wd = .25 and beta1 .75: g = 2 - .5 = 1.5, then 1.5 + .25 * -1 =
      1.25; m = .3125; v = .25 * 1.5625 = .390625, sqrt = .625; den = 1.25 + 2 = 3.25;
      p' = fma(-2, .3125 / 3.25, -1)."""
    h = {'lr': 0.5, 'beta1': 0.25, 'beta2': 0.75, 'eps': 2.0, 'wd': 0.0}
    p, m, v = lc.foreach_step_ref(1.0, 2.0, 0.0, 0.0, h, 1, None)
    assert (m, v) == (1.5, 1.0)
    assert p == float(Fraction(1) + Fraction(-(0.5 / 0.75)) * Fraction(0.375))
    h['beta1'] = 0.75
    assert lc.foreach_step_ref(1.0, 2.0, 0.0, 0.0, h, 1, None) == (0.75, 0.5, 1.0)
    assert lc.foreach_step_ref(1.0, 2.0, 0.0, 0.0, h, 1, 0.5) == (0.75, 0.5, 1.0)   # p > 0
    h['wd'] = 0.25
    p, m, v = lc.foreach_step_ref(-1.0, 2.0, 0.0, 0.0, h, 1, 0.5)
    assert (m, v) == (0.3125, 0.390625)
    assert p == float(Fraction(-1) - 2 * Fraction(0.3125 / 3.25))
    # second step: the moments enter, the bias corrections move
    h = {'lr': 0.5, 'beta1': 0.75, 'beta2': 0.75, 'eps': 2.0, 'wd': 0.0}
    p, m, v = lc.foreach_step_ref(0.75, 4.0, 0.5, 1.0, h, 2, None)
    assert (m, v) == (0.5 + 0.25 * 3.5, 0.25 * 16 + 0.75)
    den = math.sqrt(4.75) / (1 - 0.75 ** 2.0) ** 0.5 + 2.0
    assert p == lc.fma(-(0.5 / (1 - 0.75 ** 2.0)), m / den, 0.75)
    # specials by the IEEE rules
    p, m, v = lc.foreach_step_ref(-0.0, 0.0, 0.0, 0.0, HYPER, 1, 0.3)
    assert (p, m, v) == (0.0, 0.0, 0.0) and math.copysign(1, p) == -1   # -0 is not < 0; -0 + -0*0
    p, m, v = lc.foreach_step_ref(1.0, 1e160, 0.0, 1e300, HYPER, 1, None)
    assert v == lc.INF and m == lc.fma(1 - 0.9, 1e160, 0.0) and p == 1.0   # m / inf = 0
    assert all(math.isnan(x) for x in lc.foreach_step_ref(lc.NAN, 1.0, 0.0, 0.0, HYPER, 1, 0.3)[:1])
    assert all(math.isnan(x) for x in lc.foreach_step_ref(1.0, lc.INF, 0.0, 0.0, HYPER, 1, None)[0:1])


@pytest.mark.parametrize('n', [n for n in lc.LENGTHS if n >= 255])
def test_emulator_tells_the_documented_forms_from_their_neighbours(n):
    """On the random sample at step 1, the unfused second moment and the large-weight lerp each
    differ from the documented result on at least 8 elements: a kernel that used either would
    not pass the emulator's check.  (Every length with 8 random elements to its sample, at the
    seed test_gpu_loop_kernels.py uses: the length itself.)"""
    inp = lc.adam_inputs(n, seed=n)
    samp = lc.sample_indices(n, inp['special'], seed=n)
    rand = np.setdiff1d(samp, inp['special'])
    assert len(samp) <= 512 and len(rand) >= 100
    g = inp['g'][0]
    for form in ('unfused_v', 'lerp_large'):
        diff = 0
        for i in rand:
            args = (float(inp['p'][i]), float(g[i]), float(inp['m'][i]), float(inp['v'][i]), HYPER, 1, 0.3)
            diff += lc.foreach_step_ref(*args) != lc.foreach_step_ref(*args, form=form)
        assert diff >= 8, (form, diff)
    # and with the large weight (beta1 = 0.3) the large form is the documented one
    h = dict(HYPER, beta1=0.3)
    i = int(rand[0])
    args = (float(inp['p'][i]), float(g[i]), 0.0, 0.0, h, 1, None)
    assert lc.foreach_step_ref(*args) == lc.foreach_step_ref(*args, form='lerp_large')
