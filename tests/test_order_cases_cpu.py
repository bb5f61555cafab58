"""What makes tests/test_gpu_order_fuzz.py meaningful, checked on the CPU alone.

Coverage: the cases of order_cases.py, under their env, make the trace-order layer take every
one of its decisions (view tiles with tw = 2 and tw = 1, tv = 64, a tv that is neither the view
count nor 64, no tile for a prime view count / fewer than 8 views / a dynamic grid, wedges with
and without a remainder, no wedge for a narrow detector / a mixed collection, a forced and a
refused vtile: request).  This asserts that the decisions occur, not that they are right.

Sensitivity: on the oracle's reference forward alone, swapping any two adjacent views, detector
rows or detector columns — or pairing a view with a neighbouring time slice — changes some
element by more than 100 x the loosest tolerance the GPU test compares forwards with (float32's
gc.F32_RTOL; the float64 bound is 1e5 times tighter), relative to max|y|.  A forward whose rows
are permuted, or paired with the wrong slice, then cannot pass.  At most half of a case's rays
may miss the grid.
"""
import numpy as np
import pytest

import golden_cases as gc
import order_cases as oc

MARGIN = 100 * gc.F32_RTOL


def test_cases_cover_every_decision():
    seen = set()
    for case in oc.CASES:
        tiles, wedge = oc.decisions(case)
        shape, env = case.shape, case.env or ''
        orbit = len(shape) == 3
        v, w = (shape[0] if orbit else 1), shape[-1]
        if tiles is not None:
            tv, tw = tiles
            assert v % tv == 0 and w % tw == 0 and wedge is None
            if env.startswith('vtile:'):
                seen.add('forced vtile')
                continue
            seen.add(f'tile tw={tw}')
            if tv == 64:
                seen.add('tv=64')
            elif tv != v:
                seen.add('tv neither V nor 64')
        elif orbit and env.startswith('vtile:'):
            seen.add('refused vtile')
        elif orbit and case.dynamic:
            seen.add('no tile: dynamic')
        elif orbit and not env and case.kind != 'parallel':
            if v < 8:
                seen.add('no tile: V < 8')
            elif v > 64 and all(v % d for d in range(2, v)):
                seen.add('no tile: prime V')
        if wedge is not None:
            assert sorted(wedge.tolist()) == list(range(shape[-2] * w))
            seen.add('wedge w%3==0' if w % 3 == 0 else 'wedge w%3!=0')
        elif tiles is None and not env:
            if case.kind == 'circ' and w <= 3:
                seen.add('no wedge: w <= 3')
            if case.kind == 'mixed':
                seen.add('no wedge: mixed')
    want = {'tile tw=2', 'tile tw=1', 'tv=64', 'tv neither V nor 64', 'no tile: prime V',
            'no tile: V < 8', 'no tile: dynamic', 'wedge w%3==0', 'wedge w%3!=0',
            'no wedge: w <= 3', 'no wedge: mixed', 'forced vtile', 'refused vtile'}
    assert want <= seen, sorted(want - seen)


def test_case_sizes():
    for case in oc.CASES:
        grid, geom, _ = oc.build(case)
        assert tuple(geom.shape) == case.shape
        assert int(np.prod(geom.shape)) <= 6000
        nr, ne, na = grid.shape[-3:]
        assert nr * ne * na < 2000 and all(6 <= n <= 12 for n in (nr, ne, na))
        assert 2 * (nr + 1) + 2 * (ne + 1) + (na + 1) + 1 < 128
        assert bool(grid.dynamic) == case.dynamic
        if case.dynamic:
            assert grid.shape[0] == case.shape[0]


def _changed(a, b, scale):
    return float(np.abs(a - b).max()) > MARGIN * scale


@pytest.mark.parametrize('name', oc.NAMES)
def test_reference_is_sensitive_to_every_adjacent_swap(name):
    ref = oc.reference(name)
    y = ref.y
    scale = float(np.abs(y).max())
    assert scale > 0.1
    assert float(np.mean(np.diff(ref.segs[0]) == 0)) <= 0.5, 'too many rays miss the grid'
    assert float(np.mean(y == 0)) <= 0.5
    for axis, what in zip(range(y.ndim - 1, -1, -1), ('columns', 'rows', 'views')):
        for i in range(y.shape[axis] - 1):
            a, b = np.take(y, i, axis), np.take(y, i + 1, axis)
            assert _changed(a, b, scale), f'{name}: swapping {what} {i} and {i + 1} changes nothing'
    if oc.BY_NAME[name].dynamic:
        n = y.shape[0]
        for v in range(n):
            for t in (v - 1, v + 1):
                if 0 <= t < n:
                    other = oc.view_forward(ref, v, ref.x[t]).reshape(y.shape[1:])
                    assert _changed(y[v], other, scale), f'{name}: view {v} on slice {t}'


@pytest.mark.parametrize('name', oc.NAMES)
def test_reference_adjoint_is_the_transpose(name):
    """<A x, yt> = <x, A^T yt> on the oracle's own numbers: the forward and the adjoint of a
    reference pair the same rays (and, dynamic, the same slices)."""
    ref = oc.reference(name)
    lhs, rhs = float((ref.y * ref.yt).sum()), float((ref.x * ref.xt).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
