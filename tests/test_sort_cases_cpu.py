"""The lists of sort_cases.py do what tests/test_gpu_exact_sort.py needs them for, on the CPU:
the instrumented oracle (oracle.introsort_ranges) finds depth-limit ranges with live ties at every
K where the GPU cases are meant to reach the heapsort branch, the payload settings make the
expected branch known, the walk replay is right on hand-written lists, and the oracle's sort is
torch.sort on these families too."""
import os
import sys

import numpy as np
import pytest
import torch as tr

import sort_cases as sc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from oracle import oracle  # noqa: E402

INF = np.inf
# the K of the GPU cases from the smallest that reaches the depth limit (2 floor(log2 K) partition
# levels) on; 1733 and 1798 are the largest lists four waves / one wave hold in LDS
DEPTH_K = (121, 128, 256, 257, 512, 513, 1024, 1733, 1798)
SMALL_K = (1, 2, 16, 17, 33, 63, 64, 65)


def _sorted(K):
    out = {}
    for name, lists in sc.families(K).items():
        out[name] = [oracle.introsort_ranges(x) for x in lists]
    return out


@pytest.mark.parametrize('K', DEPTH_K)
def test_families_reach_the_depth_limit(K):
    """Pipes and killers reach the depth limit at every K of DEPTH_K, every such range holds a
    live tie, and the pool and the small families never get there."""
    res = _sorted(K)
    count = {name: sum(len(r[2]) for r in v) for name, v in res.items()}
    print(f'K={K}: depth-limit ranges per family {count}')
    assert count['pipe'] >= 1 and count['killer'] >= 1
    assert count['pool'] == 0 and count['equal'] == 0 and count['few'] == 0
    for name in ('pipe', 'killer'):
        tied = [sc.range_has_live_tie(ts, f, l, False) for ts, _, rg in res[name] for f, l in rg]
        assert any(tied), name


@pytest.mark.parametrize('K', SMALL_K)
def test_small_lists_stay_above_the_depth_limit(K):
    assert all(len(r[2]) == 0 for v in _sorted(K).values() for r in v)


@pytest.mark.parametrize('K', DEPTH_K)
def test_settings_fix_the_branch(K):
    """conflict: a range is ambiguous exactly when it holds a live tie, and some range is;
    noconflict: no range is ambiguous although some hold live ties."""
    cases = sc.cases(K)
    n_amb = {s: 0 for s in sc.SETTINGS}
    n_tied = 0
    for i, x in enumerate(cases['conflict'].t):
        ts, idx, rg = oracle.introsort_ranges(x)
        for f, l in rg:
            tied = sc.range_has_live_tie(ts, f, l, False)
            n_tied += tied
            for s in sc.SETTINGS:
                amb = sc.range_is_ambiguous(ts, idx, f, l, cases[s], i, False)
                n_amb[s] += amb
                if s == 'conflict':
                    assert amb == tied
                if s == 'noconflict':
                    assert not amb
    print(f'K={K}: ranges with a live tie {n_tied}, ambiguous {n_amb}')
    assert n_tied >= 1 and n_amb['conflict'] == n_tied and n_amb['noconflict'] == 0


@pytest.mark.parametrize('K', sorted(sc.INF_IN_RANGE))
def test_infinite_ties_inside_a_range(K):
    """The lists of INF_IN_RANGE: a depth-limit range with two or more +inf, ambiguous under
    invalid=True in every setting and, without it, not for their sake."""
    L = sc.cases(K)['noconflict']
    hits = 0
    for q, m in sc.INF_IN_RANGE[K]:
        x = sc.top_misses(sc.organ_pipe(K, q), m)
        i = next(j for j in range(L.n) if np.array_equal(L.t[j], x))
        ts, idx, rg = oracle.introsort_ranges(x)
        both = [(f, l) for f, l in rg if (ts[f:l] == INF).sum() >= 2]
        assert both, (q, m)
        for f, l in both:
            assert sc.range_is_ambiguous(ts, idx, f, l, L, i, True)
            assert not sc.range_is_ambiguous(ts, idx, f, l, L, i, False)
        hits += len(both)
    assert hits >= len(sc.INF_IN_RANGE[K])


def test_ranges_variant_is_the_same_sort():
    for K in (17, 128, 513, 1024):
        for lists in sc.families(K).values():
            for x in lists:
                t0, i0 = oracle.introsort(x)
                t1, i1, rg = oracle.introsort_ranges(x)
                assert np.array_equal(i0, i1) and np.array_equal(t0, t1, equal_nan=False)
                assert all(0 <= f < l <= K and l - f > 16 for f, l in rg)


@pytest.mark.parametrize('K', SMALL_K + DEPTH_K)
def test_oracle_is_torch_sort_on_the_families(K):
    """torch.sort (CPU) == the oracle's introsort on every family, heapsorted ranges included."""
    for name, lists in sc.families(K).items():
        for j, x in enumerate(lists):
            _, ref = tr.from_numpy(x.copy()).sort()
            _, got = oracle.introsort(x)
            assert np.array_equal(ref.numpy(), got), f'{name}[{j}] K={K}'


def test_families_are_what_they_say():
    K = 64
    fam = sc.families(K)
    p = fam['pipe'][0]
    h = (K + 1) // 2
    assert (np.diff(p[:h]) > 0).all() and (np.diff(p[h:]) < 0).all()
    assert (fam['equal'] == fam['equal'][:, :1]).all()
    assert all(len(np.unique(x)) <= 2 for x in fam['few'])
    assert any((np.diff(x) >= 0).all() for x in fam['few'])
    assert any((np.diff(x) <= 0).all() for x in fam['few'])
    for x in fam['trace']:
        assert x[-1] == 0.0 and sc.is_float32_valued(x) and (x == INF).any()
    pool = fam['pool']
    assert (pool == INF).any() and (pool == -INF).any() and (pool < 0).any()
    assert np.signbit(pool[pool == 0]).any() and not np.signbit(pool[pool == 0]).all()
    c = sc.cases(K)
    L = c['conflict']
    assert 2 * L.nbr >= K - 1 and len(set(L.reg[0])) == K
    assert (c['noconflict'].reg == 3).all() and (c['noconflict'].start == 3).all()
    M = c['mixed']
    assert (M.reg[:, :2 * M.nbr] != sc.NO_UPDATE).all() and (M.reg == sc.NO_UPDATE).any()


# ---- the walk replay on hand-written lists ------------------------------------------------------
def _lists(t, reg, start, nbr, nbe):
    return sc.Lists(np.array([t], np.float64), np.array([reg]), np.array([start]), nbr, nbe, ['x'])


def test_replay_by_hand():
    # K = 6: entries 0, 1 sphere (nbr = 1), 2, 3 cone (nbe = 1), 4 plane, 5 the start entry
    L = _lists([1.0, 2.0, 1.0, INF, -1.0, 0.0], [7, 8, 5, 6, 4, 0], [1, 2, 3], 1, 1)
    order = [4, 5, 0, 2, 1, 3]
    ts = L.t[0][order]
    states, inf_order = sc.replay(ts, order, L, 0)
    # t = -1 updates nothing; the start entry sets (1, 2, 3); t = 1: r = 7 and e = 5; t = 2: r = 8;
    # the +inf entry is past what a masked walk reads
    assert states == [(-1.0, 1, 2, 3), (0.0, 1, 2, 3), (1.0, 7, 5, 3), (2.0, 8, 5, 3)]
    assert inf_order is None
    # the two t = 1 entries write different rows: either order, the same states
    assert sc.replay(L.t[0][[4, 5, 2, 0, 1, 3]], [4, 5, 2, 0, 1, 3], L, 0)[0] == states
    assert not sc.entries_conflict(0, 2, L, 0)
    states_inv, inf_order = sc.replay(ts, order, L, 0, invalid=True)
    assert states_inv == states + [(INF, 8, 6, 3)] and inf_order == [3]


def test_replay_sees_a_conflict_and_no_update():
    # two sphere entries at t = 1 with different regions: the order decides the state
    L = _lists([1.0, 1.0, 3.0, 0.0], [7, 8, sc.NO_UPDATE, 0], [1, 2, 3], 1, 0)
    assert sc.entries_conflict(0, 1, L, 0)
    a = sc.replay(L.t[0][[3, 0, 1, 2]], [3, 0, 1, 2], L, 0)[0]
    b = sc.replay(L.t[0][[3, 1, 0, 2]], [3, 1, 0, 2], L, 0)[0]
    assert a == [(0.0, 1, 2, 3), (1.0, 8, 2, 3), (3.0, 8, 2, 3)]      # entry 2: "no update"
    assert b == [(0.0, 1, 2, 3), (1.0, 7, 2, 3), (3.0, 7, 2, 3)]
    # the start entry conflicts with a sphere entry of another region, not with its own
    L2 = _lists([0.0, 0.0, 0.0], [1, 9, 0], [1, 2, 3], 1, 0)
    assert not sc.entries_conflict(0, 2, L2, 0) and sc.entries_conflict(1, 2, L2, 0)
    # -0.0 and 0.0 are one group; the states carry +0.0
    L3 = _lists([-0.0, 0.0], [5, 0], [1, 2, 3], 1, 0)
    assert sc.replay(L3.t[0], [0, 1], L3, 0)[0] == [(0.0, 1, 2, 3)]
    assert sc.replay(L3.t[0][::-1], [1, 0], L3, 0)[0] == [(0.0, 5, 2, 3)]


def test_replay_invalid_keeps_the_infinite_order():
    L = _lists([INF, INF, 0.0], [7, 8, 0], [1, 2, 3], 1, 0)
    a = sc.replay(L.t[0][[2, 0, 1]], [2, 0, 1], L, 0, invalid=True)
    b = sc.replay(L.t[0][[2, 1, 0]], [2, 1, 0], L, 0, invalid=True)
    assert a[1] == [0, 1] and b[1] == [1, 0] and a[0][-1] == (INF, 8, 2, 3)
    assert sc.replay(L.t[0][[2, 0, 1]], [2, 0, 1], L, 0)[0] == [(0.0, 1, 2, 3)]
    ts = np.array([0.0, INF, INF])
    assert sc.range_is_ambiguous(ts, [2, 0, 1], 0, 3, L, 0, True)
    assert not sc.range_is_ambiguous(ts, [2, 0, 1], 0, 3, L, 0, False)
    assert sc.outside(5, [(1, 3)]).tolist() == [True, False, False, True, True]
