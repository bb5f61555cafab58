"""The exact path's sort emulations, run directly on the adversarial lists of sort_cases.py
(sphrt_exact_sort_lists) and held to the CPU oracle's introsort.

The traced tests reach this code only through rays, whose lists are benign where it branches;
here every list family reaches the depth limit from K = 121 on (test_sort_cases_cpu.py), in three
payload settings that fix which branch exact_heap_range must take:

    serial (AOS over global memory, SoA over LDS)   permutation and distances == oracle, bit for bit
    wave (one wave, four waves)                     distances == oracle; rank-sorted + heap-sorted
                                                    ranges == the oracle's depth-limit ranges;
        conflict    heap-sorted == ranges with a live tie, permutation == oracle
        noconflict  heap-sorted == 0, walk replay == oracle's, permutation == oracle outside ranges
        mixed       counters == the host's entries_conflict verdict per range, replay, outside
      four waves == one wave, bit for bit
    network (reference mode's register sort)        accepted => truly sorted and the oracle's
                                                    replay; refuses NaN, live conflicting ties and
                                                    key collisions; accepts the no-conflict
                                                    float32-valued lists

Outputs sit between guard elements.  Every case prints its oracle range count and the device's
two counters (pytest -s shows them)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch as tr

import sort_cases as sc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from oracle import oracle  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
INF = np.inf
BASE_K = (1, 2, 16, 17, 33, 63, 64, 65, 121, 128, 256, 257, 512, 513, 1024)
WAVE_K = BASE_K + ('max_wave4', 'max_wave1')
SERIAL_K = BASE_K + ('max_wave4', 'max_wave1')
NETWORK_K = tuple(k for k in BASE_K if 2 <= k <= 512)
PAY_SENTINEL = 0xDEADBEEF


def _L():
    from sph_raytracer_amd import _lib
    return _lib


def max_k(method):
    return int(_L().load().sphrt_exact_sort_max_k(method))


def resolve_k(K):
    lib = _L()
    return {'max_wave1': lambda: max_k(lib.SORT_WAVE1), 'max_wave4': lambda: max_k(lib.SORT_WAVE4),
            'max_network': lambda: max_k(lib.SORT_NETWORK)}[K]() if isinstance(K, str) else K


def sort_lists(L, method, invalid=False, gpu='cuda:0'):
    """sphrt_exact_sort_lists on the lists L -> (t_out, order, region field, info) on the host;
    the outputs lie between guards, which are checked."""
    lib_mod = _L()
    lib = lib_mod.load()
    dev = tr.device(gpu)
    n, K = L.n, L.K
    t = tr.from_numpy(L.t).to(dev)
    reg = tr.from_numpy(L.reg).to(dev)
    start = tr.from_numpy(L.start).to(dev)
    tbuf = tr.full((2 * GUARD + n * K,), float('nan'), dtype=tr.float64, device=dev)
    pbuf = tr.full((2 * GUARD + n * K,), PAY_SENTINEL - (1 << 32), dtype=tr.int32, device=dev)
    ibuf = tr.full((2 * GUARD + n * lib_mod.SORT_INFO_FIELDS,), -7, dtype=tr.int64, device=dev)
    need = lib.sphrt_exact_sort_workspace_bytes(method, n, K)
    ws = tr.empty(max(need, 1), dtype=tr.uint8, device=dev)
    lib_mod.check(lib.sphrt_exact_sort_lists(
        lib_mod.ptr(t), lib_mod.ptr(reg), lib_mod.ptr(start), n, K, L.nbr, L.nbe, method,
        int(invalid), lib_mod.ptr(tbuf[GUARD:]), lib_mod.ptr(pbuf[GUARD:]),
        lib_mod.ptr(ibuf[GUARD:]), lib_mod.ptr(ws), need, lib_mod.stream_of(dev)),
        'sphrt_exact_sort_lists')
    tr.cuda.synchronize(dev)
    th, ph, ih = tbuf.cpu().numpy(), pbuf.cpu().numpy().view(np.uint32), ibuf.cpu().numpy()
    assert np.isnan(th[:GUARD]).all() and np.isnan(th[-GUARD:]).all(), 'distance guards written'
    assert (ph[:GUARD] == PAY_SENTINEL).all() and (ph[-GUARD:] == PAY_SENTINEL).all()
    assert (ih[:GUARD] == -7).all() and (ih[-GUARD:] == -7).all(), 'info guards written'
    pay = ph[GUARD:-GUARD].reshape(n, K)
    return (th[GUARD:-GUARD].reshape(n, K), (pay >> 16).astype(np.int64),
            (pay & 0xffff).astype(np.int64) - 2, ih[GUARD:-GUARD].reshape(n, -1))


@functools.lru_cache(maxsize=None)
def host(K):
    """The lists at K in the three settings and the oracle's verdict on each list (the same
    distances in every setting): (sorted distances, permutation, depth-limit ranges)."""
    cases = sc.cases(K, n_random=12 if K <= 1024 else 6)
    ref = [oracle.introsort_ranges(x) for x in cases['conflict'].t]
    return cases, ref


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_written(L, ts, order, regf):
    """Every output was written and is a permutation of its list with the payloads intact."""
    assert not np.isnan(ts).any(), 'a distance was not written'
    for i in range(L.n):
        assert np.array_equal(np.sort(order[i]), np.arange(L.K)), f'{L.names[i]}: not a permutation'
        assert np.array_equal(bits(ts[i]), bits(L.t[i][order[i]])), L.names[i]
        assert np.array_equal(regf[i], L.reg[i][order[i]]), L.names[i]


# ---- serial ------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['SERIAL_AOS', 'SERIAL_SOA'])
@pytest.mark.parametrize('K', SERIAL_K)
def test_serial_vs_oracle(K, method, gpu):
    K = resolve_k(K)
    cases, ref = host(K)
    m = getattr(_L(), 'SORT_' + method)
    for setting, L in cases.items():
        ts, order, regf, info = sort_lists(L, m, gpu=gpu)
        check_written(L, ts, order, regf)
        assert not info.any()
        for i, (rt, ridx, _) in enumerate(ref):
            assert np.array_equal(order[i], ridx), f'{setting} {L.names[i]} K={K}: permutation'
            assert np.array_equal(bits(ts[i]), bits(rt)), f'{setting} {L.names[i]} K={K}'


@pytest.mark.parametrize('K', ['lds+1', 2500, 'max'])
def test_serial_aos_above_the_lds_limit(K, gpu):
    """The global-memory sort at K no LDS method holds, up to its own limit (two pool lists there:
    one lane sorts 65536 entries in about a second)."""
    lib = _L()
    big = K == 'max'
    K = {'lds+1': max_k(lib.SORT_WAVE1) + 1, 'max': max_k(lib.SORT_SERIAL_AOS)}.get(K, K)
    rng = np.random.default_rng(K)
    if big:
        t = np.stack([sc.pool(K, rng) for _ in range(2)])
    else:
        t = np.stack([sc.organ_pipe(K), sc.organ_pipe(K, 2, K // 3), sc.killer(K, 2),
                      sc.pool(K, rng), sc.trace_like(K, rng)])
    L = sc.payloads('conflict', t, [str(i) for i in range(len(t))])
    ts, order, regf, _ = sort_lists(L, lib.SORT_SERIAL_AOS, gpu=gpu)
    n_ranges = 0
    for i, x in enumerate(t):
        rt, ridx, rg = oracle.introsort_ranges(x)
        n_ranges += len(rg)
        assert np.array_equal(order[i], ridx) and np.array_equal(bits(ts[i]), bits(rt)), i
        assert np.array_equal(regf[i], L.reg[i][order[i]])
    print(f'serial AOS K={K}: {len(t)} lists, oracle depth-limit ranges {n_ranges}')
    assert big or n_ranges >= 1


# ---- wave --------------------------------------------------------------------------------------
@pytest.mark.parametrize('invalid', [False, True], ids=['masked', 'invalid'])
@pytest.mark.parametrize('K', WAVE_K)
def test_wave_vs_oracle(K, invalid, gpu):
    lib = _L()
    K = resolve_k(K)
    cases, ref = host(K)
    four = K <= max_k(lib.SORT_WAVE4)
    for setting, L in cases.items():
        ts, order, regf, info = sort_lists(L, lib.SORT_WAVE1, invalid, gpu)
        check_written(L, ts, order, regf)
        assert not info[:, 2:].any()
        if four:
            ts4, order4, regf4, info4 = sort_lists(L, lib.SORT_WAVE4, invalid, gpu)
            assert np.array_equal(bits(ts4), bits(ts)), f'{setting} K={K}: four waves != one wave'
            assert np.array_equal(order4, order) and np.array_equal(regf4, regf)
            assert np.array_equal(info4, info)
        n_ranges = n_tied = n_amb = n_inf = 0
        for i, (rt, ridx, rg) in enumerate(ref):
            who = f'{setting} {L.names[i]} K={K} invalid={invalid}'
            assert np.array_equal(bits(ts[i]), bits(rt)), who + ': distances'
            tied = sum(sc.range_has_live_tie(rt, f, l, invalid) for f, l in rg)
            amb = sum(sc.range_is_ambiguous(rt, ridx, f, l, L, i, invalid) for f, l in rg)
            n_ranges, n_tied, n_amb = n_ranges + len(rg), n_tied + tied, n_amb + amb
            n_inf += sum(int((rt[f:l] == INF).sum() >= 2) for f, l in rg)
            assert info[i, 0] + info[i, 1] == len(rg), who + ': depth-limit ranges'
            assert info[i, 1] == amb, who + ': heap-sorted ranges'
            out = sc.outside(K, rg)
            assert np.array_equal(order[i][out], ridx[out]), who + ': order outside the ranges'
            if setting == 'conflict':
                # every live tie conflicts: the whole permutation is the oracle's, but for ranges
                # whose ties are all dead (negative distances, masked +inf), which are rank-sorted
                assert amb == tied, who
                exact = sc.outside(K, [(f, l) for f, l in rg
                                       if not sc.range_has_live_tie(rt, f, l, invalid)])
                assert np.array_equal(order[i][exact], ridx[exact]), who + ': permutation'
            if setting == 'noconflict' and not invalid:
                assert info[i, 1] == 0, who
            assert sc.replay(ts[i], order[i], L, i, invalid) == sc.replay(rt, ridx, L, i, invalid), \
                who + ': walk replay'
        print(f'wave K={K} {setting} invalid={int(invalid)}: oracle ranges {n_ranges} (live tie '
              f'{n_tied}, ambiguous {n_amb}, two +inf {n_inf}); device rank-sorted '
              f'{int(info[:, 0].sum())} heap-sorted {int(info[:, 1].sum())}'
              f'{"" if four else " (one wave only)"}')
        assert info[:, 0].sum() + info[:, 1].sum() == n_ranges
        if setting == 'conflict':
            assert info[:, 1].sum() == n_tied
            if K >= 121:
                assert info[:, 1].sum() >= 1, 'the heapsort branch did not run'
        if setting == 'noconflict':
            # (invalid: two +inf in a range are ambiguous whatever they write)
            assert info[:, 1].sum() == (n_inf if invalid else 0)
            if K >= 121:
                assert info[:, 0].sum() >= 1, 'the rank sort did not run'
        if invalid and K in sc.INF_IN_RANGE:
            assert n_inf >= 1


# ---- network -----------------------------------------------------------------------------------
def check_network(L, ref, ts, order, regf, info, what):
    n_acc = 0
    for i, (rt, ridx, _) in enumerate(ref):
        who = f'{what} {L.names[i]}'
        assert info[i, 2] in (0, 1)
        x = L.t[i]
        groups = np.split(np.arange(L.K), np.flatnonzero(rt[1:] != rt[:-1]) + 1)
        conflict = any(len(g) > 1 and sc.live(rt[g[0]], False) and
                       sc.range_is_ambiguous(rt, ridx, g[0], g[-1] + 1, L, i, False)
                       for g in groups)
        if conflict:
            assert info[i, 2] == 0, who + ': accepted a live conflicting tie'
        if not info[i, 2]:
            assert np.isnan(ts[i]).all(), who + ': a refused list was written'
            continue
        n_acc += 1
        stable = np.argsort(x + 0.0, kind='stable')
        assert np.array_equal(order[i], stable), who + ': not sorted by (distance, position)'
        assert np.array_equal(bits(ts[i]), bits(x[stable])), who
        assert np.array_equal(regf[i], L.reg[i][stable]), who
        assert sc.replay(ts[i], order[i], L, i)[0] == sc.replay(rt, ridx, L, i)[0], \
            who + ': walk replay'
    return n_acc


@pytest.mark.parametrize('K', NETWORK_K + ('max_network',))
def test_network(K, gpu):
    lib = _L()
    K = resolve_k(K)
    cases, ref = host(K)
    for setting, L in cases.items():
        ts, order, regf, info = sort_lists(L, lib.SORT_NETWORK, gpu=gpu)
        assert not info[:, [0, 1, 3]].any()
        n_acc = check_network(L, ref, ts, order, regf, info, f'{setting} K={K}')
        f32 = np.array([sc.is_float32_valued(x) for x in L.t])
        print(f'network K={K} {setting}: accepted {n_acc} of {L.n} ({int(f32.sum())} float32-valued)')
        if setting == 'noconflict':
            assert f32.sum() >= L.n // 2
            assert info[f32, 2].all(), 'refused a float32-valued list without a conflict'
        if setting == 'conflict':
            # every list with a finite non-negative tie conflicts
            tie = np.array([sc.range_has_live_tie(rt, 0, K, False) for rt, _, _ in ref])
            assert not info[tie, 2].any() and tie.any()


def test_network_refuses_nan_and_key_collisions(gpu):
    lib = _L()
    K = max_k(lib.SORT_NETWORK)
    base = np.arange(K, dtype=np.float64) / 4 + 1.0          # float32-valued, strictly ascending
    nan = base.copy()
    nan[K // 3] = np.nan
    # two distances one ulp apart, the larger first: the composite keys (the distance's bits
    # above the 9 index bits) agree, so the key sort orders them by position, against the truth
    lo = 37.0
    collide = base + 100.0
    collide[5], collide[K - 7] = np.nextafter(lo, INF), lo
    ascending = base + 100.0
    ascending[5], ascending[K - 7] = lo, np.nextafter(lo, INF)   # the same pair in list order
    t = np.stack([base, nan, collide, ascending])
    L = sc.payloads('noconflict', t, ['base', 'nan', 'collide', 'ascending'])
    ts, order, regf, info = sort_lists(L, lib.SORT_NETWORK, gpu=gpu)
    assert info[:, 2].tolist() == [1, 0, 0, 1]
    assert np.isnan(ts[1]).all() and np.isnan(ts[2]).all()
    for i in (0, 3):
        stable = np.argsort(t[i], kind='stable')
        assert np.array_equal(order[i], stable) and np.array_equal(bits(ts[i]), bits(t[i][stable]))


# ---- refusals ----------------------------------------------------------------------------------
def test_k_limits_are_refused_not_launched(gpu):
    lib_mod = _L()
    lib = lib_mod.load()
    dev = tr.device(gpu)
    buf = tr.zeros(16, dtype=tr.float64, device=dev)       # far too small: must not be touched
    methods = ('SERIAL_AOS', 'SERIAL_SOA', 'WAVE1', 'WAVE4', 'NETWORK')
    limits = {m: max_k(getattr(lib_mod, 'SORT_' + m)) for m in methods}
    print(f'largest K per method: {limits}')
    assert limits['NETWORK'] == 512 and limits['SERIAL_AOS'] == 1 << 16
    assert limits['WAVE4'] < limits['WAVE1'] == limits['SERIAL_SOA'] < 1815
    assert lib.sphrt_exact_sort_max_k(99) == -1

    def call(method, K, n=1):
        return lib.sphrt_exact_sort_lists(
            lib_mod.ptr(buf), lib_mod.ptr(buf), lib_mod.ptr(buf), n, K, 1, 1, method, 0,
            lib_mod.ptr(buf), lib_mod.ptr(buf), lib_mod.ptr(buf), lib_mod.ptr(buf), 1 << 40,
            lib_mod.stream_of(dev))

    for m in methods:
        code = getattr(lib_mod, 'SORT_' + m)
        for K in (limits[m] + 1, 0, -1):
            assert call(code, K) != 0, f'{m} K={K} was not refused'
            assert b'entries' in lib.sphrt_last_error()
    assert call(lib_mod.SORT_NETWORK, 1) != 0          # the composite key needs an index bit
    assert call(99, 8) != 0 and call(lib_mod.SORT_WAVE1, 8, n=-1) != 0
    tr.cuda.synchronize(dev)
    assert not buf.any()
