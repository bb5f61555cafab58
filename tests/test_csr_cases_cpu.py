"""The synthetic CSR cases (csr_cases.py) without a GPU: the numpy restatements are consistent
with one another on every case, and sphrt_forward_plan (host code) chooses, for every case and
both element sizes, the forward kernel the case was designed for — the matrix reaches every
branch of the plan.  The GPU suite (test_gpu_csr_synthetic.py) runs the same cases."""
import ctypes

import numpy as np
import pytest

import csr_cases as cc

NAMES = list(cc.CASES)
PLAN_FIELDS = ('mode', 'tab_bytes', 'edma', 'runs', 'half', 'dense', 'early_rounds', 'fallback')


def _restated(name):
    c = cc.make(name)
    ix = cc.index_ref(c.n_rays, c.row_ptr, c.ray_ids)
    return c, ix, cc.tables_ref(ix['blocks'], c.vox, ix['heads'])


@pytest.mark.parametrize('name', NAMES)
def test_restatements_are_consistent(name):
    """Every non-empty row is owned by exactly one block, the empty shares partition the list,
    the stride is in the range the case was designed for, and transposing twice returns the CSR
    (each row stably sorted by column)."""
    c, ix, t = _restated(name)
    total = int(c.row_ptr[-1])
    b = ix['blocks']
    assert len(b) == total // cc.SPB + 1
    # blocks tile the segments in order: each non-empty row starts in exactly one [s0, s1)
    assert b[0, 2] == 0 and b[-1, 3] == total and (b[1:, 2] == b[:-1, 3]).all()
    assert (b[:, 2] <= b[:, 3]).all()
    heads = ix['heads']
    owner = np.searchsorted(b[:, 3], heads, side='right')
    assert ((b[owner, 2] <= heads) & (heads < b[owner, 3])).all()
    assert (heads // cc.SPB == owner).all()            # the block of the window the row starts in
    # row_lo counts the rows of the earlier blocks
    assert np.array_equal(b[:, 4], np.searchsorted(heads, b[:, 2], side='left'))
    # empty shares: consecutive, covering the list
    n_empty = len(ix['empty_ray'])
    assert b[0, 0] == 0 and b[-1, 1] == n_empty and (b[1:, 0] == b[:-1, 1]).all()
    assert len(ix['row_ray']) + n_empty == c.n_rays
    ids = np.arange(c.n_rays) if c.ray_ids is None else c.ray_ids
    assert np.array_equal(np.sort(np.concatenate((ix['row_ray'], ix['empty_ray']))), np.sort(ids))
    lo, hi = cc.CASES[name][3]
    assert lo <= t['stride'] <= hi, t['stride']
    # transpose twice
    tc = cc.transposed_case(c)
    assert tc.row_ptr[-1] == total and np.array_equal(np.bincount(c.vox, minlength=c.n_cols),
                                                       np.diff(tc.row_ptr))
    back = cc.transposed_case(tc)
    order = np.lexsort((np.arange(total), c.vox,
                        np.repeat(np.arange(c.n_rays), np.diff(c.row_ptr))))
    assert np.array_equal(back.row_ptr, c.row_ptr)
    assert np.array_equal(back.vox, c.vox[order]) and np.array_equal(back.len, c.len[order])
    # dense ranges of the transpose partition its outputs
    tx = cc.index_ref(tc.n_rays, tc.row_ptr, None, cc.SPB_DENSE)
    d = cc.dense_ranges_ref(tx['blocks'], tx['row_ray'], tc.n_rays)
    assert d[0, 0] == 0 and d[-1, 1] == tc.n_rays and (d[1:, 0] == d[:-1, 1]).all()
    # the exact reference is what float64 arithmetic gives too (every term exact)
    rng = np.random.default_rng(1)
    dens = cc.exact_density(rng, 1, c.n_cols)
    ref = cc.forward_exact(c, dens)
    rows = np.array([np.sum(dens[0, c.vox[a:e]] * c.len[a:e])
                     for a, e in zip(c.row_ptr[:-1], c.row_ptr[1:])])
    assert np.array_equal(ref[0, ids], rows)


def plan_descriptor(c, ix, t, runs=None, order=0, n_blocks=None):
    """A complete descriptor for sphrt_forward_plan from the numpy-derived tab_stride, n_fallback
    and tab_bytes, with dummy non-null pointers (the plan reads the fields only)."""
    from sph_raytracer_amd import _lib
    p = 64
    d = _lib.CSR()
    d.n_rays, d.n_segments = c.n_rays, int(c.row_ptr[-1])
    d.n_blocks = ix['n_blocks'] if n_blocks is None else n_blocks
    d.row_ptr = d.vox = d.len = d.len32 = d.row_ray = d.blocks = d.empty_ray = d.loc = d.tab = p
    d.tab_stride, d.n_fallback, d.n_cols = t['stride'], t['n_fallback'], c.n_cols
    d.tab_bytes, d.order = cc.tab_bytes_of(c.n_cols), order
    if runs is None:
        runs = cc.runs_fit(cc.expected_runs(ix['blocks'], ix['row_ray'], ix['empty_ray'],
                                            c.n_rays))
    d.runs = p if runs else None
    return d


def plan_of(d, elem, density=64, n_chan=1, chan_stride=None, div=0):
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    p = _lib.ForwardPlan()
    cs = d.n_cols if chan_stride is None else chan_stride
    assert lib.sphrt_forward_plan(ctypes.byref(d), elem, density, n_chan, cs, div,
                                  ctypes.byref(p)) == 0, lib.sphrt_last_error()
    return {k: getattr(p, k) for k in PLAN_FIELDS}


def designed_plan(name, elem):
    """The plan sphrt_forward_plan gives for a case's numpy-derived descriptor."""
    c, ix, t = _restated(name)
    return plan_of(plan_descriptor(c, ix, t), elem)


def test_every_case_plans_the_kernel_it_was_designed_for(monkeypatch):
    """sphrt_forward_plan on every case x {float32, float64}, then the call variants (a density
    4 bytes off granule alignment, three channels with a stride that is no multiple of 4, time
    slices, dense output ranges, whole float64 tables), and the union: every mode, table width,
    early-DMA setting and round count, half tables, run records, dense ranges, the fallback
    launch, and all three reasons for a gather."""
    monkeypatch.delenv('SPHRT_FWD_HALF', raising=False)
    plans = {}
    for name in NAMES:
        for elem in (4, 8):
            plans[name, elem] = got = designed_plan(name, elem)
            assert got == cc.CASES[name][2][elem], (name, elem)
    # call variants on short_rows (stride 256, whole granules)
    c, ix, t = _restated('short_rows')
    d = plan_descriptor(c, ix, t)
    base = cc.CASES['short_rows'][2]
    for elem in (4, 8):
        plans['misaligned', elem] = plan_of(d, elem, density=64 + 4)
        assert plans['misaligned', elem] == cc.GATHER
        plans['chan_stride', elem] = plan_of(d, elem, n_chan=3, chan_stride=c.n_cols + 2)
        assert plans['chan_stride', elem] == cc.GATHER
        assert plan_of(d, elem, n_chan=3, chan_stride=c.n_cols + 4) == base[elem]
        plans['slices', elem] = plan_of(d, elem, div=97)
        assert plans['slices', elem] == dict(cc.GATHER, mode=2)
    # dense output ranges: the transposes the GPU suite runs
    for name in ('short_rows', 'sparse_cols'):
        tc = cc.transposed_case(cc.make(name))
        tx = cc.index_ref(tc.n_rays, tc.row_ptr, None, cc.SPB_DENSE)
        tt = cc.tables_ref(tx['blocks'], tc.vox, tx['heads'])
        assert tx['n_blocks'] == int(tc.row_ptr[-1]) // cc.SPB_DENSE + 1
        dd = plan_descriptor(tc, tx, tt, runs=False, order=4)
        for elem in (4, 8):
            plans['dense ' + name, elem] = got = plan_of(dd, elem)
            assert got['dense'] == 1 and got['mode'] == 0 and got['runs'] == 0, (name, got)
        rng = cc.dense_ranges_ref(tx['blocks'], tx['row_ray'], tc.n_rays)
        width = rng[:, 1] - rng[:, 0]
        if name == 'sparse_cols':      # ranges zeroed in global memory, unaligned ends
            assert (width > cc.OUT_STAGE).any() and (rng[1:, 0] % 4 != 0).any()
        else:                          # ranges staged in LDS
            assert (width <= cc.OUT_STAGE).all() and (width > 0).sum() >= 2
    # whole float64 tables where half tables are planned by default
    monkeypatch.setenv('SPHRT_FWD_HALF', '0')
    for name in ('tab_half_one_pass', 'tab_half_two_pass'):
        assert designed_plan(name, 8) == dict(cc.CASES[name][2][8], half=0)
    monkeypatch.delenv('SPHRT_FWD_HALF')

    def seen(field, **where):
        return {p[field] for p in plans.values() if all(p[k] == v for k, v in where.items())}

    assert seen('mode') == {0, 1, 2}
    assert seen('tab_bytes', mode=0) == {2, 4}
    assert seen('edma', mode=0) == {0, 1}
    assert seen('early_rounds', mode=0, edma=1, half=0) == {1, 2, 3}
    assert 1 in seen('half') and 1 in seen('runs') and 1 in seen('dense') and 1 in seen('fallback')
    # the three reasons for a gather
    assert plans['tab_2046', 8] == cc.GATHER and plans['tab_2046', 4]['mode'] == 0
    assert _restated('tab_2046')[2]['stride'] == 2048
    assert plans['misaligned', 4]['mode'] == 1 and plans['chan_stride', 4]['mode'] == 1


def test_case_paths():
    """The row structures the cases exist for are really there (so a later edit of a generator
    cannot quietly lose one)."""
    from sph_raytracer_amd import _lib

    def blocks(name):
        return _restated(name)[1]['blocks']

    assert (cc.BLOCK_FIELDS, cc.RUN_FIELDS, cc.MAX_RUNS, cc.HEAD) == (
        _lib.BLOCK_FIELDS, _lib.RUN_FIELDS, _lib.MAX_RUNS, _lib.ROW_HEAD)

    c = cc.make('short_rows')
    cnt = np.diff(c.row_ptr)
    assert cnt[0] == 0 and cnt[-1] == 0 and set(cnt) == {0, 1, 2, 3}
    assert len(blocks('short_rows')) >= 3
    heads = np.zeros(int(c.row_ptr[-1]) + 8, dtype=int)
    heads[c.row_ptr[:-1][cnt > 0]] = 1
    per_chunk = heads[:len(heads) // 8 * 8].reshape(-1, 8).sum(1)
    assert (per_chunk >= 3).mean() > 0.9 and (per_chunk == 8).any()   # the second walk
    empty = cnt == 0
    runs = np.diff(np.flatnonzero(np.diff(np.concatenate(([0], empty, [0])))))[::2]
    assert (runs == 1).any() and (runs > 8).any()
    for last, s1 in ((257, cc.K_PASS), (258, cc.K_PASS + 1)):
        c = cc.make(f'chunk_edges_{last}')
        assert (cc.SPB - 1) in c.row_ptr and blocks(f'chunk_edges_{last}')[0, 3] == s1
        assert {7, 8, 9, 15, 16, 17} <= set(np.diff(c.row_ptr))
    c = cc.make('block_edges')
    assert cc.SPB in c.row_ptr and 2 * cc.SPB - 1 in c.row_ptr
    b = blocks('block_edges')
    assert b[1, 2] == cc.SPB and b[2, 2] > 2 * cc.SPB
    b, t = blocks('long_row_5000'), _restated('long_row_5000')[2]
    assert np.diff(cc.make('long_row_5000').row_ptr).max() == 5000
    assert t['n_tab'][0] == -1 and (b[1:, 2] == b[1:, 3]).any() and (t['n_tab'][2:] > 0).all()
    assert blocks('long_row_4096')[0, 3] == 4096 and _restated('long_row_4096')[2]['n_tab'][0] > 0
    assert blocks('long_row_4097')[0, 3] == 4097 and _restated('long_row_4097')[2]['n_tab'][0] == -1
    for name, ray in (('one_ray_first', 0), ('one_ray_last', 4999)):
        assert np.flatnonzero(np.diff(cc.make(name).row_ptr)).tolist() == [ray]
    assert len(blocks('one_ray_first')) == 3
    t = _restated('tab_half_one_pass')[2]['n_tab']
    assert np.sort(t)[-2] <= cc.HALF_TAB < t.max()
    b, t = blocks('tab_half_two_pass'), _restated('tab_half_two_pass')[2]['n_tab']
    assert t[0] > cc.HALF_TAB and b[0, 3] - b[0, 2] > cc.K_PASS
    assert _restated('tab_2046')[2]['n_tab'].max() == cc.MAX_GRAN
    t = _restated('tab_2047')[2]
    b = blocks('tab_2047')
    assert t['n_fallback'] == 1 and (b[:, 3] - b[:, 2]).max() <= cc.LOCAL_MAX
    for k in range(4):
        c = cc.make(f'cols_mod4_{k}')
        assert c.n_cols % 4 == k and c.vox.max() == c.n_cols - 1
    assert cc.tab_bytes_of(cc.make('cols_2p18').n_cols) == 2
    c = cc.make('cols_2p18_plus_4')
    assert cc.tab_bytes_of(c.n_cols) == 4 and c.vox.max() >> 2 == 65536
    for name, fit in (('ray_perm_random', False), ('ray_perm_pieces', True)):
        c, ix, _ = _restated(name)
        r = cc.expected_runs(ix['blocks'], ix['row_ray'], ix['empty_ray'], c.n_rays)
        assert cc.runs_fit(r) == fit
        if fit:
            assert max(len(rr) for rr, _ in r) in (2, 3) and max(len(er) for _, er in r) <= 2
    c = cc.make('sparse_cols')
    assert c.n_cols == 20000 and len(np.unique(c.vox)) == 300
