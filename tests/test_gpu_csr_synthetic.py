"""The CSR apply kernels (csrc/apply.hip, transpose.hip, the count scan) on the synthetic CSRs of
csr_cases.py, against exact references.

Every other GPU test of this code takes its CSR from a traced geometry, whose rows are benign;
these cases put rows on every boundary forward_kernel treats separately (chunk, pass and block
edges, rowless blocks, one-segment rows, table sizes in every class of the forward plan).

Tolerances: the *exact* value set (integer densities, lengths in eighths) must be reproduced bit
for bit by every kernel variant, float32 included; the *random* set must stay within
gamma_n * sum|d * l| of a wider-precision row sum (csr_cases.forward_random_ref).  Descriptors
are built with the project's own calls and allocations (raytracer._seg_alloc, _local_tables,
_dense_ranges), outputs sit between NaN guards."""
import ctypes
import types

import numpy as np
import pytest
import torch as tr

import csr_cases as cc
from gpu_helpers import _check_granule_tables
from test_csr_cases_cpu import PLAN_FIELDS

pytestmark = pytest.mark.gpu
NAMES = list(cc.CASES)
GUARD = 64
DT = {4: tr.float32, 8: tr.float64}


# ---- build helper ------------------------------------------------------------------------------
class Built:
    """A case on the device: the descriptor and every tensor it points to."""

    def __init__(self, case, gpu, dense=False):
        from sph_raytracer_amd import _lib, raytracer as rt
        lib = _lib.load()
        stream = _lib.stream_of(gpu)
        self.case, self.gpu, self.dense = case, gpu, dense
        n, total = case.n_rays, int(case.row_ptr[-1])
        self.n, self.total = n, total
        nblocks = (lib.sphrt_csr_blocks_dense if dense else lib.sphrt_csr_blocks)(total)
        self.nblocks = nblocks
        self.row_ptr = tr.from_numpy(case.row_ptr.copy()).to(gpu)
        # per-segment arrays: raytracer's allocation; the entries past the total (never used,
        # sphrt.h) hold column 0 and NaN lengths
        self.vox = tr.zeros(rt._seg_alloc(total), dtype=tr.int32, device=gpu)
        self.vox[:total] = tr.from_numpy(case.vox.copy()).to(gpu)
        self.len = tr.full((rt._seg_alloc(total),), float('nan'), dtype=tr.float64, device=gpu)
        self.len[:total] = tr.from_numpy(case.len.copy()).to(gpu)
        self.len32 = tr.full(self.vox.shape, float('nan'), dtype=tr.float32, device=gpu)
        self.row_ray = tr.full((max(n, 1),), -1, dtype=tr.int32, device=gpu)
        self.empty_ray = tr.full((n + 1,), -1, dtype=tr.int32, device=gpu)
        self.blocks = tr.empty(_lib.BLOCK_FIELDS * nblocks, dtype=tr.int64, device=gpu)
        self.ray_ids = (None if case.ray_ids is None
                        else tr.from_numpy(case.ray_ids.copy()).to(gpu))
        iws = tr.empty(lib.sphrt_csr_index_workspace_bytes(n), dtype=tr.uint8, device=gpu)
        index = lib.sphrt_csr_index_dense if dense else lib.sphrt_csr_index
        _lib.check(index(_lib.ptr(self.row_ptr), n, _lib.ptr(self.vox), _lib.ptr(self.row_ray),
                         _lib.ptr(self.empty_ray), _lib.ptr(self.blocks), nblocks,
                         _lib.ptr(self.ray_ids), _lib.ptr(iws), stream), 'sphrt_csr_index')
        tr.cuda.synchronize(gpu)
        del iws
        self.blocks_indexed = self.blocks.cpu().numpy().reshape(-1, _lib.BLOCK_FIELDS).copy()
        c = _lib.CSR()
        c.n_rays, c.n_segments, c.n_blocks, c.n_cols = n, total, nblocks, case.n_cols
        c.row_ptr, c.vox, c.len, c.len32 = (self.row_ptr.data_ptr(), self.vox.data_ptr(),
                                            self.len.data_ptr(), self.len32.data_ptr())
        c.row_ray, c.blocks, c.empty_ray = (self.row_ray.data_ptr(), self.blocks.data_ptr(),
                                            self.empty_ray.data_ptr())
        self.loc, self.tab, self.runs = rt._local_tables(lib, c, self.blocks, nblocks, total, gpu,
                                                         stream)
        if dense:
            rt._dense_ranges(c, self.blocks, self.row_ray, n)
            self.runs = None
        self.desc = c

    def set_lengths(self, lens):
        """Other lengths on the same structure (len, and len32 = (float)len as the table build
        makes it)."""
        from sph_raytracer_amd import _lib
        lib = _lib.load()
        self.len[:self.total] = tr.from_numpy(np.array(lens)).to(self.gpu)
        _lib.check(lib.sphrt_f64_to_f32(_lib.ptr(self.len), _lib.ptr(self.len32), self.total,
                                        _lib.stream_of(self.gpu)), 'sphrt_f64_to_f32')

    def variant(self, **fields):
        from sph_raytracer_amd import _lib
        d = _lib.CSR.from_buffer_copy(self.desc)
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    def plan(self, elem, density, n_chan, cs, div=0, desc=None):
        from sph_raytracer_amd import _lib
        p = _lib.ForwardPlan()
        _lib.check(_lib.load().sphrt_forward_plan(ctypes.byref(desc or self.desc), elem,
                                                  _lib.ptr(density), n_chan, cs, div,
                                                  ctypes.byref(p)), 'sphrt_forward_plan')
        return {k: getattr(p, k) for k in PLAN_FIELDS}

    def forward(self, density, div=0, desc=None, n_out=None):
        """sphrt_forward_f32/_f64 of a (n_chan, cs) device density into a NaN-filled buffer with
        GUARD elements on each side and channels n_out + 7 apart; checks the guards and the
        inter-channel padding and returns the (n_chan, n_out) outputs on the host."""
        from sph_raytracer_amd import _lib, raytracer as rt
        lib = _lib.load()
        n_out = self.n if n_out is None else n_out
        n_chan, cs = (1, density.shape[1]) if div > 0 else density.shape
        ocs = n_out + 7 if n_chan > 1 else n_out
        buf = tr.full((2 * GUARD + n_chan * ocs,), float('nan'), dtype=density.dtype,
                      device=self.gpu)
        out = buf[GUARD:]
        assert out.data_ptr() % 16 == 0
        fn = lib.sphrt_forward_f32 if density.dtype == tr.float32 else lib.sphrt_forward_f64
        rt._call_forward(fn, desc or self.desc, density, n_chan, cs, div, out, ocs, self.gpu)
        host = buf.cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[-GUARD:]).all(), 'guards written'
        body = host[GUARD:-GUARD].reshape(n_chan, ocs)
        assert np.isnan(body[:, n_out:]).all(), 'inter-channel padding written'
        assert np.isfinite(body[:, :n_out]).all(), 'an output was not written, or is not finite'
        return body[:, :n_out].copy()


_BUILT = {}


@pytest.fixture
def built(gpu, monkeypatch):
    """name -> the case on the device (built once per module run, run records wherever they
    fit: SPHRT_RUNS=on)."""
    monkeypatch.setenv('SPHRT_RUNS', 'on')
    monkeypatch.delenv('SPHRT_TABLES', raising=False)
    monkeypatch.delenv('SPHRT_FWD_HALF', raising=False)

    def get(name, dense=False, transposed=False):
        key = (name, dense, transposed)
        if key not in _BUILT:
            case = cc.make(name)
            _BUILT[key] = Built(cc.transposed_case(case) if transposed else case, gpu, dense)
        return _BUILT[key]

    return get


def _density(gpu, host, elem, cs=None, offset=0):
    """(n_chan, n) host values -> a device (n_chan, cs) view starting `offset` elements into its
    allocation (columns past n: NaN)."""
    n_chan, n = host.shape
    cs = n if cs is None else cs
    full = np.full((n_chan, cs), np.nan)
    full[:, :n] = host
    flat = tr.full((offset + n_chan * cs,), float('nan'), dtype=DT[elem], device=gpu)
    flat[offset:] = tr.from_numpy(full.reshape(-1)).to(gpu).to(DT[elem])
    return flat[offset:].view(n_chan, cs)


# ---- index, tables, run records, time columns, transpose ----------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_index_and_tables_equal_their_restatements(name, built, gpu):
    from sph_raytracer_amd import _lib
    from test_csr_cases_cpu import designed_plan
    b = built(name)
    c = b.case
    ix = cc.index_ref(c.n_rays, c.row_ptr, c.ray_ids)
    assert b.nblocks == ix['n_blocks']
    assert np.array_equal(b.blocks_indexed, ix['blocks'])
    vox = b.vox.cpu().numpy().view(np.uint32)
    assert np.array_equal(vox[:b.total], cc.with_heads(c.vox, ix['heads']))
    assert (vox[b.total:] == 0).all()
    n_rows = len(ix['row_ray'])
    assert np.array_equal(b.row_ray.cpu().numpy()[:n_rows], ix['row_ray'])
    assert np.array_equal(b.empty_ray.cpu().numpy()[:c.n_rays - n_rows], ix['empty_ray'])
    assert (b.row_ray.cpu().numpy()[n_rows:] == -1).all()
    assert (b.empty_ray.cpu().numpy()[c.n_rays - n_rows:] == -1).all()
    # tables
    t = cc.tables_ref(ix['blocks'], c.vox, ix['heads'])
    blocks = b.blocks.cpu().numpy().reshape(-1, _lib.BLOCK_FIELDS)
    assert np.array_equal(blocks[:, :5], ix['blocks'][:, :5])
    assert np.array_equal(blocks[:, 5], t['n_tab'])
    d = b.desc
    assert (d.n_fallback, d.tab_stride, d.tab_bytes) == (t['n_fallback'], t['stride'],
                                                         cc.tab_bytes_of(c.n_cols))
    assert b.tab.numel() == b.nblocks * d.tab_stride + 3 * 256
    tab = b.tab.cpu().numpy()
    tab = tab.view(np.uint16).astype(np.int64) if d.tab_bytes == 2 else tab.astype(np.int64)
    for k, g in enumerate(t['tabs']):
        if g is not None:
            assert np.array_equal(tab[k * d.tab_stride:k * d.tab_stride + len(g)], g), k
    loc = b.loc.cpu().numpy().view(np.uint16)[:b.total]
    assert np.array_equal(loc[t['in_table']], t['loc'][t['in_table']])
    assert np.array_equal(b.len32.cpu().numpy()[:b.total], c.len.astype(np.float32))
    # run records
    want = cc.expected_runs(ix['blocks'], ix['row_ray'], ix['empty_ray'], c.n_rays)
    assert bool(d.runs) == cc.runs_fit(want) == bool(cc.CASES[name][2][4]['runs'])
    if d.runs:
        rec = b.runs.cpu().numpy().reshape(-1, _lib.RUN_FIELDS)
        for k, (rr, er) in enumerate(want):
            assert rec[k, 0] == len(rr) and rec[k, 1] == len(er)
            for i, (off, ray, _) in enumerate(rr):
                assert (rec[k, 2 + 2 * i], rec[k, 3 + 2 * i]) == (off, ray)
            for i, (_, ray, cnt) in enumerate(er):
                assert (rec[k, 16 + 2 * i], rec[k, 17 + 2 * i]) == (ray, cnt)
    # the plan asserted on the CPU
    for elem in (4, 8):
        x = tr.zeros(c.n_cols, dtype=DT[elem], device=gpu)
        got = b.plan(elem, x, 1, c.n_cols)
        assert got == cc.CASES[name][2][elem] == designed_plan(name, elem), (name, elem)


@pytest.mark.parametrize('name', NAMES)
def test_transpose_and_time_columns_equal_their_restatements(name, built, gpu):
    from sph_raytracer_amd import _lib, raytracer as rt
    lib = _lib.load()
    b = built(name)
    c = b.case
    stream = _lib.stream_of(gpu)
    col_ptr = tr.full((c.n_cols + 1,), -1, dtype=tr.int64, device=gpu)
    t_ray = tr.full((rt._seg_alloc(b.total),), -1, dtype=tr.int32, device=gpu)
    t_len = tr.full((rt._seg_alloc(b.total),), float('nan'), dtype=tr.float64, device=gpu)
    ws = tr.empty(lib.sphrt_transpose_workspace_bytes(b.total, c.n_cols), dtype=tr.uint8,
                  device=gpu)
    _lib.check(lib.sphrt_csr_transpose(b.desc, c.n_cols, _lib.ptr(col_ptr), _lib.ptr(t_ray),
                                       _lib.ptr(t_len), _lib.ptr(ws), ws.numel(), stream),
               'sphrt_csr_transpose')
    want_ptr, want_ray, want_len = cc.transpose_ref(c)
    assert np.array_equal(col_ptr.cpu().numpy(), want_ptr)
    assert np.array_equal(t_ray.cpu().numpy()[:b.total], want_ray)
    assert np.array_equal(t_len.cpu().numpy()[:b.total], want_len)
    assert (t_ray.cpu().numpy()[b.total:] == -1).all()
    div, vol = 97, c.n_cols
    if -(-c.n_rays // div) * vol < 2 ** 31:
        out = tr.full((rt._seg_alloc(b.total),), -1, dtype=tr.int32, device=gpu)
        _lib.check(lib.sphrt_csr_time_columns(b.desc, div, vol, _lib.ptr(out), stream),
                   'sphrt_csr_time_columns')
        vox_h = b.vox.cpu().numpy().view(np.uint32)[:b.total]
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:b.total], cc.time_columns_ref(c.row_ptr, vox_h, div, vol))
        assert (got[b.total:] == 0xffffffff).all()


class _SyntheticOp:
    """What _check_granule_tables needs of an Operator, over a synthetic CSR and its transpose
    (its columns are the case's rows, its outputs the case's columns)."""

    def __init__(self, b, bt):
        self.b, self.bt = b, bt
        self._csr = dict(blocks=b.blocks, vox=b.vox, loc=b.loc, tab=b.tab, total=b.total,
                         desc=b.desc)

    def _transposed(self):
        return dict(desc=self.bt.desc)

    def __call__(self, x):
        return tr.from_numpy(self.b.forward(x.reshape(-1, x.shape[-1])))

    def T(self, y):
        return tr.from_numpy(self.bt.forward(y.reshape(1, -1)))


@pytest.mark.parametrize('name', [n for n in NAMES if not cc.CASES[n][2][4]['fallback']])
def test_granule_tables_pass_the_traced_checks(name, built, gpu):
    """_check_granule_tables (the checks the traced CSRs get) on every case whose blocks all keep
    a table, and on its transpose."""
    b, bt = built(name), built(name, transposed=True)
    assert bt.desc.n_fallback == 0
    grid = types.SimpleNamespace(shape=(b.case.n_cols,))
    geom = types.SimpleNamespace(shape=(b.case.n_rays,))
    _check_granule_tables(grid, geom, _SyntheticOp(b, bt), gpu, cc.tab_bytes_of(b.case.n_cols))


# ---- forward -------------------------------------------------------------------------------------
def _variants(b, elem, x, n_chan, cs, monkeypatch):
    """(label, descriptor, environment) of every variant that must give the same bits."""
    plan = b.plan(elem, x, n_chan, cs)
    out = [('again', None, None), ('gather', b.variant(loc=None, tab=None), None)]
    for bits in (1, 2, 3):
        out.append((f'order {bits}', b.variant(order=b.desc.order | bits), None))
    if plan['half']:
        out.append(('whole tables', None, '0'))
    if plan['runs']:
        out.append(('row lists', b.variant(runs=None), None))
    return plan, out


def _forward_all_variants(b, elem, x, monkeypatch, expect_plan=None):
    n_chan, cs = x.shape
    plan, variants = _variants(b, elem, x, n_chan, cs, monkeypatch)
    if expect_plan is not None:
        assert plan == expect_plan
    first = b.forward(x)
    for label, desc, half in variants:
        if half is not None:
            monkeypatch.setenv('SPHRT_FWD_HALF', half)
            assert b.plan(elem, x, n_chan, cs)['half'] == 0
        got = b.forward(x, desc=desc)
        monkeypatch.delenv('SPHRT_FWD_HALF', raising=False)
        assert np.array_equal(got, first), f'{label} differs from the planned kernel'
    return first


@pytest.mark.parametrize('elem', [4, 8])
@pytest.mark.parametrize('name', NAMES)
def test_forward_exact(name, elem, built, gpu, monkeypatch):
    """Exact values: every variant reproduces the integer reference bit for bit, with one
    channel (a density of exactly n_cols elements) and three (whole-granule stride; then a
    stride that is no multiple of 4 and a density 4 bytes off alignment: planned gathers).
    Columns no segment reads are NaN."""
    b = built(name)
    c = b.case
    b.set_lengths(c.len)
    rng = np.random.default_rng(cc.seed_of(name) + elem)
    used = np.unique(c.vox)
    designed = cc.CASES[name][2][elem]
    for n_chan in (1, 3):
        dens = cc.exact_density(rng, n_chan, c.n_cols, used)
        ref = cc.forward_exact(c, dens)
        cs = c.n_cols if n_chan == 1 else (c.n_cols + 3) // 4 * 4 + 4
        x = _density(gpu, dens, elem, cs)
        got = _forward_all_variants(b, elem, x, monkeypatch, designed)
        assert np.array_equal(got.astype(np.float64), ref), f'{name}: {n_chan} channel(s)'
        if n_chan == 3:
            for kw in (dict(cs=cs + 2), dict(cs=cs, offset=1)):
                xg = _density(gpu, dens, elem, **kw)
                assert b.plan(elem, xg, 3, xg.shape[1]) == cc.GATHER
                assert np.array_equal(b.forward(xg).astype(np.float64), ref), (name, kw)


@pytest.mark.parametrize('elem', [4, 8])
@pytest.mark.parametrize('name', NAMES)
def test_forward_random_within_the_summation_bound(name, elem, built, gpu, monkeypatch):
    """Random values: within gamma_n * sum|d * l| of the wide reference, all variants bitwise
    equal to one another."""
    b = built(name)
    c = b.case
    rng = np.random.default_rng(cc.seed_of(name) + 100 + elem)
    for n_chan in (1, 3):
        dens, lens = cc.random_values(rng, n_chan, c.n_cols, b.total)
        b.set_lengths(lens)
        try:
            cs = c.n_cols if n_chan == 1 else (c.n_cols + 3) // 4 * 4 + 4
            x = _density(gpu, dens, elem, cs)
            got = _forward_all_variants(b, elem, x, monkeypatch, cc.CASES[name][2][elem])
        finally:
            b.set_lengths(c.len)
        ref, bound = cc.forward_random_ref(c, dens, lens, elem)
        err = np.abs(got.astype(np.longdouble) - ref)
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        assert (err <= bound).all(), (name, worst, float(err[worst]), float(bound[worst]))


# ---- time slices ---------------------------------------------------------------------------------
@pytest.mark.parametrize('elem', [4, 8])
@pytest.mark.parametrize('name', ['short_rows', 'chunk_edges_257', 'chunk_edges_258'])
def test_time_slices_exact(name, elem, built, gpu, monkeypatch):
    """ray_chan_div > 0 (ray i reads slice i // div) against the exact reference, and the same
    integrals as a static forward over sphrt_csr_time_columns with its own tables."""
    from sph_raytracer_amd import _lib, raytracer as rt
    lib = _lib.load()
    b = built(name)
    c = b.case
    b.set_lengths(c.len)
    div, vol = 97, c.n_cols
    n_t = -(-c.n_rays // div)
    rng = np.random.default_rng(cc.seed_of(name) + 200 + elem)
    dens = cc.exact_density(rng, n_t, vol)
    ref = cc.forward_exact(c, dens, div=div)
    x = _density(gpu, dens, elem)
    assert b.plan(elem, x, 1, vol, div)['mode'] == 2
    got = b.forward(x, div=div)
    assert np.array_equal(got.astype(np.float64), ref)
    assert np.array_equal(b.forward(x, div=div), got)
    # time-paired columns, as raytracer._paired builds them
    stream = _lib.stream_of(gpu)
    vox_p = tr.zeros(rt._seg_alloc(b.total), dtype=tr.int32, device=gpu)
    _lib.check(lib.sphrt_csr_time_columns(b.desc, div, vol, _lib.ptr(vox_p), stream),
               'sphrt_csr_time_columns')
    blocks_p = b.blocks.clone()
    p = b.variant(vox=vox_p.data_ptr(), blocks=blocks_p.data_ptr(), n_cols=n_t * vol,
                  order=b.desc.order | 2, loc=None, tab=None, tab_stride=0, n_fallback=0,
                  len32=None)
    keep = rt._local_tables(lib, p, blocks_p, b.nblocks, b.total, gpu, stream)
    p.len32 = b.len32.data_ptr()
    flat = x.reshape(1, -1)
    assert b.plan(elem, flat, 1, n_t * vol, desc=p)['mode'] == 0
    assert np.array_equal(b.forward(flat, desc=p), got)
    del keep


# ---- transposed and dense ------------------------------------------------------------------------
@pytest.mark.parametrize('elem', [4, 8])
@pytest.mark.parametrize('name', ['short_rows', 'sparse_cols'])
def test_transposed_dense_ranges_exact(name, elem, built, gpu, monkeypatch):
    """The transpose indexed with sphrt_csr_index_dense and _dense_ranges: a forward with y as the
    density equals the exact adjoint, and the same CSR through sphrt_csr_index (empty-ray list)
    gives the same bits.  short_rows: ranges staged in LDS; sparse_cols: ranges above kOutStage
    with unaligned ends, zeroed in global memory."""
    from sph_raytracer_amd import _lib
    c = cc.make(name)
    dense, plain = built(name, dense=True, transposed=True), built(name, transposed=True)
    for t in (dense, plain):
        t.set_lengths(t.case.len)
    blocks = dense.blocks.cpu().numpy().reshape(-1, _lib.BLOCK_FIELDS)
    tx = cc.index_ref(c.n_cols, dense.case.row_ptr, None, cc.SPB_DENSE)
    assert np.array_equal(dense.blocks_indexed, tx['blocks'])
    assert np.array_equal(blocks[:, :5], cc.dense_ranges_ref(tx['blocks'], tx['row_ray'],
                                                             c.n_cols)[:, :5])
    assert dense.desc.order & 4 and not dense.desc.runs
    rng = np.random.default_rng(cc.seed_of(name) + 300 + elem)
    y = rng.integers(-8, 9, size=(1, c.n_rays)).astype(np.float64)
    ref = cc.adjoint_exact(c, y)
    yd = _density(gpu, y, elem)
    plan = dense.plan(elem, yd, 1, c.n_rays)
    assert plan['dense'] == 1 and plan['mode'] == 0
    got = _forward_all_variants(dense, elem, yd, monkeypatch)
    assert np.array_equal(got.astype(np.float64), ref)
    assert np.array_equal(_forward_all_variants(plain, elem, yd, monkeypatch), got)


# ---- float64-atomic adjoint ----------------------------------------------------------------------
@pytest.mark.parametrize('y_f64', [0, 1])
@pytest.mark.parametrize('name', NAMES)
def test_adjoint_accumulate_exact(name, y_f64, built, gpu):
    """sphrt_adjoint_accumulate with integer-valued y (float32 and float64): the float64 atomics
    add exact terms, so the sums equal the integer reference bit for bit in any order — two
    channels, then time slices.  The accumulator sits between NaN guards."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    b = built(name)
    c = b.case
    b.set_lengths(c.len)
    rng = np.random.default_rng(cc.seed_of(name) + 400 + y_f64)
    stream = _lib.stream_of(gpu)
    div = 97
    n_t = -(-c.n_rays // div)
    for n_chan, d, n_acc in ((2, 0, 2), (1, div, n_t)):
        y = rng.integers(-8, 9, size=(n_chan, c.n_rays)).astype(np.float64)
        ycs = c.n_rays + 5
        yd = _density(gpu, y, 8 if y_f64 else 4, ycs)
        cs = c.n_cols + 3
        buf = tr.full((2 * GUARD + n_acc * cs,), float('nan'), dtype=tr.float64, device=gpu)
        acc = buf[GUARD:GUARD + n_acc * cs].view(n_acc, cs)
        acc[:, :c.n_cols] = 0
        _lib.check(lib.sphrt_adjoint_accumulate(b.desc, _lib.ptr(yd), y_f64, n_chan, ycs, d,
                                                _lib.ptr(acc), cs, stream),
                   'sphrt_adjoint_accumulate')
        host = buf.cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[-GUARD:]).all()
        body = host[GUARD:-GUARD].reshape(n_acc, cs)
        assert np.isnan(body[:, c.n_cols:]).all()
        ref = cc.adjoint_exact(c, y, n_slices=n_acc, div=d)
        assert np.array_equal(body[:, :c.n_cols], ref), (name, n_chan, d)


# ---- scan and gather -----------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 255, 256, 257, 1023, 1024, 1025, 65536, 65537])
def test_scan_counts(n, gpu):
    """sphrt_scan_counts against np.cumsum: zeros among the counts, counts up to 2^30 (sums far
    past 2^31), sizes around the 256-thread and 1024-entry block edges."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(n)
    for hi in (4, 2 ** 30):
        counts = rng.integers(0, hi, size=n).astype(np.int32)
        counts[rng.random(n) < 0.3] = 0
        counts[-1] = hi - 1
        cd = tr.from_numpy(counts).to(gpu)
        row_ptr = tr.full((n + 1,), -1, dtype=tr.int64, device=gpu)
        ws = tr.empty(lib.sphrt_scan_workspace_bytes(n), dtype=tr.uint8, device=gpu)
        _lib.check(lib.sphrt_scan_counts(_lib.ptr(cd), n, _lib.ptr(row_ptr), _lib.ptr(ws),
                                         _lib.stream_of(gpu)), 'sphrt_scan_counts')
        want = np.concatenate(([0], np.cumsum(counts.astype(np.int64))))
        assert np.array_equal(row_ptr.cpu().numpy(), want)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1024, 1027])
def test_gather(n, gpu):
    """sphrt_gather_f32 / _f64: dst[i] = src[idx[i]] exactly, nothing written past n."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(n)
    for dt, fn in ((tr.float32, lib.sphrt_gather_f32), (tr.float64, lib.sphrt_gather_f64)):
        src = tr.from_numpy(rng.normal(size=2 * n + 3)).to(gpu).to(dt)
        idx = rng.integers(0, 2 * n + 3, size=n).astype(np.int32)
        idx[0], idx[-1] = 2 * n + 2, 0
        dst = tr.full((n + GUARD,), float('nan'), dtype=dt, device=gpu)
        _lib.check(fn(_lib.ptr(src), _lib.ptr(tr.from_numpy(idx).to(gpu)), n, _lib.ptr(dst),
                      _lib.stream_of(gpu)), 'sphrt_gather')
        assert tr.equal(dst[:n].cpu(), src.cpu()[tr.from_numpy(idx).long()])
        assert dst[n:].isnan().all()
