"""Helpers shared by the GPU test modules (no tests here)."""
import numpy as np
import torch as tr


def exact_stats(grid, geom, gpu):
    """(deferred rays, depth-limit ranges rank-sorted, ranges heap-sorted by one lane) of a count
    pass: the trace workspace's counters (trace.hip launch_trace, exact_heap_range)."""
    from sph_raytracer_amd import _lib, raytracer as rt
    lib = _lib.load()
    plan = rt._Plan(grid, gpu)
    batch = rt._RayBatch(grid, geom.ray_starts, rt._geom_rays(geom, gpu), gpu)
    counts = tr.empty(max(batch.n, 1), dtype=tr.int32, device=gpu)
    tws = rt._workspace(lib, plan, batch.n, gpu)
    _lib.check(lib.sphrt_trace_count(plan.handle, batch.desc, _lib.ptr(counts), _lib.ptr(tws),
                                     tws.numel(), _lib.stream_of(gpu)), 'sphrt_trace_count')
    head = tws[:256].cpu().view(tr.int64)
    return int(head[0]), int(head[16]), int(head[17])


def _stage_col(v, shape, brick):
    """Natural voxel -> brick-staged column (apply.hip stage_col), numpy."""
    (nr, ne, na), (br, be, ba) = shape, brick
    r, e, a = v // (ne * na), (v // na) % ne, v % na
    nbe, nba = -(-ne // be), -(-na // ba)
    blk = ((r // br) * nbe + e // be) * nba + a // ba
    return blk * (br * be * ba) + ((r % br) * be + e % be) * ba + a % ba


def _check_granule_tables(grid, geom, op, gpu, tab_bytes):
    from sph_raytracer_amd import _lib
    csr = op._csr
    blocks = csr['blocks'].cpu().numpy().reshape(-1, _lib.BLOCK_FIELDS)
    vox = csr['vox'].cpu().numpy().view(np.uint32)[:csr['total']]
    loc = csr['loc'].cpu().numpy().view(np.uint16)[:csr['total']]
    tab = csr['tab'].cpu().numpy()
    assert csr['desc'].tab_bytes == tab_bytes
    tab = tab.view(np.uint16).astype(np.int64) if tab_bytes == 2 else tab.astype(np.int64)
    s0, s1, n_tab = blocks[:, 2], blocks[:, 3], blocks[:, 5]
    assert (n_tab >= 0).all() and (n_tab <= s1 - s0).all() and csr['desc'].n_fallback == 0
    owner = np.repeat(np.arange(len(blocks)), s1 - s0)
    off = (loc & 0x7fff).astype(np.int64)   # byte offset in the float LDS image (zero granule first)
    assert (off % 4 == 0).all() and (off >= 16).all()
    slot = off // 4 - 4
    assert (slot // 4 < n_tab[owner]).all()
    v = (vox & 0x7fffffff).astype(np.int64)
    d = csr['desc']
    if d.stage_shape[0] > 0:                 # brick staging: tables address the staged columns
        v = _stage_col(v, tuple(d.stage_shape), tuple(d.stage_brick))
    stride = csr['desc'].tab_stride
    assert stride >= n_tab.max() and stride % 64 == 0
    assert np.array_equal(tab[owner * stride + slot // 4], v >> 2)
    assert np.array_equal(slot % 4, v % 4)
    assert np.array_equal(loc >> 15, vox >> 31)
    for b in range(0, len(blocks), 97):
        t0 = b * stride
        assert (np.diff(tab[t0:t0 + n_tab[b]]) > 0).all()
    g = tr.Generator(device=gpu).manual_seed(3)
    for dt in (tr.float32, tr.float64):
        x = tr.rand(grid.shape, dtype=dt, device=gpu, generator=g)
        y = tr.rand(geom.shape, dtype=dt, device=gpu, generator=g)
        xc = tr.rand((2,) + tuple(grid.shape), dtype=dt, device=gpu, generator=g)
        a, at, ac = op(x), op.T(y), op(xc)
        descs = [csr['desc'], op._transposed()['desc']]
        saved = [(d.loc, d.tab) for d in descs]
        try:
            for d in descs:
                d.loc, d.tab = None, None
            assert tr.equal(op(x), a)
            assert tr.equal(op.T(y), at)
            assert tr.equal(op(xc), ac)
        finally:
            for d, (lc, tb) in zip(descs, saved):
                d.loc, d.tab = lc, tb
