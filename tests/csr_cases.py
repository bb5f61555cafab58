"""Synthetic CSRs for the apply kernels, and numpy restatements of what the library builds from
them (no tests here; pure numpy, importable without a GPU).

Traced CSRs have benign row structure (neighbouring rows of similar length, empty rays in large
groups, hardly any one-segment row, block and pass boundaries hit only by accident).  The cases
here put rows exactly where csrc/apply.hip's forward_kernel has separate code, and come with two
value sets whose reference leaves no room for a lost segment:

  exact   integer densities in [-8, 8], lengths in {1..4} / 8: every product and partial sum of
          a row is a multiple of 1/8 below 2^24 / 8, exactly representable in float32, so every
          summation order gives the integer result bit for bit;
  random  signed uniform densities, log-uniform lengths; the reference is a wider-than-float64
          row sum and the bound gamma_n * sum|d * l| (gamma_n = n u / (1 - n u)) holds for any
          summation order.

Every generator takes a seeded numpy Generator and returns
(n_rays, row_ptr int64, vox int32 without head bits, len float64, n_cols, ray_ids or None),
valid under include/sphrt.h: columns below n_cols, lengths above 0, at least one ray."""
import math
import zlib
from collections import namedtuple

import numpy as np

# constants of csrc/apply.hip
K_PER = 8                 # kPer: segments per thread per pass
K_PASS = 2048             # kPass: segments per pass
SPB = 1792                # kSegPerBlock: row starts per workgroup
SPB_DENSE = 1984          # kDenseSegPerBlock
LOCAL_MAX = 4096          # kLocalMax: segments per workgroup with a granule table
MAX_GRAN = 2046           # kMaxGran: granules per table
HALF_TAB = 768            # kHalfTab
OUT_STAGE = 2560          # kOutStage
BLOCK_FIELDS = 6
RUN_FIELDS = 32
MAX_RUNS = 7
HEAD = 0x80000000

Case = namedtuple('Case', 'n_rays row_ptr vox len n_cols ray_ids')


# ---- building blocks ---------------------------------------------------------------------------
def _row_ptr(lengths):
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64)))).astype(np.int64)


def _exact_len(rng, total):
    return rng.integers(1, 5, size=total).astype(np.float64) / 8.0


def _random_cols(rng, total, n_cols):
    """Random columns with the last column (and so the last granule) used."""
    vox = rng.integers(0, n_cols, size=total).astype(np.int32)
    vox[rng.integers(0, total)] = n_cols - 1
    return vox


def _fill_to(rng, lengths, target, choices=(1, 2, 3, 5, 7, 8, 9, 12)):
    """Append small rows to `lengths` until they sum to exactly `target`."""
    pos = int(sum(lengths))
    assert pos <= target
    while pos < target:
        n = min(int(rng.choice(choices)), target - pos)
        lengths.append(n)
        pos += n
    return lengths


def _case(rng, lengths, n_cols, vox=None, ray_ids=None):
    row_ptr = _row_ptr(lengths)
    total = int(row_ptr[-1])
    if vox is None:
        vox = _random_cols(rng, total, n_cols)
    return Case(len(lengths), row_ptr, np.asarray(vox, dtype=np.int32), _exact_len(rng, total),
                n_cols, None if ray_ids is None else np.asarray(ray_ids, dtype=np.int32))


# ---- row-structure cases -----------------------------------------------------------------------
def short_rows(rng, n_cols=1000):
    """Lengths from {1, 1, 1, 2, 3}: most 8-segment chunks hold 3 to 8 heads (the second walk of
    the closes).  Empty rays interleaved singly and in runs, ray 0 and the last ray empty; a
    little over three blocks."""
    lengths = [0]
    while sum(lengths) < 3 * SPB + 200:
        u = rng.random()
        if u < 0.15:
            lengths.append(0)
        elif u < 0.18:
            lengths.extend([0] * int(rng.integers(2, 41)))
        lengths.append(int(rng.choice([1, 1, 1, 2, 3])))
    lengths.append(0)
    return _case(rng, lengths, n_cols)


def chunk_edges(rng, last=257, n_cols=1600):
    """Lengths cycling through 7, 8, 9, 15, 16, 17 (rows ending one short of, on and one past a
    thread's chunk), and a row that starts at segment 1791, the last slot of block 0: with length
    257 block 0 ends exactly at kPass; with 258 one segment is left for a second pass."""
    cyc = (7, 8, 9, 15, 16, 17)
    lengths, i = [], 0
    while sum(lengths) + cyc[i % 6] <= SPB - 1 - 20:
        lengths.append(cyc[i % 6])
        i += 1
    _fill_to(rng, lengths, SPB - 1)
    lengths.append(last)
    while sum(lengths) < 3 * SPB + 100:
        lengths.append(cyc[i % 6])
        i += 1
    return _case(rng, lengths, n_cols)


def block_edges(rng, n_cols=2800):
    """One row ends exactly at segment 1792 and the next starts there (block 1's first row starts
    on base0: no window clamp), block 1 has a row starting at its slot 1791, and block 2's first
    row therefore starts past its base0 (the clamp lo = -1 is not taken: lo > 0)."""
    lengths = _fill_to(rng, [], SPB - 11)
    lengths.append(11)                                 # ends exactly at 1792
    lengths.append(6)                                  # starts at 1792
    _fill_to(rng, lengths, 2 * SPB - 1)
    lengths.append(40)                                 # starts at slot 1791 of block 1
    _fill_to(rng, lengths, 3 * SPB + 300)
    return _case(rng, lengths, n_cols)


def long_row(rng, first_block=None, n_cols=1000):
    """A few short rows, one long row, short rows again.  first_block None: the long row has 5000
    segments — its block exceeds kLocalMax (n_tab = -1, the fallback launch next to table blocks)
    and the blocks inside it own no row.  first_block 4096: block 0 has exactly kLocalMax segments
    (table kept, two passes); 4097: one more (fallback)."""
    lengths = _fill_to(rng, [], 100)
    lengths.append(5000 if first_block is None else first_block - 100)
    _fill_to(rng, lengths, int(sum(lengths)) + 2500)
    return _case(rng, lengths, n_cols)


def all_empty_but_one(rng, where='first', length=4000, n_cols=1000):
    """One non-empty ray among 5000 (the first or the last ray): every block's work is its share
    of the empty list."""
    lengths = [0] * 5000
    lengths[0 if where == 'first' else -1] = length
    return _case(rng, lengths, n_cols)


# ---- table-shape cases -------------------------------------------------------------------------
def _rows_for_blocks(rng, n_blocks, big=None):
    """Row lengths filling n_blocks blocks with small rows; big = {block: segments} gives that
    block exactly that many segments (its last row overhangs the next blocks' windows)."""
    big = big or {}
    lengths, pos = [], 0
    for b in range(n_blocks):
        end = (b + 1) * SPB
        if pos >= end:
            continue                                   # a rowless block inside an overhang
        s0 = pos
        while pos + 12 < end - 1:
            n = int(rng.integers(1, 13))
            lengths.append(n)
            pos += n
        n = s0 + big[b] - pos if b in big else int(rng.integers(1, 13))
        assert n >= 1
        lengths.append(n)
        pos += n
    return lengths


def table_shape(rng, grans, big=None, n_cols=16384):
    """Blocks whose distinct-granule counts are exactly grans[b] (a random granule set per block,
    dealt round-robin over the block's segments, random lanes)."""
    lengths = _rows_for_blocks(rng, len(grans), big)
    row_ptr = _row_ptr(lengths)
    total = int(row_ptr[-1])
    blocks = index_ref(len(lengths), row_ptr)['blocks']
    vox = np.zeros(total, dtype=np.int32)
    n_gran = n_cols // 4
    for b, (s0, s1) in enumerate(blocks[:, 2:4]):
        n = int(s1 - s0)
        if n == 0:
            continue
        g = min(grans[min(b, len(grans) - 1)], n)     # (a short tail block: what it has)
        gset = rng.permutation(n_gran)[:g]
        slot = rng.permutation(n) % g
        vox[s0:s1] = 4 * gset[slot] + rng.integers(0, 4, size=n)
    return Case(len(lengths), row_ptr, vox, _exact_len(rng, total), n_cols, None)


# ---- column-count and ray-id cases -------------------------------------------------------------
def col_count(rng, n_cols):
    """Random rows of 1 to 12 segments over n_cols columns, the last column used."""
    lengths = []
    while sum(lengths) < SPB + 900:
        lengths.append(int(rng.integers(0, 13)))
    return _case(rng, lengths, n_cols)


def ray_perm_random(rng, n_cols=1000):
    """ray_ids a random permutation: every block's rows scatter, run records overflow."""
    c = col_count(rng, n_cols)
    return c._replace(ray_ids=rng.permutation(c.n_rays).astype(np.int32))


def ray_perm_pieces(rng, n_cols=1000):
    """ray_ids a permutation of three consecutive pieces, no empty ray except one group at the
    end: every block maps to at most three runs and its empty share to at most two ranges."""
    lengths = []
    while sum(lengths) < 2 * SPB + 500:
        lengths.append(int(rng.integers(5, 13)))
    lengths.extend([0] * 40)
    n = len(lengths)
    a, b = n // 3, 2 * n // 3 + 5
    ids = np.concatenate((np.arange(b, n), np.arange(0, a), np.arange(a, b)))
    return _case(rng, lengths, n_cols, ray_ids=ids)


def sparse_cols(rng, n_cols=20000, used=300):
    """300 used columns out of 20000: the transpose has output ranges above kOutStage with
    unaligned ends."""
    lengths = []
    while sum(lengths) < 3 * SPB_DENSE + 300:
        lengths.append(int(rng.integers(0, 9)))
    total = int(sum(lengths))
    cols = np.sort(rng.choice(np.arange(3, n_cols - 5), used, replace=False))
    vox = cols[rng.integers(0, used, size=total)]
    return _case(rng, lengths, n_cols, vox=vox)


def _table(tab_bytes, edma, rounds, half=0, fallback=0, runs=1):
    return dict(mode=0, tab_bytes=tab_bytes, edma=edma, runs=runs, half=half, dense=0,
                early_rounds=rounds, fallback=fallback)


GATHER = dict(mode=1, tab_bytes=4, edma=0, runs=0, half=0, dense=0, early_rounds=3, fallback=0)

# name: (generator, keyword arguments, {element bytes: the forward plan the case is designed for,
#        with run records wherever every block's rows and empty share fit them},
#        (lowest, highest) tab_stride the design allows)
CASES = {
    'short_rows': (short_rows, {},
                   {4: _table(2, 1, 1, runs=0), 8: _table(2, 1, 1, runs=0)}, (256, 256)),
    'chunk_edges_257': (chunk_edges, dict(last=257),
                        {4: _table(2, 1, 2), 8: _table(2, 1, 2)}, (320, 448)),
    'chunk_edges_258': (chunk_edges, dict(last=258),
                        {4: _table(2, 1, 2), 8: _table(2, 1, 2)}, (320, 448)),
    'block_edges': (block_edges, {}, {4: _table(2, 1, 3), 8: _table(2, 1, 3)}, (576, 704)),
    'long_row_5000': (long_row, {}, {4: _table(2, 1, 1, fallback=1),
                                     8: _table(2, 1, 1, fallback=1)}, (256, 256)),
    'long_row_4096': (long_row, dict(first_block=4096),
                      {4: _table(2, 1, 1), 8: _table(2, 1, 1)}, (256, 256)),
    'long_row_4097': (long_row, dict(first_block=4097),
                      {4: _table(2, 1, 1, fallback=1), 8: _table(2, 1, 1, fallback=1)}, (256, 256)),
    'one_ray_first': (all_empty_but_one, dict(where='first', length=4000),
                      {4: _table(2, 1, 1), 8: _table(2, 1, 1)}, (256, 256)),
    'one_ray_last': (all_empty_but_one, dict(where='last', length=5),
                     {4: _table(2, 1, 1), 8: _table(2, 1, 1)}, (64, 64)),
    'tab_256': (table_shape, dict(grans=[200, 130, 200]),
                {4: _table(2, 1, 1), 8: _table(2, 1, 1)}, (256, 256)),
    'tab_512': (table_shape, dict(grans=[300, 400, 257]),
                {4: _table(2, 1, 2), 8: _table(2, 1, 2)}, (448, 448)),
    'tab_768': (table_shape, dict(grans=[700, 768, 10]),
                {4: _table(2, 1, 3), 8: _table(2, 1, 3)}, (768, 768)),
    'tab_1216': (table_shape, dict(grans=[1000, 769, 1216]),
                 {4: _table(2, 1, 3), 8: _table(2, 1, 3)}, (1216, 1216)),
    # (the stride follows the largest n_tab, so a half-table plan always has a block above
    # kHalfTab: here that block is a one-pass block and every other block stays at or below it)
    'tab_half_one_pass': (table_shape, dict(grans=[768, 1300, 500]),
                          {4: _table(2, 1, 3), 8: _table(2, 1, 3, half=1)}, (1344, 1344)),
    'tab_half_two_pass': (table_shape, dict(grans=[1500, 600, 769], big={0: 3000}),
                          {4: _table(2, 1, 3), 8: _table(2, 1, 3, half=1)}, (1536, 1536)),
    'tab_1984': (table_shape, dict(grans=[1700, 1600, 900]),
                 {4: _table(2, 1, 3), 8: _table(2, 1, 3)}, (1728, 1728)),
    'tab_2046': (table_shape, dict(grans=[2046, 300, 300], big={0: 2300}),
                 {4: _table(2, 1, 3), 8: GATHER}, (2048, 2048)),
    'tab_2047': (table_shape, dict(grans=[300, 2047, 300, 300], big={1: 2300}),
                 {4: _table(2, 1, 2, fallback=1), 8: _table(2, 1, 2, fallback=1)}, (320, 320)),
    'cols_mod4_0': (col_count, dict(n_cols=1000),
                    {4: _table(2, 1, 1, runs=0), 8: _table(2, 1, 1, runs=0)}, (256, 256)),
    'cols_mod4_1': (col_count, dict(n_cols=1001),
                    {4: _table(2, 0, 3, runs=0), 8: _table(2, 0, 3, runs=0)}, (256, 256)),
    'cols_mod4_2': (col_count, dict(n_cols=1002),
                    {4: _table(2, 0, 3, runs=0), 8: _table(2, 0, 3, runs=0)}, (256, 256)),
    'cols_mod4_3': (col_count, dict(n_cols=1003),
                    {4: _table(2, 0, 3, runs=0), 8: _table(2, 0, 3, runs=0)}, (256, 256)),
    'cols_2p18': (col_count, dict(n_cols=262144),
                  {4: _table(2, 1, 3, runs=0), 8: _table(2, 1, 3, runs=0)}, (1600, 1792)),
    'cols_2p18_plus_4': (col_count, dict(n_cols=262148),
                         {4: _table(4, 1, 3, runs=0), 8: _table(4, 1, 3, runs=0)}, (1600, 1792)),
    'ray_perm_random': (ray_perm_random, {},
                        {4: _table(2, 1, 1, runs=0), 8: _table(2, 1, 1, runs=0)}, (256, 256)),
    'ray_perm_pieces': (ray_perm_pieces, {},
                        {4: _table(2, 1, 1), 8: _table(2, 1, 1)}, (256, 256)),
    'sparse_cols': (sparse_cols, {},
                    {4: _table(2, 1, 2, runs=0), 8: _table(2, 1, 2, runs=0)}, (320, 320)),
}

_MADE = {}


def seed_of(name):
    return zlib.crc32(name.encode())


def make(name):
    """The case of that name (deterministic: seeded by the name; made once, never modified)."""
    if name not in _MADE:
        gen, kw = CASES[name][:2]
        c = gen(np.random.default_rng(seed_of(name)), **kw)
        check_valid(c)
        for a in (c.row_ptr, c.vox, c.len) + (() if c.ray_ids is None else (c.ray_ids,)):
            a.setflags(write=False)
        _MADE[name] = c
    return _MADE[name]


def check_valid(c):
    """The promises of include/sphrt.h, the sizes the suite keeps to, and the exactness bound of
    the exact value set."""
    total = int(c.row_ptr[-1])
    assert c.n_rays >= 1 and len(c.row_ptr) == c.n_rays + 1 and c.row_ptr[0] == 0
    assert (np.diff(c.row_ptr) >= 0).all() and len(c.vox) == total == len(c.len)
    assert total >= 1 and (c.vox >= 0).all() and (c.vox < c.n_cols).all() and (c.len > 0).all()
    assert total <= 21000 and c.n_cols <= 2 ** 18 + 8
    assert c.row_ptr.dtype == np.int64 and c.vox.dtype == np.int32 and c.len.dtype == np.float64
    if c.ray_ids is not None:
        assert np.array_equal(np.sort(c.ray_ids), np.arange(c.n_rays))
    # exact set: |density| <= 8, 8 * len in {1..4}: a row's partial sums are multiples of 1/8
    # bounded by 4 * n, so 32 * n < 2^24 keeps every one of them exact in float32
    assert np.array_equal(c.len * 8, np.round(c.len * 8)) and (c.len * 8 <= 4).all()
    assert 32 * int(np.diff(c.row_ptr).max()) < 2 ** 24


# ---- numpy restatements ------------------------------------------------------------------------
def index_ref(n_rays, row_ptr, ray_ids=None, spb=SPB):
    """sphrt_csr_index (spb = SPB) / sphrt_csr_index_dense (SPB_DENSE): head positions, row_ray,
    the used prefix of empty_ray and the six block fields (n_tab = -1)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    ne = np.diff(row_ptr) > 0
    ids = np.arange(n_rays, dtype=np.int32) if ray_ids is None else np.asarray(ray_ids, np.int32)
    total = int(row_ptr[-1])
    row_pre = np.concatenate(([0], np.cumsum(ne))).astype(np.int64)
    nb = total // spb + 1
    # first ray r < n with row_ptr[r] >= b * spb (n when there is none)
    lo = np.searchsorted(row_ptr[:n_rays], np.arange(nb) * spb, side='left')
    hi = np.append(lo[1:], n_rays)
    n_empty = n_rays - int(row_pre[-1])
    e_chunk = -(-n_empty // nb)
    b = np.arange(nb)
    blocks = np.stack([np.minimum(b * e_chunk, n_empty), np.minimum((b + 1) * e_chunk, n_empty),
                       row_ptr[lo], row_ptr[hi], row_pre[lo], np.full(nb, -1)], axis=1)
    return dict(heads=row_ptr[:-1][ne], row_ray=ids[ne], empty_ray=ids[~ne],
                blocks=blocks.astype(np.int64), n_blocks=nb)


def with_heads(vox, heads):
    v = np.asarray(vox).astype(np.uint32)
    v[heads] |= np.uint32(HEAD)
    return v


def tables_ref(blocks, vox, heads):
    """sphrt_csr_local_*: per block the ascending distinct granules (voxel >> 2) of its segments,
    n_tab (-1 for more than LOCAL_MAX segments or MAX_GRAN granules), and per segment of a table
    block loc = 16 * (rank + 1) + 4 * (voxel & 3) with the row-head flag in bit 15.  Returns
    dict(n_tab, tabs, loc, in_table, n_fallback, max_tab, stride)."""
    vox = np.asarray(vox, dtype=np.int64)
    head = np.zeros(len(vox), dtype=np.int64)
    head[heads] = 1
    n_tab = np.empty(len(blocks), dtype=np.int64)
    tabs, loc = [], np.zeros(len(vox), dtype=np.uint16)
    in_table = np.zeros(len(vox), dtype=bool)
    for b, (s0, s1) in enumerate(blocks[:, 2:4]):
        v = vox[s0:s1]
        g = np.unique(v >> 2)
        if s1 - s0 > LOCAL_MAX or len(g) > MAX_GRAN:
            n_tab[b] = -1
            tabs.append(None)
            continue
        n_tab[b] = len(g)
        tabs.append(g)
        rank = np.searchsorted(g, v >> 2)
        loc[s0:s1] = (16 * (rank + 1) + 4 * (v & 3)) | (head[s0:s1] << 15)
        in_table[s0:s1] = True
    max_tab = int(max(n_tab.max(), 0))
    return dict(n_tab=n_tab, tabs=tabs, loc=loc, in_table=in_table,
                n_fallback=int((n_tab < 0).sum()), max_tab=max_tab,
                stride=max(64, (max_tab + 63) // 64 * 64))


def tab_bytes_of(n_cols):
    """raytracer._tables_one_pass: 16-bit table entries when every granule index fits."""
    return 2 if (n_cols + 3) // 4 <= 65536 else 4


def expected_runs(blocks, row_ray, empty, n_rays):
    """block_runs_kernel: per block, the runs (first row relative to the block, its ray, length)
    of consecutive rays of its rows and of its share of the empty list (None for more than
    MAX_RUNS)."""
    n_rows = n_rays - blocks[-1, 1]

    def runs(v):
        if len(v) == 0:
            return []
        cut = np.nonzero(np.diff(v) != 1)[0] + 1
        starts = np.concatenate(([0], cut))
        ends = np.concatenate((cut, [len(v)]))
        return [(int(a), int(v[a]), int(b - a)) for a, b in zip(starts, ends)]

    out = []
    for b in range(len(blocks)):
        k0 = blocks[b, 4]
        k1 = blocks[b + 1, 4] if b + 1 < len(blocks) else n_rows
        rr = runs(row_ray[k0:k1])
        er = runs(empty[blocks[b, 0]:blocks[b, 1]])
        out.append((rr if len(rr) <= MAX_RUNS else None,
                    er if len(er) <= MAX_RUNS else None))
    return out


def runs_fit(runs):
    return all(rr is not None and er is not None for rr, er in runs)


def dense_ranges_ref(blocks, row_ray, n_out):
    """raytracer._dense_ranges: block b's output range [lo, hi) — from its first row's output (0
    for the first block) to the first row of the next block with rows (n_out for the last)."""
    blocks = blocks.copy()
    n_rows = max(len(row_ray), 1)
    has = blocks[:, 2] < blocks[:, 3]
    k0 = np.clip(blocks[:, 4], 0, n_rows - 1)
    first = np.where(has, np.asarray(row_ray, dtype=np.int64)[k0] if len(row_ray) else n_out,
                     n_out)
    first = np.minimum.accumulate(first[::-1])[::-1]
    lo = first.copy()
    lo[0] = 0
    blocks[:, 0] = lo
    blocks[:, 1] = np.append(first[1:], n_out)
    return blocks


def time_columns_ref(row_ptr, vox_h, div, vol):
    """sphrt_csr_time_columns on head-flagged columns: (r / div) * vol + voxel, head bit kept."""
    r = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    v = np.asarray(vox_h).astype(np.uint32)
    col = (r // div) * vol + (v & np.uint32(HEAD - 1))
    return (v & np.uint32(HEAD)) | col.astype(np.uint32)


def transpose_ref(c):
    """sphrt_csr_transpose: col_ptr (n_cols + 1), and per column its segments in ray order (a
    stable sort by column): t_ray, t_len."""
    seg_ray = np.repeat(np.arange(c.n_rays, dtype=np.int32), np.diff(c.row_ptr))
    perm = np.argsort(c.vox, kind='stable')
    col_ptr = np.concatenate(([0], np.cumsum(np.bincount(c.vox, minlength=c.n_cols))))
    return col_ptr.astype(np.int64), seg_ray[perm], c.len[perm]


def transposed_case(c):
    """The transpose as a case of its own: rows are c's columns, columns its rays (trace rows)."""
    col_ptr, t_ray, t_len = transpose_ref(c)
    return Case(c.n_cols, col_ptr, t_ray.astype(np.int32), t_len, c.n_rays, None)


# ---- value sets and references -----------------------------------------------------------------
def _ids(c):
    return np.arange(c.n_rays) if c.ray_ids is None else c.ray_ids.astype(np.int64)


def _row_sums(prod, row_ptr):
    """Per-row sums of prod (rows of row_ptr), 0 for empty rows; integer or floating."""
    ne = np.diff(row_ptr) > 0
    out = np.zeros(len(row_ptr) - 1, dtype=prod.dtype)
    out[ne] = np.add.reduceat(prod, row_ptr[:-1][ne])
    return out


def exact_density(rng, n_chan, n_cols, used=None):
    """Integers in [-8, 8] as float64, (n_chan, n_cols).  With `used` (columns some segment
    reads), every other column is NaN: a value no output may depend on."""
    d = rng.integers(-8, 9, size=(n_chan, n_cols)).astype(np.float64)
    if used is not None:
        mask = np.ones(n_cols, dtype=bool)
        mask[used] = False
        d[:, mask] = np.nan
    return d


def random_values(rng, n_chan, n_cols, total):
    """Signed uniform densities (n_chan, n_cols) and log-uniform lengths in [1e-3, 10]."""
    return rng.uniform(-1, 1, size=(n_chan, n_cols)), 10.0 ** rng.uniform(-3, 1, size=total)


def forward_exact(c, density, div=0):
    """out[ch, ray] of the exact value set in integer arithmetic (eighths), as float64: every
    summation order in float32 or float64 must give these bits.  div > 0: density is
    (T, n_cols) and ray i reads slice i // div, output (1, n_rays)."""
    len8 = np.round(c.len * 8).astype(np.int64)
    ids = _ids(c)
    cnt = np.diff(c.row_ptr)
    d = np.nan_to_num(density).astype(np.int64)
    if div > 0:
        sl = np.repeat(ids // div, cnt)
        chans = [d[sl, c.vox]]
    else:
        chans = [dc[c.vox] for dc in d]
    out = np.zeros((len(chans), c.n_rays))
    for k, dv in enumerate(chans):
        s = _row_sums(dv * len8, c.row_ptr)
        assert np.abs(s).max() < 2 ** 24
        out[k, ids] = s / 8.0
    return out


def adjoint_exact(c, y, n_slices=0, div=0):
    """acc[ch, col] += y[ch, ray] * len in integer arithmetic, as float64 (y integer-valued).
    div > 0: y is (1, n_rays) and ray i adds into slice i // div of n_slices."""
    len8 = np.round(c.len * 8).astype(np.int64)
    ray = np.repeat(_ids(c), np.diff(c.row_ptr))
    yi = np.asarray(y).astype(np.int64)
    if div > 0:
        acc = np.zeros((n_slices, c.n_cols), dtype=np.int64)
        np.add.at(acc, (ray // div, c.vox), yi[0, ray] * len8)
    else:
        acc = np.zeros((len(yi), c.n_cols), dtype=np.int64)
        for k in range(len(yi)):
            np.add.at(acc[k], c.vox, yi[k, ray] * len8)
    return acc / 8.0


WIDE = np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant


def forward_random_ref(c, density, lens, elem):
    """(reference, bound) per (channel, ray) for the random value set.  float32 (elem 4): the
    kernel's inputs are the float32-rounded density and lengths.  Reference: np.longdouble row
    sums where longdouble is wider than float64, else math.fsum over the float64 products.
    Bound: gamma_n * sum|d * l|, n the row length, u = 2^-24 / 2^-53 — the standard bound of a
    length-n inner product in any summation order — plus the same expression for the reference's
    own sum (u = the longdouble's; 0 for fsum's exactly rounded sum of rounded products, which
    the products' u covers)."""
    if elem == 4:
        density = density.astype(np.float32).astype(np.float64)
        lens = lens.astype(np.float32).astype(np.float64)
    u = 2.0 ** -24 if elem == 4 else 2.0 ** -53
    n = np.diff(c.row_ptr).astype(np.float64)
    ids = _ids(c)
    ref = np.zeros((len(density), c.n_rays), dtype=np.longdouble)
    bound = np.zeros((len(density), c.n_rays))
    u_ref = float(np.finfo(np.longdouble).eps) / 2 if WIDE else 2.0 ** -53
    for k, dc in enumerate(density):
        dv = dc[c.vox]
        if WIDE:
            s = _row_sums(dv.astype(np.longdouble) * lens.astype(np.longdouble), c.row_ptr)
        else:
            p = dv * lens
            s = np.array([math.fsum(p[a:b]) for a, b in zip(c.row_ptr[:-1], c.row_ptr[1:])])
        mag = _row_sums(np.abs(dv * lens), c.row_ptr)
        gam = n * u / (1 - n * u) + (n + 1) * u_ref / (1 - (n + 1) * u_ref)
        ref[k, ids] = s
        bound[k, ids] = gam * mag * (1 + 2.0 ** -50)    # (mag itself is a rounded float64 sum)
    return ref, bound
