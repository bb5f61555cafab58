"""Named irregular wide grids and rays for the wave trace's sort and fill ladder, and a numpy
restatement of that ladder (no tests here).

csrc/trace.hip trace_one picks a ray's path from the length F of its crossing list and from how
much of it is shell crossings (n_other = F - s_near - nfar): one of ten sort rungs (sort_regs<1>,
merge_sort<2,1>, sort_regs<2>, merge_sort<4,1>, <4,2>, sort_regs<4>, merge_sort<8,2>, <8,4>,
sort_regs<8>, sort_lds), inside merge_sort the merge path or the bitonic half-cleaners
(shell_run_ascending), one of seven fills (fill_regs<1|2|3|4|6|8> or the LDS chunk loop), 64-wide
chunk skipping for families of more than 64 boundaries, the half-plane wedge for more than 64
half-planes, and a tie analysis that carries state from one 64-entry chunk to the next.  Each case
below is a seeded (r_b, e_b, a_b, xs, rays) of at most 2000 rays picked for some of those;
`list_classes(name)` says, from the C oracle's solves alone, which ray takes which.
tests/test_trace_cases_cpu.py asserts on that restatement that every rung, skip, wrap, near-tie and
late-tie input is present; tests/test_gpu_trace_cases.py runs the cases on the GPU.

Grids: explicit boundary vectors with irregular gaps (test_gpu_fuzz._bounds), hollow and solid
radial ranges, full and partial elevation ranges, azimuth full, partial, partial across 0 and
[0, 2 pi].  `dup` grids carry extra boundaries 1 ulp and 4 ulps (np.nextafter) above existing ones
in one family: gaps under 1e-12 x the scale, so the sliver voxels' segments fall under
golden_cases.compare_segments' drop rule.  Two distances a few ulps apart are the input on which
composite keys collide above the candidate bits and shell_run_ascending fails.

Rays: lines from outside aimed at random points of the ball; starts in and around the ball in
random directions (those inside a voxel get a head segment, no wedge and the bound K); and, in
`tie` cases, lattice rays (tests/golden/make_golden.py lattice: starts with coordinates in {-2, -1,
-1/2, 0, 1/2, 1, 2} x the 26 directions with components in {-1, 0, 1}) whose line reaches the
ball, on grids that hold the boundaries such rays hit exactly: shells 0.5 and 1, the cone pi / 2,
half-planes 0, +-pi / 2 (pi / 2, pi, 3 pi / 2 on the [0, 2 pi] grid).
"""
import functools
import math
from collections import namedtuple

import numpy as np

Case = namedtuple('Case', 'name shape r e a dup tie n')
Case.__new__.__defaults__ = (None, False, 1600)

PI = math.pi
# shape (nr, ne, na); r / e: (lo, hi); a: 'full' (-pi, pi), '2pi' (0, 2 pi) or (lo, hi);
# dup: the family that carries near-duplicate boundaries (they add to the shape: 3 pairs 1 ulp
# apart and 3 pairs 4 ulps apart); tie: lattice rays, and boundaries at the values they hit.
CASES = [
    Case('small_30x20x12', (30, 20, 12), (0.15, 1.1), (0.15, 2.95), (0.2, 3.1)),
    Case('az_5x5x144_dup_a', (5, 5, 144), (0.0, 1.0), (0.0, PI), 'full', 'a'),
    Case('shells_124x6x6_dup_r', (124, 6, 6), (0.2, 1.3), (0.0, PI), 'full', 'r'),
    Case('az_6x40x200', (6, 40, 200), (0.0, 0.9), (0.2, 2.9), (-2.9, 2.7)),
    Case('shells_200x20x20_tie', (200, 20, 20), (0.0, 1.5), (0.0, PI), 'full', None, True, 2000),
    Case('wide_100x100x150_tie', (100, 100, 150), (0.0, 1.0), (0.0, PI), '2pi', None, True, 2000),
    Case('cones_10x150x360_dup_e', (10, 150, 360), (0.3, 1.2), (0.0, PI), 'full', 'e'),
    Case('shells_254x4x4_dup_r', (254, 4, 4), (0.0, 1.0), (0.0, PI), 'full', 'r', False, 2000),
    Case('cones_8x90x30', (8, 90, 30), (0.3, 1.4), (0.4, 2.6), (-1.6, 2.4)),
    Case('lds_300x10x10', (300, 10, 10), (0.05, 1.0), (0.0, PI), 'full', None, False, 2000),
    Case('all65_64x64x64_tie', (64, 64, 64), (0.0, 1.0), (0.0, PI), 'full', None, True),
    Case('all64_63x63x63', (63, 63, 63), (0.1, 1.2), (0.4, 2.8), (-3.0, 2.8)),
    Case('k512_150x60x86', (150, 60, 86), (0.0, 1.0), (0.0, PI), (-3.05, 2.95), None, False, 2000),
    Case('k514_150x60x88', (150, 60, 88), (0.15, 1.25), (0.25, 3.0), 'full', None, False, 2000),
]
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
SCALE = 4.0         # compare_segments' length scale, as test_gpu_fuzz.py: above every start
N_DUP = 3           # pairs of each kind (1 ulp, 4 ulps) in a `dup` family

# sort rungs in trace_one's order, the template arguments (M, M2) (M2 = 0: the full network)
RUNGS = ['regs1', 'merge2_1', 'regs2', 'merge4_1', 'merge4_2', 'regs4', 'merge8_2', 'merge8_4',
         'regs8', 'lds']
RUNG_M = dict(regs1=1, merge2_1=2, regs2=2, merge4_1=4, merge4_2=4, regs4=4, merge8_2=8,
              merge8_4=8, regs8=8, lds=0)
FILLS = [1, 2, 3, 4, 6, 8, 0]       # fill_regs<M>; 0: the LDS chunk loop
_F_EDGES = [0, 64, 128, 256, 512]   # sort: F in (edge, next edge]
_FILL_EDGES = [0, 64, 128, 192, 256, 384, 512]


def _seed(case):
    return 4000 + NAMES.index(case.name)


def _bounds(rng, n, lo, hi):
    """n + 1 ascending boundaries from lo to hi, gaps random but at least (hi - lo) / (8 n)
    (test_gpu_fuzz._bounds)."""
    w = rng.uniform(1.0, 8.0, n)
    w = w / w.sum() * (hi - lo)
    return np.concatenate([[lo], lo + np.cumsum(w)[:-1], [hi]])


def _through(b, marks):
    """b with, for every mark strictly inside it, the nearest interior boundary moved onto it."""
    b = b.copy()
    taken = set()
    for m in marks:
        if not b[0] < m < b[-1]:
            continue
        order = np.argsort(np.abs(b[1:-1] - m)) + 1
        k = next(int(k) for k in order if int(k) not in taken)
        taken.add(k)
        b[k] = m
    b.sort()
    assert (np.diff(b) > 0).all()
    return b


def _near_duplicates(rng, b):
    """b with N_DUP boundaries 1 ulp and N_DUP boundaries 4 ulps above existing interior ones."""
    picks = rng.choice(np.arange(1, len(b) - 1), 2 * N_DUP, replace=False)
    extra = []
    for i, k in enumerate(picks):
        v = b[k]
        for _ in range(1 if i < N_DUP else 4):
            v = np.nextafter(v, np.inf)
        extra.append(v)
    out = np.sort(np.concatenate([b, extra]))
    assert (np.diff(out) > 0).all() and len(out) == len(b) + 2 * N_DUP
    return out


def _lattice_rays(rng, n, r1):
    """n lattice rays whose line comes within r1 of the origin ahead of (or around) the start."""
    c = np.array([-2, -1, -0.5, 0, 0.5, 1, 2])
    xs = np.stack(np.meshgrid(c, c, c, indexing='ij'), -1).reshape(-1, 3)
    s = np.array([-1.0, 0.0, 1.0])
    d = np.stack(np.meshgrid(s, s, s, indexing='ij'), -1).reshape(-1, 3)
    d = d[np.abs(d).sum(1) > 0]
    xs, d = np.repeat(xs, len(d), 0), np.tile(d, (len(xs), 1))
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    tc = -(xs * u).sum(1)
    dd2 = (xs * xs).sum(1) - tc * tc
    ok = (dd2 <= r1 * r1) & (tc + np.sqrt(np.maximum(r1 * r1 - dd2, 0.0)) > 0)
    pick = rng.choice(np.flatnonzero(ok), n, replace=False)
    return xs[pick], d[pick]


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (r_b, e_b, a_b, xs, rays): float64 arrays, rays of unit length; treat as read-only."""
    case = BY_NAME[name]
    rng = np.random.default_rng(_seed(case))
    nr, ne, na = case.shape
    a_lo, a_hi = {'full': (-PI, PI), '2pi': (0.0, 2 * PI)}.get(case.a, case.a)
    r_b = _bounds(rng, nr, *case.r)
    e_b = _bounds(rng, ne, *case.e)
    a_b = _bounds(rng, na, a_lo, a_hi)
    if case.tie:
        r_b = _through(r_b, [0.5, 1.0])
        e_b = _through(e_b, [PI / 2])
        a_b = _through(a_b, [PI / 2, PI, 3 * PI / 2] if case.a == '2pi' else [-PI / 2, 0.0, PI / 2])
    if case.dup:
        fam = dict(r=r_b, e=e_b, a=a_b)
        fam[case.dup] = _near_duplicates(rng, fam[case.dup])
        r_b, e_b, a_b = fam['r'], fam['e'], fam['a']
    r1 = case.r[1]
    n_tie = 400 if case.tie else 0
    n = case.n - n_tie
    h = n // 2
    xs, d = np.empty((n, 3)), np.empty((n, 3))
    v = rng.normal(size=(h, 3))
    xs[:h] = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(1.6, 4.0, (h, 1))
    w = rng.normal(size=(h, 3))
    tgt = w / np.linalg.norm(w, axis=1, keepdims=True) * r1 * rng.uniform(0, 1, (h, 1)) ** (1 / 3)
    d[:h] = tgt - xs[:h]
    xs[h:] = rng.uniform(-1.1, 1.1, (n - h, 3)) * r1
    d[h:] = rng.normal(size=(n - h, 3))
    if n_tie:
        lx, ld = _lattice_rays(rng, n_tie, r1)
        xs, d = np.concatenate([xs, lx]), np.concatenate([d, ld])
    import torch as tr
    from sph_raytracer_amd import ViewGeom
    d = ViewGeom(tr.from_numpy(xs), tr.from_numpy(d)).rays.numpy().copy()   # as the geometry has them
    for a in (r_b, e_b, a_b, xs, d):
        a.setflags(write=False)
    return r_b, e_b, a_b, xs, d


def tie_rays(name):
    """Bool per ray: the lattice rays of a `tie` case."""
    case = BY_NAME[name]
    m = np.zeros(case.n, bool)
    if case.tie:
        m[-400:] = True
    return m


def K_of(name):
    nr, ne, na = (len(b) - 1 for b in build(name)[:3])
    return 2 * (nr + 1) + 2 * (ne + 1) + (na + 1) + 1


def make(name):
    """-> (SphericalGrid, ViewGeom) of a case."""
    import torch as tr
    from sph_raytracer_amd import SphericalGrid, ViewGeom
    r_b, e_b, a_b, xs, d = build(name)
    grid = SphericalGrid(r_b=tr.from_numpy(r_b.copy()), e_b=tr.from_numpy(e_b.copy()),
                         a_b=tr.from_numpy(a_b.copy()))
    geom = ViewGeom(tr.from_numpy(xs.copy()), tr.from_numpy(d.copy()))
    geom.rays = tr.from_numpy(d.copy())     # (a second normalisation may move a last bit: the
    return grid, geom                       # oracle and the device trace the same directions)


def _oracle():
    from oracle import oracle
    oracle.use_mkl_sqrt(False)
    return oracle


@functools.lru_cache(maxsize=None)
def starts(name):
    import torch as tr
    from sph_raytracer_amd.raytracer import find_starts
    grid, _ = make(name)
    s = find_starts(grid, tr.from_numpy(build(name)[3].copy())).numpy()
    s.setflags(write=False)
    return s


Reference = namedtuple('Reference', 'segs n_vox x y yt xt seconds')


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's answer for a case (IEEE square roots), computed once: its segments (ptr, vox,
    len), a random density x of the grid's shape with its forward y, a random yt per ray with its
    adjoint xt, and the seconds the trace took.  Arrays are numpy float64; read-only."""
    import time
    ora = _oracle()
    r_b, e_b, a_b, xs, d = build(name)
    g = ora.Grid.from_boundaries(r_b.copy(), e_b.copy(), a_b.copy())
    t0 = time.perf_counter()
    segs = ora.trace_segments(g, xs, d, starts(name))
    seconds = time.perf_counter() - t0
    shape = (g.nr, g.ne, g.na)
    n_vox = math.prod(shape)
    rng = np.random.default_rng(_seed(BY_NAME[name]) + 500)
    x = rng.random(shape)
    yt = rng.random(len(xs))
    y = np.asarray(ora.forward(*segs, x, n_vox)).reshape(-1)
    xt = np.asarray(ora.adjoint(*segs, yt, n_vox)).reshape(shape)
    for a in segs + (x, y, yt, xt):
        a.setflags(write=False)
    return Reference(segs, n_vox, x, y, yt, xt, seconds)


def _bits(t):
    return (np.asarray(t, np.float64) + 0.0).view(np.uint64)        # -0 -> +0, as push()


def _rung(F, n_other):
    if F > 512:
        return 'lds'
    if F <= 64:
        return 'regs1'
    if F <= 128:
        return 'merge2_1' if n_other <= 64 else 'regs2'
    if F <= 256:
        return 'merge4_1' if n_other <= 64 else 'merge4_2' if n_other <= 128 else 'regs4'
    return 'merge8_2' if n_other <= 128 else 'merge8_4' if n_other <= 256 else 'regs8'


def _fill(F):
    return 0 if F > 512 else next(m for m, hi in zip(FILLS, _FILL_EDGES[1:]) if F <= hi)


def _clear(v, edges, margin=2):
    """v is at least `margin` away from every threshold `v <= edge` of `edges` on either side."""
    return all(v <= e - margin or v >= e + 1 + margin for e in edges)


def _other_edges(F):
    """The n_other thresholds that choose the rung at list length F."""
    return [] if F <= 64 or F > 512 else [64] if F <= 128 else [64, 128] if F <= 256 else [128, 256]


def _first_conflict(t, cand, reg, r_lim, e_lim, start_c, sv):
    """Index in the (distance, candidate)-sorted list of the first group of equal distances in
    which two entries write different values to one region row (tie_groups_ambiguous), or -1."""
    order = np.lexsort((cand, t))
    t, cand, reg = t[order], cand[order], reg[order]
    eq = np.flatnonzero(t[1:] == t[:-1])
    if len(eq) == 0:
        return -1
    starts_ = np.flatnonzero(np.concatenate([[True], t[1:] != t[:-1]]))
    ends = np.concatenate([starts_[1:], [len(t)]])
    for g0, g1 in zip(starts_, ends):
        if g1 - g0 < 2:
            continue
        seen = [set(), set(), set()]
        for c, r in zip(cand[g0:g1], reg[g0:g1]):
            if c == start_c:
                for row in range(3):
                    seen[row].add(int(sv[row]))
            elif c < r_lim:
                seen[0].add(int(r))
            elif r != -2:
                seen[1 if c < e_lim else 2].add(int(r))
        if any(len(s) > 1 for s in seen):
            return int(g0)
    return -1


Classes = namedtuple('Classes', 'hit inside F s_near nfar n_other rung fill interior_rung '
                     'interior_fill chunks_r chunks_e total_r total_e skip_before skip_after wedge '
                     'p_start p_count near_pair shell_disorder first_conflict')


@functools.lru_cache(maxsize=None)
def list_classes(name):
    """trace_one's ladder restated in numpy from oracle.solve (IEEE square roots), per ray:

    hit            the ray is traced at all (screen_kernel: a valid start shell, or the outer
                   sphere's chord is not NaN); everything below is meaningful for hit rays only
    inside         the start lies in a voxel (start_ok)
    F, s_near, nfar, n_other   the list's length, its near / far shell entries, the rest: the
                   crossings kept by trace_one's `keep` (finite, not negative, not beyond t_hi, not
                   before t_lo when t_lo > 0; t_lo / t_hi the outer shell's crossings, t_hi = inf
                   for a valid start shell whose exit is behind the start), less the second of a
                   double root writing the same region, plus the start entry when t_lo <= 0
    rung, fill     the sort rung (RUNGS) and the fill width (FILLS; 0 = the LDS chunk loop)
    interior_rung, interior_fill   F and n_other are at least 2 away from every edge of the rung /
                   the fill: the device takes t_lo / t_hi from make_ray, so its F may differ by one
                   or two on a few rays
    chunks_r, chunks_e, total_r, total_e   64-wide chunks the device solves for the shells / cones
                   (from the first boundary that can cross, those holding one that can:
                   sphere_may_cross, cone_q_may_cross) and ceil(boundaries / 64); equal for a
                   family of at most 64 boundaries (one chunk, no pre-pass)
    skip_before, skip_after   a chunk is saved before the first solved one (the pre-pass starts
                   the chunks late enough to need fewer) / a chunk after it holds no boundary that
                   can cross (the ballot skips it), in some family of more than 64 boundaries
    wedge, p_start, p_count   the half-plane wedge applies (more than 64 half-planes, start
                   outside every voxel, finite t_hi, line away from the z axis, one cyclic run)
                   and its run [p_start, p_start + p_count) mod nba
    near_pair      two adjacent listed distances agree above the candidate-bit mask (cbits) without
                   being equal
    shell_disorder the shell run's composite keys, read as merge_sort reads them, do not ascend
                   strictly (shell_run_ascending is false)
    first_conflict index in the sorted list of the first tie group that writes different values to
                   one row; -1 when there is none
    Distances come from the oracle's per-family solves, with the direction normalised as the
    trace hands it to each family up to the rounding of a norm; the device's own may differ in
    the last bits, which moves a few rays across an edge (hence `interior_*`) but no class count
    by much."""
    ora = _oracle()
    r_b, e_b, a_b, xs, d = build(name)
    g = ora.Grid.from_boundaries(r_b.copy(), e_b.copy(), a_b.copy())
    nbr, nbe, nba = len(r_b), len(e_b), len(a_b)
    nr, ne, na = nbr - 1, nbe - 1, nba - 1
    K = g.K
    cmask = np.uint64((1 << (K - 1).bit_length()) - 1)
    n = len(xs)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    w = u / np.linalg.norm(u, axis=1, keepdims=True)
    tr_, rr_, _ = ora.solve(g, 0, xs, d)        # r_torch normalises once: u
    te_, re_, _ = ora.solve(g, 1, xs, u)        # e_torch once more: w
    ta_, ra_, _ = ora.solve(g, 2, xs, w)        # a_torch takes w as it is
    s = starts(name)
    sr, se, sa = s[0], s[1], s[2]
    r_ok = (sr >= 0) & (sr < nr)
    inside = r_ok & (se >= 0) & (se < ne) & (sa >= 0) & (sa < na)
    t_in_o, t_out_o = tr_[:, nr], tr_[:, nbr + nr]
    chord = np.isfinite(t_out_o)
    hit = r_ok | chord
    t_lo = np.where(chord, t_in_o, -np.inf)
    t_hi = np.where(chord, t_out_o, np.inf)
    t_hi = np.where(r_ok & (t_hi < 0), np.inf, t_hi)
    clip_lo = t_lo > 0

    def keep(t):
        return (np.isfinite(t) & ~(t < 0) & ~(t > t_hi[:, None]) &
                ~(clip_lo[:, None] & (t < t_lo[:, None])))

    def pairs(t, reg, nb):     # (kept first roots, kept second roots less the double roots)
        a, b = t[:, :nb], t[:, nb:]
        return keep(a), keep(b) & ~((a == b) & (reg[:, :nb] == reg[:, nb:]))
    k_near, k_far = pairs(tr_, rr_, nbr)
    k_e1, k_e2 = pairs(te_, re_, nbe)
    k_a = keep(ta_)
    s_near, nfar = k_near.sum(1), k_far.sum(1)
    start_entry = ~clip_lo
    n_other = k_e1.sum(1) + k_e2.sum(1) + k_a.sum(1) + start_entry
    F = s_near + nfar + n_other

    # chunk skipping: spheres by R^2 - dd^2 >= 0 (the solve's own finiteness), cones by the
    # snapped discriminant (solve.hpp cone_coeffs / cone_q_may_cross, in numpy)
    may_r = np.isfinite(tr_[:, :nbr]) | np.isfinite(tr_[:, nbr:])
    c2 = np.asarray(g._keep[4])
    wx = (w * xs).sum(1)
    nx2 = (xs * xs).sum(1)
    aa = w[:, 2:3] ** 2 - c2[None]
    bb = 2 * (w[:, 2:3] * xs[:, 2:3] - wx[:, None] * c2[None])
    cc = xs[:, 2:3] ** 2 - nx2[:, None] * c2[None]
    aa = np.where(np.abs(aa) < g.th, 0.0, aa)
    delta = bb * bb - 4 * aa * cc
    delta = np.where(np.abs(delta) < g.th, 0.0, delta)
    may_e = (delta >= 0) | ((np.abs(aa) < g.th) & ~(np.abs(bb) < g.th))

    def chunks(may, nb):
        total = -(-nb // 64)
        solved = np.full(n, total)
        before = np.zeros(n, bool)
        after = np.zeros(n, bool)
        if nb <= 64:
            return solved, total, before, after
        for i in range(n):
            idx = np.flatnonzero(may[i])
            if len(idx) == 0:
                solved[i], before[i] = 0, True
                continue
            first = int(idx[0])
            ran = -(-(nb - first) // 64)
            has = np.unique((idx - first) // 64)
            solved[i] = len(has)
            before[i] = ran < total
            after[i] = len(has) < ran
        return solved, total, before, after
    chunks_r, total_r, before_r, after_r = chunks(may_r, nbr)
    chunks_e, total_e, before_e, after_e = chunks(may_e, nbe)

    # the wedge (trace_one), from the twice-normalised direction
    a_asc = bool((np.diff(a_b) > 0).all())
    Lz = xs[:, 0] * w[:, 1] - xs[:, 1] * w[:, 0]
    wedge = np.zeros(n, bool)
    p_start = np.zeros(n, np.int64)
    p_count = np.full(n, nba)
    cos_a, sin_a = np.asarray(g._keep[5]), np.asarray(g._keep[6])
    if nba > 64 and a_asc:
        can = hit & ~inside & np.isfinite(t_hi) & (Lz * Lz >= 1e-12 * (w[:, 0] ** 2 + w[:, 1] ** 2))
        for i in np.flatnonzero(can):
            x0, x1 = xs[i, 0], xs[i, 1]
            b0, b1 = x0 + t_hi[i] * w[i, 0], x1 + t_hi[i] * w[i, 1]
            tol_a = 1e-12 * (x0 * x0 + x1 * x1) * Lz[i] ** 2
            tol_b = 1e-12 * (b0 * b0 + b1 * b1) * Lz[i] ** 2
            ca = (x0 * sin_a - x1 * cos_a) * Lz[i]
            cb = (cos_a * b1 - sin_a * b0) * Lz[i]
            inn = ((ca >= 0) | (ca * ca <= tol_a)) & ((cb >= 0) | (cb * cb <= tol_b))
            cnt = int(inn.sum())
            run_starts = np.flatnonzero(inn & ~np.roll(inn, 1))
            if cnt == 0:
                wedge[i], p_count[i] = True, 0
            elif len(run_starts) == 1:
                wedge[i], p_start[i], p_count[i] = True, run_starts[0], cnt
            elif cnt == nba:        # every half-plane: no run start, the default run stays
                wedge[i] = True

    # per-ray list properties (the listed distances, candidates and regions)
    r_lim, e_lim, start_c = 2 * nbr, 2 * nbr + 2 * nbe, K - 1
    near_pair = np.zeros(n, bool)
    shell_disorder = np.zeros(n, bool)
    first_conflict = np.full(n, -1)
    all_t = np.concatenate([tr_, te_, ta_], 1)
    all_reg = np.concatenate([rr_, re_, ra_], 1)
    all_keep = np.concatenate([k_near, k_far, k_e1, k_e2, k_a], 1)
    for i in np.flatnonzero(hit):
        cand = np.flatnonzero(all_keep[i])
        t, reg = all_t[i, cand], all_reg[i, cand]
        if start_entry[i]:
            cand, t, reg = np.append(cand, start_c), np.append(t, 0.0), np.append(reg, 0)
        tb = np.sort(_bits(t))
        hi_bits = tb & ~cmask
        near_pair[i] = bool(((hi_bits[1:] == hi_bits[:-1]) & (tb[1:] != tb[:-1])).any())
        jn, jf = np.flatnonzero(k_near[i]), np.flatnonzero(k_far[i])
        run = np.concatenate([(_bits(tr_[i, jn[::-1]]) & ~cmask) | jn[::-1].astype(np.uint64),
                              (_bits(tr_[i, nbr + jf]) & ~cmask) | (nbr + jf).astype(np.uint64)])
        shell_disorder[i] = bool((run[1:] <= run[:-1]).any())
        first_conflict[i] = _first_conflict(t, cand, reg, r_lim, e_lim, start_c, s[:, i])

    rung = np.array([_rung(f, o) for f, o in zip(F, n_other)])
    fill = np.array([_fill(f) for f in F])
    interior_rung = np.array([_clear(f, _F_EDGES[1:]) and _clear(o, _other_edges(f)) and f >= 2
                              for f, o in zip(F, n_other)])
    interior_fill = np.array([_clear(f, _FILL_EDGES[1:]) and f >= 2 for f in F])
    out = Classes(hit, inside, F, s_near, nfar, n_other, rung, fill, interior_rung, interior_fill,
                  chunks_r, chunks_e, total_r, total_e, before_r | before_e, after_r | after_e,
                  wedge, p_start, p_count, near_pair, shell_disorder, first_conflict)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
