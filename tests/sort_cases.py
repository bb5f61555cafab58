"""Adversarial lists for the exact path's sort emulations (csrc/introsort.hpp and the wave-parallel
sort of csrc/trace.hip), with the host side of what the device must reproduce.

A *list* is what the trace hands its sort for one ray: K distances in concatenation order (2 nbr
sphere roots, 2 nbe cone roots, the half-planes, the start entry last), the region each entry
writes, and the ray's start voxel.  The device sorts it with the reference's unstable introsort;
the oracle (oracle.introsort_ranges) gives that order and the ranges the depth limit heap-sorts.

`families(K)` builds the distance lists, deterministically from K; `payloads(setting, t)` the
region / start / boundary-count side in one of three settings whose expected branch is known:

    conflict     every entry but the start is a sphere crossing, all regions distinct: every tie
                 of live entries conflicts, so a depth-limit range with one must be heap-sorted
    noconflict   one region everywhere: nothing conflicts, every range must be rank-sorted
    mixed        random families and regions, with "no update" (-2) cone and plane entries

`replay` is the walk's region-row updates over an ordered list — the definition of "the same
segments" that the rank-sort shortcut and the register network claim."""
import numpy as np

NO_UPDATE = -2
INF = np.inf
SETTINGS = ('conflict', 'noconflict', 'mixed')


# ---- distance families --------------------------------------------------------------------------
def organ_pipe(K, q=1, rot=0):
    """Ascending then descending (a ray's two roots per shell), quantised by // q, rotated."""
    h = (K + 1) // 2
    x = np.concatenate([np.arange(h), np.arange(K - h)[::-1]]).astype(np.float64)
    return np.roll(x // q, rot)


def killer(K, q=2):
    """Musser's median-of-three killer (every pivot the second smallest of its range), values
    quantised by // q so that the ranges that reach the depth limit hold ties."""
    n = K - (K & 1)
    k = n // 2
    a = np.zeros(K, np.float64)
    for i in range(1, k + 1):
        if i & 1:
            a[i - 1] = i
            if i < k:
                a[i] = k + i
        a[k + i - 1] = 2 * i
    if k and not k & 1:
        a[k - 1] = 2 * k - 1
    if K & 1:
        a[K - 1] = K
    return a // q


def with_misses(x, frac):
    """The largest `frac` of the values -> +inf (crossings that miss)."""
    x = x.copy()
    if len(x) > 1:
        x[x > np.quantile(x, 1.0 - frac)] = INF
    return x


def top_misses(x, m):
    """The m largest values -> +inf."""
    y = x.copy()
    y[x >= np.sort(x)[-m]] = INF
    return y


# Lists with two or more +inf inside one depth-limit range (what invalid=True must heap-sort):
# organ pipes (quantiser q) with their m largest values turned into misses.  Ties of +inf
# partition evenly, so such ranges are rare: a search over every m for pipes, killers and their
# negations at the K of the GPU tests found them only at the two largest.  {K: [(q, m), ...]}
INF_IN_RANGE = {1733: [(1, 1386), (2, 878), (2, 1387)], 1798: [(1, 159), (1, 1463), (2, 1464)]}


POOL = np.array([-INF, INF, 0.0, -0.0, 1.0, 2.0, -1.0, 0.5, -2.5, 3.0])


def pool(K, rng):
    """Tie-heavy random lists from a small pool with ±0, ±inf and negatives."""
    kind = int(rng.integers(3))
    if kind == 0:
        return rng.choice(POOL, K)
    if kind == 1:
        return np.where(rng.random(K) < 0.3, INF, rng.choice(POOL, K))
    return np.where(rng.random(K) < 0.3, np.round(rng.normal(size=K), 1), rng.choice(POOL, K))


def trace_like(K, rng):
    """A ray's list: per shell the entry root (descending in the shell index) and the exit root
    (ascending), +inf for the shells inside the impact parameter; two roots per cone; one per
    half-plane; the start entry last at t = 0.  Distances in sixteenths: exact ties, and exactly
    representable in float32."""
    if K < 6:
        return np.concatenate([np.round(rng.normal(2, 2, K - 1) * 16) / 16, [0.0]])
    nbr = max(1, int(0.4 * (K - 1)) // 2 * 2 // 2)
    nbe = max(1, int(0.2 * (K - 1)))
    while 2 * nbr + 2 * nbe > K - 2:
        nbr, nbe = max(1, nbr - 1), max(1, nbe - 1)
    nba = K - 1 - 2 * nbr - 2 * nbe
    tc = rng.uniform(-2, 6)
    b = rng.uniform(0, 0.6)
    r = np.linspace(0.1, 1.0, nbr) * (1 + nbr / 8)
    h = np.sqrt(np.maximum(r * r - b * b, 0.0))
    hit = r > b
    ti = np.where(hit, tc - h, INF)
    to = np.where(hit, tc + h, INF)
    ce = rng.uniform(-3, 8, (2, nbe))
    ce[rng.random((2, nbe)) < 0.3] = INF
    pa = rng.uniform(-3, 8, nba)
    pa[rng.random(nba) < 0.3] = INF
    x = np.concatenate([ti, to, ce[0], ce[1], pa, [0.0]])
    return np.round(x * 16) / 16


def families(K, n_random=12, seed=0):
    """{name: (n, K) float64} — every family at this K.  NaN-free."""
    rng = np.random.default_rng([seed, K])
    fam = {}
    pipes = [organ_pipe(K, q, rot) for q in (1, 2, 3) for rot in (0, 1, K // 3)]
    pipes += [with_misses(organ_pipe(K, q), f) for q in (1, 2) for f in (0.1, 0.3)]
    pipes += [top_misses(organ_pipe(K, q), m) for q, m in INF_IN_RANGE.get(K, [])]
    fam['pipe'] = np.stack(pipes)
    kill = [killer(K, 2), killer(K, 4), with_misses(killer(K, 2), 0.1),
            with_misses(killer(K, 2), 0.3), -killer(K, 2)]
    fam['killer'] = np.stack(kill)
    fam['pool'] = np.stack([pool(K, rng) for _ in range(n_random)])
    fam['trace'] = np.stack([trace_like(K, rng) for _ in range(n_random)])
    fam['equal'] = np.stack([np.full(K, v) for v in (1.0, INF, 0.0, -1.0)])
    few = []
    for cut in sorted({0, 1, K // 2, K - 1}):
        lo_hi = np.where(np.arange(K) < cut, 1.0, 2.0)
        few += [lo_hi, lo_hi[::-1].copy()]
    few += [np.where(np.arange(K) < K // 2, 0.5, INF), np.where(np.arange(K) < K // 2, INF, 0.5)]
    fam['few'] = np.stack(few)
    for v in fam.values():
        assert v.shape[1] == K and not np.isnan(v).any()
    return fam


# ---- payload settings ---------------------------------------------------------------------------
class Lists:
    """n lists of K entries with their payload side."""

    def __init__(self, t, reg, start, nbr, nbe, names):
        self.t = np.ascontiguousarray(t, np.float64)
        self.reg = np.ascontiguousarray(reg, np.int32)
        self.start = np.ascontiguousarray(start, np.int32)
        self.nbr, self.nbe, self.names = int(nbr), int(nbe), list(names)
        self.n, self.K = self.t.shape
        assert self.reg.shape == self.t.shape and self.start.shape == (self.n, 3)
        assert self.reg.min() >= NO_UPDATE and self.reg.max() + 2 < 1 << 16


def payloads(setting, t, names, seed=0):
    n, K = t.shape
    rng = np.random.default_rng([seed, K, SETTINGS.index(setting)])
    if setting == 'conflict':
        # 2 nbr >= K - 1: every entry before the start entry is a sphere crossing
        reg = np.broadcast_to(np.arange(K) % 60000, (n, K))
        start = np.broadcast_to(np.array([60001, 60002, 60003]), (n, 3))
        return Lists(t, reg, start, K // 2, 0, names)
    if setting == 'noconflict':
        return Lists(t, np.full((n, K), 3), np.full((n, 3), 3), K // 3, K // 5, names)
    nbr, nbe = K // 3, K // 5
    reg = rng.integers(0, 4, (n, K))
    skip = (rng.random((n, K)) < 0.3) & (np.arange(K) >= 2 * nbr)
    reg[skip] = NO_UPDATE
    return Lists(t, reg, rng.integers(0, 4, (n, 3)), nbr, nbe, names)


def cases(K, n_random=12, seed=0):
    """{setting: Lists} over every family at K (the same distances in each setting)."""
    fam = families(K, n_random, seed)
    t = np.concatenate(list(fam.values()))
    names = [f'{k}[{i}]' for k, v in fam.items() for i in range(len(v))]
    return {s: payloads(s, t, names, seed) for s in SETTINGS}


# ---- the walk's updates, on the host ------------------------------------------------------------
def entry_rows(c, reg, K, r_lim, e_lim, start):
    """(rows set by entry c as a bit mask r=1 e=2 a=4, the three values) — trace.hip entry_rows."""
    if c == K - 1:
        return 7, tuple(int(v) for v in start)
    if c < r_lim:
        return 1, (reg, reg, reg)
    if c < e_lim:
        return (2 if reg != NO_UPDATE else 0), (reg, reg, reg)
    return (4 if reg != NO_UPDATE else 0), (reg, reg, reg)


def entries_conflict(ca, cb, L, i):
    """Two entries of list i set one region row to different values."""
    r_lim, e_lim = 2 * L.nbr, 2 * L.nbr + 2 * L.nbe
    ma, va = entry_rows(ca, int(L.reg[i, ca]), L.K, r_lim, e_lim, L.start[i])
    mb, vb = entry_rows(cb, int(L.reg[i, cb]), L.K, r_lim, e_lim, L.start[i])
    m = ma & mb
    return any((m >> k) & 1 and va[k] != vb[k] for k in range(3))


def live(t, invalid):
    """An entry whose update can be read: t >= 0 and, without invalid=True, finite."""
    return t >= 0.0 and (invalid or t < INF)


def replay(t_sorted, order, L, i, invalid=False):
    """The walk over list i in the given order (`order[k]` the list position of the k-th entry,
    t_sorted[k] its distance): the (distance, r, e, a) state after every maximal group of equal
    distances that the walk reads — without invalid, up to the first +inf — and, for invalid, the
    order inside the infinite group (each of its NaN-long segments is kept)."""
    K = L.K
    r_lim, e_lim = 2 * L.nbr, 2 * L.nbr + 2 * L.nbe
    state = [int(v) for v in L.start[i]]
    states = []
    k = 0
    while k < K:
        tv = t_sorted[k]
        if not invalid and tv == INF:
            break
        j = k
        while j < K and t_sorted[j] == tv:
            if not tv < 0.0:
                c = int(order[j])
                m, v = entry_rows(c, int(L.reg[i, c]), K, r_lim, e_lim, L.start[i])
                for row in range(3):
                    if (m >> row) & 1:
                        state[row] = v[row]
            j += 1
        states.append((float(tv) + 0.0, *state))
        k = j
    inf_order = [int(c) for c, tv in zip(order, t_sorted) if tv == INF] if invalid else None
    return states, inf_order


def range_has_live_tie(t_sorted, first, last, invalid):
    seg = t_sorted[first:last]
    eq = seg[1:] == seg[:-1]
    return bool(any(e and live(v, invalid) for e, v in zip(eq, seg[1:])))


def range_is_ambiguous(t_sorted, order, first, last, L, i, invalid):
    """exact_heap_range's decision on a depth-limit range: a tie of live entries that conflict
    (invalid: any two infinite ones)."""
    k = first
    while k < last:
        j = k
        while j < last and t_sorted[j] == t_sorted[k]:
            j += 1
        if j - k > 1 and live(t_sorted[k], invalid):
            if invalid and t_sorted[k] == INF:
                return True
            # some pair conflicts <=> some row is set to two different values inside the group
            r_lim, e_lim = 2 * L.nbr, 2 * L.nbr + 2 * L.nbe
            seen = [set(), set(), set()]
            for a in range(k, j):
                c = int(order[a])
                m, v = entry_rows(c, int(L.reg[i, c]), L.K, r_lim, e_lim, L.start[i])
                for row in range(3):
                    if (m >> row) & 1:
                        seen[row].add(v[row])
            if any(len(s) > 1 for s in seen):
                return True
        k = j
    return False


def outside(K, ranges):
    """Mask of the sorted positions outside every depth-limit range."""
    m = np.ones(K, bool)
    for f, l in ranges:
        m[f:l] = False
    return m


def is_float32_valued(t):
    return bool(np.array_equal(t.astype(np.float32).astype(np.float64), t))
