"""What makes tests/test_gpu_trace_cases.py meaningful, checked on the CPU alone.

On trace_cases.list_classes — the numpy restatement of trace_one's ladder over the C oracle's
solves — the cases of trace_cases.py are shown to hold every input the GPU test is there for:
each of the ten sort rungs and seven fill paths with rays well inside it, skipped 64-wide chunks
before and after the first solved one, wedge runs that wrap past the last half-plane, distances
that agree above the candidate bits without being equal (and shell runs they leave out of order),
and conflicting tie groups beyond the first and second 64-entry chunk.  This asserts that the
inputs occur, not that the kernel treats them rightly.

A ray counts for a rung or a fill only when `interior`: its F and n_other at least 2 away from
every edge of it, since the device derives the outer sphere's span from its own set-up and may
list one or two entries more or fewer on a few rays.  Rays counted for a near-tie input have no
conflicting tie group, so the wave path (not the exact path they would be deferred to) emits
them.

No ray is masked from the GPU test's length contract: the masked count is 0 in every case.
"""
import numpy as np
import pytest

import trace_cases as tc

MIN_RAYS = 16

# rung / fill -> the named case that must reach it with MIN_RAYS interior rays
RUNG_CASE = dict(regs1='small_30x20x12', merge2_1='shells_124x6x6_dup_r',
                 regs2='az_5x5x144_dup_a', merge4_1='shells_124x6x6_dup_r',
                 merge4_2='wide_100x100x150_tie', regs4='cones_10x150x360_dup_e',
                 merge8_2='lds_300x10x10', merge8_4='wide_100x100x150_tie',
                 regs8='cones_10x150x360_dup_e', lds='lds_300x10x10')
FILL_CASE = {1: 'small_30x20x12', 2: 'az_5x5x144_dup_a', 3: 'cones_10x150x360_dup_e',
             4: 'k512_150x60x86', 6: 'k514_150x60x88', 8: 'lds_300x10x10', 0: 'lds_300x10x10'}
# A list of more than 512 entries needs nearly the whole chord of a 300-shell grid through its
# centre (every shell twice): a start inside a voxel lists only what lies ahead of it, and no
# random start inside the ball sits at the outer shell aimed at the centre.  The LDS sort and the
# LDS fill are reached by lines from outside only.
OUTSIDE_ONLY = {'lds', 0}

WIDE = [n for n in tc.NAMES if max(len(b) for b in tc.build(n)[:2]) > 64]
# An after-skip needs a chunk's worth of boundaries that cannot cross behind one that can.
# sphere_may_cross is monotone in the radius (every shell beyond the first that can cross can), so
# shells never give one; cones do (a line's elevations reach the cones of a band and of its mirror
# image about pi / 2, not those between), when there are enough of them: with 65 cones the chunks
# start at the first cone that can cross and one chunk covers the rest.
SKIP_AFTER = [n for n in tc.NAMES if len(tc.build(n)[1]) > 90]
WIDE_A = [n for n in tc.NAMES if len(tc.build(n)[2]) > 64]
DUP = [c.name for c in tc.CASES if c.dup]
DUP_R = [c.name for c in tc.CASES if c.dup == 'r']
TIE = [c.name for c in tc.CASES if c.tie]


def _m(name):
    return np.array([tc.RUNG_M[r] for r in tc.list_classes(name).rung])


def test_case_set():
    """The grids the cases promise: families over 64 boundaries, K on both sides of 512, hollow
    and solid, full and partial ranges, the four azimuth ranges, near-duplicates per family."""
    nb = {n: tuple(len(b) for b in tc.build(n)[:3]) for n in tc.NAMES}
    assert sum(v[0] > 64 for v in nb.values()) >= 4
    assert sum(v[1] > 64 for v in nb.values()) >= 3
    assert sum(v[2] > 64 for v in nb.values()) >= 4
    assert any(min(v) > 64 for v in nb.values())
    assert tc.K_of('k512_150x60x86') == 512 and tc.K_of('k514_150x60x88') == 514
    r_lo = [tc.build(n)[0][0] for n in tc.NAMES]
    assert min(r_lo) == 0.0 and max(r_lo) > 0.0
    e = [(tc.build(n)[1][0], tc.build(n)[1][-1]) for n in tc.NAMES]
    assert (0.0, np.pi) in e and any(lo > 0 and hi < np.pi for lo, hi in e)
    a = [(tc.build(n)[2][0], tc.build(n)[2][-1]) for n in tc.NAMES]
    assert (-np.pi, np.pi) in a and (0.0, 2 * np.pi) in a
    assert any(lo > 0 for lo, hi in a)                              # partial, without 0
    assert any(-np.pi < lo < 0 < hi < np.pi for lo, hi in a)        # partial, across 0
    assert sorted(tc.BY_NAME[n].dup for n in DUP) == ['a', 'e', 'r', 'r']
    assert len(TIE) >= 3 and all(max(nb[n]) > 64 for n in TIE)
    for name in tc.NAMES:
        r_b, e_b, a_b, xs, d = tc.build(name)
        assert len(xs) == len(d) == tc.BY_NAME[name].n <= 2000
        assert np.abs(xs).max() < tc.SCALE and r_b[-1] < tc.SCALE
        for b in (r_b, e_b, a_b):
            assert (np.diff(b) > 0).all()


@pytest.mark.parametrize('name', DUP)
def test_near_duplicate_boundaries(name):
    """tc.N_DUP pairs 1 ulp apart and as many 4 ulps apart, every gap under 1e-12 x the scale
    (compare_segments drops the sliver voxel's segments)."""
    b = tc.build(name)['rea'.index(tc.BY_NAME[name].dup)]
    gaps = np.diff(b)
    ulps = np.rint(gaps / np.spacing(np.maximum(np.abs(b[:-1]), np.abs(b[1:]))))
    assert int((ulps == 1).sum()) == tc.N_DUP and int((ulps == 4).sum()) == tc.N_DUP
    assert gaps[ulps <= 4].max() < 1e-12 * tc.SCALE and gaps[ulps > 4].min() > 1e-6


@pytest.mark.parametrize('name', TIE)
def test_tie_grids_hold_the_lattice_boundaries(name):
    r_b, e_b, a_b, _, _ = tc.build(name)
    assert 0.5 in r_b and 1.0 in r_b and np.pi / 2 in e_b
    marks = [np.pi / 2, np.pi, 3 * np.pi / 2] if a_b[0] == 0 else [-np.pi / 2, 0.0, np.pi / 2]
    assert all(m in a_b for m in marks)
    assert tc.tie_rays(name).sum() == 400


@pytest.mark.parametrize('rung', tc.RUNGS)
def test_every_sort_rung_is_reached(rung):
    c = tc.list_classes(RUNG_CASE[rung])
    m = c.hit & (c.rung == rung) & c.interior_rung
    print(f'{rung} in {RUNG_CASE[rung]}: {m.sum()} interior rays, {(m & c.inside).sum()} from '
          f'inside a voxel')
    assert m.sum() >= MIN_RAYS
    assert (m & ~c.inside).sum() >= 4
    if rung not in OUTSIDE_ONLY:
        assert (m & c.inside).sum() >= 4


@pytest.mark.parametrize('fill', tc.FILLS)
def test_every_fill_path_is_reached(fill):
    c = tc.list_classes(FILL_CASE[fill])
    m = c.hit & (c.fill == fill) & c.interior_fill
    print(f'fill {fill} in {FILL_CASE[fill]}: {m.sum()} interior rays, {(m & c.inside).sum()} '
          f'from inside a voxel')
    assert m.sum() >= MIN_RAYS
    assert (m & ~c.inside).sum() >= 4
    if fill not in OUTSIDE_ONLY:
        assert (m & c.inside).sum() >= 4


@pytest.mark.parametrize('name', WIDE)
def test_chunks_are_skipped(name):
    """More than 64 shells or cones: rays that solve fewer chunks than the family has, with a
    chunk saved before the first solved one, and (SKIP_AFTER) one skipped after it."""
    c = tc.list_classes(name)
    fewer = c.hit & ((c.chunks_r < c.total_r) | (c.chunks_e < c.total_e))
    assert fewer.sum() >= MIN_RAYS
    assert (c.hit & c.skip_before).sum() >= MIN_RAYS
    if name in SKIP_AFTER:
        assert (c.hit & c.skip_after).sum() >= MIN_RAYS


def test_skip_after_cases():
    assert len(SKIP_AFTER) >= 3


@pytest.mark.parametrize('name', WIDE_A)
def test_wedge_runs_wrap(name):
    """More than 64 half-planes: wedge runs that wrap past index nba - 1, runs that do not, and
    rays without a wedge (starts inside a voxel)."""
    c = tc.list_classes(name)
    nba = len(tc.build(name)[2])
    run = c.hit & c.wedge & (c.p_count > 0) & (c.p_count < nba)
    wraps = run & (c.p_start + c.p_count > nba)
    assert wraps.sum() >= MIN_RAYS and (run & ~wraps).sum() >= MIN_RAYS
    assert (c.hit & ~c.wedge).sum() >= MIN_RAYS


@pytest.mark.parametrize('name', DUP)
def test_near_ties_reach_the_wide_sorts(name):
    """Near-duplicate boundaries: lists of more than 64 entries (M >= 2) in which two adjacent
    distances agree above the candidate bits without being equal; near-duplicate shells: in an
    M >= 4 merge rung, a shell run out of composite-key order (shell_run_ascending fails, the
    bitonic merge runs and fix_near_ties repairs)."""
    c = tc.list_classes(name)
    wave = c.hit & (c.first_conflict < 0)
    m = _m(name)
    assert (wave & c.near_pair & (m >= 2)).sum() >= MIN_RAYS
    if name in DUP_R:
        merge = np.char.startswith(c.rung, 'merge') & (m >= 4)
        assert (wave & merge & c.shell_disorder).sum() >= MIN_RAYS


def test_merge_path_is_reached():
    """Without near-duplicate shells the run ascends: M >= 4 merge rungs take merge_path."""
    c = tc.list_classes('lds_300x10x10')
    merge = np.char.startswith(c.rung, 'merge') & (_m('lds_300x10x10') >= 4)
    assert (c.hit & merge & c.interior_rung & ~c.shell_disorder).sum() >= MIN_RAYS


@pytest.mark.parametrize('name', TIE)
def test_late_tie_groups(name):
    """Lattice rays: conflicting tie groups whose first lies beyond the first 64-entry chunk of
    the sorted list (tie_groups_ambiguous carries grp and last[3] into it)."""
    c = tc.list_classes(name)
    late = c.hit & (c.first_conflict >= 64)
    assert late.sum() >= 8
    assert (c.hit & (c.first_conflict >= 0) & (c.first_conflict < 64)).sum() >= 8


def test_a_tie_group_beyond_the_second_chunk():
    assert max((tc.list_classes(n).first_conflict >= 128).sum() for n in TIE) >= 8


@pytest.mark.parametrize('name', tc.NAMES)
def test_miss_cap_and_oracle_time(name):
    """At most half of a case's rays miss the grid, and its oracle trace takes under 2 s."""
    ref = tc.reference(name)
    missed = np.diff(ref.segs[0]) == 0
    assert missed.mean() <= 0.5, f'{name}: {missed.mean():.2f} of the rays miss'
    assert ref.seconds < 2.0, f'{name}: oracle trace {ref.seconds:.2f} s'
    assert len(ref.segs[1]) > 1000
