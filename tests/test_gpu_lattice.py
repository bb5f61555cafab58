"""The HIP trace on lattice rays that tie exactly (tests/golden/lattice_*.npz, make_golden.py
lattice): 7^3 starts with coordinates in {-2, -1, -1/2, 0, 1/2, 1, 2} x the 26 directions with
components in {-1, 0, 1} = 8918 rays on four grids.  The rays pass through the z axis and the
origin, lie in half-planes and in the xy-plane (an e = pi/2 boundary), run along +-z, and start
exactly on shells, cones, the axis and at the origin — the inputs of ambiguous_ties /
tie_groups_ambiguous, fix_near_ties, the exact path's introsort emulation, the equal-valued ties
that stay on the wave path, segment_bound's through_axis and start_ok branches and (lattice_wide_a,
100 azimuth bins) the azimuth wedge.

Every ray, in every construction path (native, Python one-pass, Python two-pass), is held to the
C oracle with IEEE square roots (the GPU's arithmetic) under golden_cases.compare_segments: voxel
sequences exact once segments under 1e-12 x scale are dropped, lengths 1e-12 relative + 1e-12 x
scale.  The rays outside a fixture's `sqrt_sensitive` mask are also held to the reference's own
trace, forward (1e-10 / float32 1e-5 relative) and adjoint (1e-10 x max).  The mask marks the rays
whose voxel sequence the oracle's two sqrt modes (MKL, as the reference; IEEE) give differently: on
the hollow grid, rays starting exactly on the outer shell r = 1.5, where the reference's result
turns on the last bit of a square root.  It comes from the oracle at generation time, never from
the HIP code.

Masked rays per fixture (of 8918): lattice_full 0, lattice_a2pi 0, lattice_hollow 72,
lattice_wide_a 0 (dense regs under invalid=True, CPU tests only: lattice_f32 0, lattice_invalid
14).
Deferred / hit rays per fixture (rays the wave path hands to the exact path / rays with at least
one segment), printed by test_lattice_ties_exercised:
lattice_full 560 / 1428, lattice_a2pi 469 / 1287, lattice_hollow 834 / 3840, lattice_wide_a
536 / 1369.

What the lattice found in csrc/trace.hip (each kept as a named regression test below): the wave
path cut the crossing list at the outer sphere's exit although that exit rounds behind a start
on the sphere (24 lattice_hollow rays, all three paths); segment_bound gave 2 to lines through
the origin whose d^2 rounds below zero, and too little to tangents from a start on the outer
sphere, when the start's azimuth lies outside the grid (lattice_wide_a: the one-pass trace fell
back to the fill pass and the native construction to Python, silently).

What each test was checked to catch (mutations of csrc/trace.hip, each built and run once):
  - tie_groups_ambiguous returning false: test_lattice_trace_forward_adjoint (all 12),
    test_lattice_fused_and_atomic (all 4) and test_lattice_ties_exercised[lattice_a2pi] fail;
  - the wave path clipping at t_hi again (the first finding): test_lattice_trace_forward_adjoint
    [lattice_hollow-*] and test_start_on_outer_shell_exit_behind_start fail;
  - segment_bound taking `!(tb >= ta)` for a miss again (the second finding):
    test_lattice_bounds_hold[lattice_wide_a], the native and python_onepass path assertions of
    test_lattice_trace_forward_adjoint[lattice_wide_a-*] and
    test_line_through_origin_invalid_start_azimuth_bound fail;
  - the azimuth wedge's run of half-planes shortened by its first plane:
    test_lattice_trace_forward_adjoint[lattice_wide_a-*] and
    test_lattice_fused_and_atomic[lattice_wide_a] fail.
Not caught by any lattice test (the bounds stay above the counts): through_axis forced false in
segment_bound (a sweep of pi already counts every half-plane), its final + 4 dropped, and the
wedge's 1e-12 tolerance terms removed.  test_lattice_reference_modes_vs_oracle and
test_lattice_solvers run the reference-mode trace and sphrt_solve, which these mutations do not
touch; they were not mutated.
"""
import os
import sys

import numpy as np
import pytest
import torch as tr

import golden_cases as gc
from gpu_helpers import exact_stats

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

PATHS = ['native', 'python_onepass', 'python_twopass']
_TRACE_ENTRIES = ('sphrt_trace_bound', 'sphrt_trace_emit', 'sphrt_trace_count', 'sphrt_trace_fill')


def _oracle():
    from oracle import oracle
    oracle.use_mkl_sqrt(False)
    return oracle


@pytest.fixture(scope='module')
def lattice():
    """name -> (case, the IEEE-sqrt oracle's (ptr, vox, len), its forward of density0, its adjoint
    of y0): computed once per fixture, read-only."""
    cache = {}

    def get(name):
        if name not in cache:
            ora = _oracle()
            case = gc.load(name)
            g = ora.Grid.from_boundaries(case['r_b'], case['e_b'], case['a_b'])
            seg = ora.trace_segments(g, case['xs'], case['rays'], case['starts'])
            n_vox = int(np.prod(case['shape']))
            fwd = np.asarray(ora.forward(*seg, case['density0'], n_vox)).reshape(-1)
            adj = np.asarray(ora.adjoint(*seg, case['y0'], n_vox)).reshape(-1)
            for a in seg + (fwd, adj):
                a.setflags(write=False)
            cache[name] = (case, seg, fwd, adj)
        return cache[name]

    return get


def _geom(case):
    """FixtureGeom over copies of the stored rays (the cached case stays as loaded)."""
    return gc.FixtureGeom(dict(case, xs=case['xs'].copy(), rays=case['rays'].copy()))


def _count_calls(monkeypatch, names):
    """Counters over libsphrt entry points (raytracer.py looks them up per call)."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    calls = {k: 0 for k in names}
    for k in names:
        def counted(*args, _real=getattr(lib, k), _k=k):
            calls[_k] += 1
            return _real(*args)
        monkeypatch.setattr(lib, k, counted)
    return calls


def _construct(case, path, gpu, monkeypatch):
    """Operator over the fixture through one construction path, asserted to have run."""
    from sph_raytracer_amd import Operator, raytracer as rt
    for k in rt._NATIVE_OFF + ('SPHRT_CONSTRUCT',):
        monkeypatch.delenv(k, raising=False)
    if path != 'native':
        monkeypatch.setenv('SPHRT_CONSTRUCT', 'python')
        monkeypatch.setenv('SPHRT_TRACE', path.split('_')[1])
    calls = _count_calls(monkeypatch, _TRACE_ENTRIES)
    op = Operator(gc.make_grid(case), _geom(case), device=gpu)
    if path == 'native':        # csrc/construct.cpp build_rays: no Python trace call, no plan
        assert isinstance(op._batch, rt._NativeBatch) and op._plan is None
        assert not any(calls.values()), calls
    elif path == 'python_onepass':   # bound + emit, and no bound failed (no fill pass)
        assert op._plan is not None
        assert calls == dict(sphrt_trace_bound=1, sphrt_trace_emit=1, sphrt_trace_count=0,
                             sphrt_trace_fill=0), calls
    else:
        assert op._plan is not None
        assert calls == dict(sphrt_trace_bound=0, sphrt_trace_emit=0, sphrt_trace_count=1,
                             sphrt_trace_fill=1), calls
    return op


@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('name', gc.LATTICE_CASES)
def test_lattice_trace_forward_adjoint(name, path, gpu, lattice, monkeypatch):
    """Segments, float64 / float32 forward and the adjoint of every lattice ray against the IEEE
    oracle, and of the unmasked rays against the reference, per construction path."""
    case, ora_seg, ora_fwd, ora_adj = lattice(name)
    keep = ~case['sqrt_sensitive']
    op = _construct(case, path, gpu, monkeypatch)
    got = tuple(t.cpu().numpy() for t in op.segments())
    scale = gc.scale_of(case)
    msg = gc.compare_segments(ora_seg, got, scale, f'{name} {path} vs IEEE oracle')
    assert msg is None, msg
    ref = (case['seg_ptr'], case['seg_vox'], case['seg_len'])
    msg = gc.compare_segments(gc.take_rays(*ref, keep), gc.take_rays(*got, keep), scale,
                              f'{name} {path} vs reference (unmasked rays)')
    assert msg is None, msg
    assert not np.isnan(got[2]).any() and (got[2] > 0).all()
    x = tr.from_numpy(case['density0']).to(gpu)
    f64 = op(x).cpu().numpy().reshape(-1)
    err = gc.rel_close(f64, ora_fwd, gc.F64_RTOL)
    assert err <= gc.F64_RTOL, f'{name} {path}: f64 forward vs oracle {err:.3g}'
    err = gc.rel_close(f64[keep], case['fwd64_0'].reshape(-1)[keep], gc.F64_RTOL)
    assert err <= gc.F64_RTOL, f'{name} {path}: f64 forward vs reference {err:.3g}'
    f32 = op(x.float())
    assert f32.dtype == tr.float32
    f32 = f32.cpu().numpy().reshape(-1)
    err = gc.rel_close(f32, ora_fwd, gc.F32_RTOL)
    assert err <= gc.F32_RTOL, f'{name} {path}: f32 forward vs oracle {err:.3g}'
    err = gc.rel_close(f32[keep], case['fwd32_0'].reshape(-1)[keep], gc.F32_RTOL)
    assert err <= gc.F32_RTOL, f'{name} {path}: f32 forward vs reference {err:.3g}'
    adj = op.T(tr.from_numpy(case['y0']).to(gpu)).cpu().numpy().reshape(-1)
    for want, what in ((ora_adj, 'oracle'), (case['adj64_0'].reshape(-1), 'reference')):
        err = float(np.abs(adj - want).max()) / max(float(np.abs(want).max()), 1e-300)
        assert err <= 1e-10, f'{name} {path}: adjoint vs {what} {err:.3g}'


@pytest.mark.parametrize('name', gc.LATTICE_CASES)
def test_lattice_fused_and_atomic(name, gpu, lattice, monkeypatch):
    """line_integrals (the fused trace + integrate kernel) against the oracle's forward, and the
    float64-atomic adjoint against the oracle's adjoint."""
    from sph_raytracer_amd import Operator
    from sph_raytracer_amd.raytracer import line_integrals
    case, _, ora_fwd, ora_adj = lattice(name)
    grid, geom = gc.make_grid(case), _geom(case)
    x = tr.from_numpy(case['density0']).to(gpu)
    fused = _count_calls(monkeypatch, ('sphrt_trace_integrate_f64', 'sphrt_trace_integrate_f32'))
    got = line_integrals(grid, geom, x).cpu().numpy().reshape(-1)
    err = gc.rel_close(got, ora_fwd, gc.F64_RTOL)
    assert err <= gc.F64_RTOL, f'{name}: fused f64 forward vs oracle {err:.3g}'
    got = line_integrals(grid, geom, x.float()).cpu().numpy().reshape(-1)
    err = gc.rel_close(got, ora_fwd, gc.F32_RTOL)
    assert err <= gc.F32_RTOL, f'{name}: fused f32 forward vs oracle {err:.3g}'
    assert fused == dict(sphrt_trace_integrate_f64=1, sphrt_trace_integrate_f32=1)
    op = Operator(grid, geom, device=gpu)
    atomic = _count_calls(monkeypatch, ('sphrt_adjoint_accumulate',))
    op.adjoint_mode = 'atomic'
    adj = op.T(tr.from_numpy(case['y0']).to(gpu)).cpu().numpy().reshape(-1)
    assert atomic == dict(sphrt_adjoint_accumulate=1), 'the atomic adjoint did not run'
    err = float(np.abs(adj - ora_adj).max()) / max(float(np.abs(ora_adj).max()), 1e-300)
    assert err <= 1e-10, f'{name}: atomic adjoint vs oracle {err:.3g}'


@pytest.mark.parametrize('name', gc.LATTICE_CASES)
def test_lattice_ties_exercised(name, gpu, lattice):
    """The lattice reaches the tie code: some rays are deferred to the exact path (ambiguous tie
    groups), and fewer than the rays with a segment (the rest, equal-valued ties among them, stay
    on the wave path)."""
    case, ora_seg, _, _ = lattice(name)
    deferred = exact_stats(gc.make_grid(case), _geom(case), gpu)[0]
    hit = int((np.diff(ora_seg[0]) > 0).sum())
    print(f'{name}: deferred {deferred} / hit {hit} rays')
    assert 0 < deferred < hit, (deferred, hit)


@pytest.mark.parametrize('name', gc.LATTICE_CASES)
def test_lattice_bounds_hold(name, gpu, lattice, monkeypatch):
    """segment_bound is a true upper bound of every lattice ray's segment count (a failing bound
    would silently fall back to the two-pass fill)."""
    from sph_raytracer_amd import Operator, raytracer as rt
    case, _, _, _ = lattice(name)
    seen = []
    monkeypatch.setenv('SPHRT_CONSTRUCT', 'python')
    monkeypatch.setenv('SPHRT_TRACE', 'onepass')
    monkeypatch.setattr(rt, '_bound_hook', lambda b: seen.append(b.clone()))
    op = Operator(gc.make_grid(case), _geom(case), device=gpu)
    assert len(seen) == 1 and op._csr['ray_id'] is None       # (rows in geometry order)
    bounds = seen[0].cpu().numpy().astype(np.int64)
    counts = np.diff(op.segments()[0].cpu().numpy())
    assert bounds.shape == counts.shape == (len(case['xs']),)
    low = np.flatnonzero(bounds < counts)
    assert len(low) == 0, (f'{name}: {len(low)} rays over their bound; first ray {low[0]}: start '
                           f'{case["xs"][low[0]].tolist()} direction {case["rays"][low[0]].tolist()}'
                           f' bound {bounds[low[0]]} count {counts[low[0]]}')
    assert counts.max() > 0 and bounds.max() <= int(op._plan.K)


def _split_nonfinite(ptr, vox, seg):
    """(finite CSR, (ray, voxel, kind) of the non-finite segments: +1 inf, -1 -inf, 0 NaN)."""
    n = len(ptr) - 1
    ray = np.repeat(np.arange(n), np.diff(ptr))
    fin = np.isfinite(seg)
    fptr = np.concatenate([[0], np.cumsum(np.bincount(ray[fin], minlength=n))])
    kind = np.where(np.isnan(seg[~fin]), 0, np.sign(seg[~fin]))
    return (fptr, vox[fin], seg[fin]), (ray[~fin], vox[~fin], kind)


@pytest.mark.parametrize('name', gc.LATTICE_F32_CASES + gc.LATTICE_INVALID_CASES)
def test_lattice_reference_modes_vs_oracle(name, gpu):
    """The lattice under ftype=float32 (bit for bit the oracle's float32 trace) and invalid=True
    (test_random_grid_reference_modes_vs_oracle's rules: the non-finite segments exactly, the
    finite ones under the contract)."""
    from sph_raytracer_amd import Operator
    ora = _oracle()
    case = gc.load(name)
    f32 = name in gc.LATTICE_F32_CASES
    kw = dict(ftype=tr.float32) if f32 else dict(invalid=True)
    op = Operator(gc.make_grid(case), _geom(case), device=gpu, **kw)
    ptr, vox, seg = (t.cpu().numpy() for t in op.segments())
    g = ora.Grid.from_boundaries(case['r_b'], case['e_b'], case['a_b'],
                                 ftype='float32' if f32 else 'float64')
    optr, ovox, oseg = ora.trace_segments(g, case['xs'], case['rays'],
                                          gc.ref_mode_starts(case, f32), invalid=not f32)
    if f32:
        assert np.array_equal(ptr, optr), f'{name}: segment counts differ'
        assert np.array_equal(vox, ovox), f'{name}: voxels differ'
        assert np.array_equal(seg, oseg), f'{name}: lengths differ'
        assert len(ovox) > 1000
        return
    got_f, got_n = _split_nonfinite(ptr, vox, seg)
    ref_f, ref_n = _split_nonfinite(optr, ovox, oseg)
    for a, b, what in zip(got_n, ref_n, ('rays', 'voxels', 'kinds')):
        assert np.array_equal(a, b), f'{name}: non-finite segments differ ({what})'
    assert len(ref_n[0]) >= len(case['xs']), 'every list ends in an infinite segment'
    msg = gc.compare_segments(ref_f, got_f, gc.scale_of(case), name)
    assert msg is None, msg


def test_lattice_solvers(gpu):
    """r_torch / e_torch / a_torch of this package (sphrt_solve) on the lattice rays: NaN / inf at
    the reference's positions, and test_gpu_golden.test_solvers_bitlevel's comparison with the
    reference (no distance off by more than 1e-9, 99.9 % within 4 ulp, regions and signs exact
    where finite) — except its share of bit-exact distances, which measures the reference's MKL
    square root and not this code: the lattice has 207 distinct sphere distances, and the C oracle
    with IEEE square roots itself equals the fixture on 0.9152 of the r entries (0.9957 e, 1.0 a;
    all within one ulp, 4.4e-16), under the 0.95 random rays give.  Instead every entry must be
    the IEEE oracle's bit for bit, which is the stronger statement about this code."""
    from sph_raytracer_amd.raytracer import a_torch, e_torch, r_torch
    z = gc.load(gc.LATTICE_SOLVERS)
    xs, rays = tr.from_numpy(z['xs']), tr.from_numpy(z['rays'])
    ora = _oracle()
    g = ora.Grid.from_boundaries(z['r_b'], z['e_b'], z['a_b'])
    for fam, (key, fn) in enumerate((('r', r_torch), ('e', e_torch), ('a', a_torch))):
        t, reg, _, neg = fn(tr.from_numpy(z[f'{key}_b']), xs.clone(), rays.clone())
        t, reg, neg = t.numpy(), reg.numpy(), neg.numpy()
        rt = z[f'{key}_t']
        for what, f in (('+inf', np.isposinf), ('-inf', np.isneginf), ('NaN', np.isnan)):
            assert np.array_equal(f(t), f(rt)), f'{key}: {what} pattern differs'
        fin = np.isfinite(rt)
        d = np.abs(t[fin] - rt[fin])
        tol = 4 * np.spacing(np.abs(rt[fin])) + 1e-13
        frac_exact, frac_ulp = float(np.mean(d == 0)), float(np.mean(d <= tol))
        print(f'{key}: {frac_exact:.4f} of distances bit-exact, {frac_ulp:.4f} within 4 ulp, '
              f'max {d.max():.3g}')
        assert d.max() <= 1e-9, f'{key}: distance error {d.max():.3g}'
        assert frac_ulp >= 0.999, f'{key}: only {frac_ulp:.4f} of distances within 4 ulp'
        assert np.array_equal(reg[fin], z[f'{key}_reg'][fin]), f'{key}: regions differ'
        assert np.array_equal(neg[fin], z[f'{key}_neg'][fin]), f'{key}: negative_crossing differs'
        ot, oreg, oneg = ora.solve(g, fam, z['xs'], z['rays'])
        same = (t == ot) | (np.isnan(t) & np.isnan(ot))
        assert same.all(), f'{key}: {int((~same).sum())} distances differ from the IEEE oracle'
        assert np.array_equal(reg, oreg), f'{key}: regions differ from the IEEE oracle'
        assert np.array_equal(neg, oneg), f'{key}: negative_crossing differs from the IEEE oracle'


# ---- named regression rays (found by the lattice) ----------------------------------------------

def _single_ray(case_name, start, direction, gpu, monkeypatch, hook=None):
    """One ray (as a ViewGeom normalises it) on a lattice fixture's grid through the Python
    one-pass construction -> (operator, the IEEE oracle's segments)."""
    from sph_raytracer_amd import Operator, ViewGeom, raytracer as rt
    case = gc.load(case_name)
    grid = gc.make_grid(case)
    geom = ViewGeom(tr.tensor([start], dtype=tr.float64), tr.tensor([direction], dtype=tr.float64))
    xs, d = geom.ray_starts.numpy().copy(), geom.rays.numpy().copy()
    monkeypatch.setenv('SPHRT_CONSTRUCT', 'python')
    monkeypatch.setenv('SPHRT_TRACE', 'onepass')
    if hook is not None:
        monkeypatch.setattr(rt, '_bound_hook', hook)
    op = Operator(grid, geom, device=gpu)
    ora = _oracle()
    g = ora.Grid.from_boundaries(case['r_b'], case['e_b'], case['a_b'])
    ref = ora.trace_segments(g, xs, d, rt.find_starts(grid, tr.from_numpy(xs)).numpy())
    return op, ref


def test_start_on_outer_shell_exit_behind_start(gpu, monkeypatch):
    """Start (-1, -1, -1/2), |x| = 1.5 exactly on the outer shell of the hollow grid, along -z:
    the shell's far crossing rounds to -4.4e-16, behind the start, so the reference never lists
    the exit, keeps the start's shell and walks on through the cones ahead (3.27 in voxel 121,
    1.63 in voxel 129: longer than the grid is wide).  The wave path used to cut the list at that
    exit and gave 2.95 in voxel 121 only, while the exact path gave the reference's answer."""
    op, ref = _single_ray('lattice_hollow', [-1, -1, -0.5], [0, 0, -1], gpu, monkeypatch)
    got = tuple(t.cpu().numpy() for t in op.segments())
    msg = gc.compare_segments(ref, got, 2.0, 'start on the outer shell')
    assert msg is None, msg
    _, vox, seg = gc.canonical(*got, 2e-12)
    assert vox.tolist() == [121, 129]
    assert np.allclose(seg, [3.265986323711, 1.632993161855], rtol=1e-11, atol=0)


def test_line_through_origin_invalid_start_azimuth_bound(gpu, monkeypatch):
    """Start (-1/2, -1/2, -1/2) along (1, 1, 1) on the a in [0, 2 pi] grid of 100 azimuth bins:
    the start's azimuth (-3 pi / 4) lies outside the range, so it is in no voxel though its shell
    is valid, and the line's d^2 rounds below zero, so the outer sphere's chord is NaN.  The ray
    still yields segments, and segment_bound, which took the NaN for a miss, gave 2."""
    seen = []
    op, ref = _single_ray('lattice_wide_a', [-0.5, -0.5, -0.5], [1, 1, 1], gpu, monkeypatch,
                          hook=lambda b: seen.append(b.clone()))
    got = tuple(t.cpu().numpy() for t in op.segments())
    msg = gc.compare_segments(ref, got, 1.0, 'line through the origin')
    assert msg is None, msg
    count = int(np.diff(got[0])[0])
    assert len(seen) == 1 and count > 2
    assert int(seen[0][0]) >= count, (int(seen[0][0]), count)
