"""The wave trace's sort and fill ladder on irregular wide grids, against the C oracle.

Every case of tests/trace_cases.py — irregular hollow / partial grids with up to 301 shells, 157
cones and 361 half-planes, near-duplicate boundaries, lattice tie rays; tests/
test_trace_cases_cpu.py shows on the oracle alone which rung, fill, chunk skip, wedge wrap,
near-tie and late tie each holds — runs through the trace in every mode and is held to the
oracle's reference for the case (IEEE square roots, the GPU's arithmetic), computed once per case
(trace_cases.reference):

  - Operator.segments() under golden_cases.compare_segments with test_gpu_fuzz.py's scale and
    tolerance (voxel sequences exact after dropping segments under 1e-12 x the scale, lengths
    1e-12 relative + 1e-12 x the scale), the float64 / float32 forward (1e-10 / 1e-5 relative) and
    op.T (1e-10 x max);
  - the one-pass CSR bit for bit the two-pass one, and (more than 64 half-planes) the one without
    the wedge;
  - segment_bound (the binary-search branch: no grid here is evenly spaced; the window loop on
    partial azimuth ranges) at least the count and at most K for every ray, with no fill pass;
  - the modes that compact into LDS (kFillLds): line_integrals float64 / float32, back_project in
    both modes, MatrixFreeOperator.residual_gradient in both modes, at the tolerances of
    test_gpu_matrix_free*.py (float64 1e-10, float32 1e-5, x max|reference|), and the
    deterministic back-projection twice with equal bits;
  - tie cases: some rays deferred to the exact path, fewer than the hit rays;
  - K = 512 and K = 514: ftype=float32 bit for bit the oracle's float32 trace and invalid=True by
    the rules of test_gpu_fuzz.test_random_grid_reference_modes_vs_oracle, across kNetworkMaxK.

No ray is masked from any comparison (masked rays per case: 0 in all fourteen).

Mutations of csrc/trace.hip, each built and run once against this file:
  - the spheres' chunk-skip ballot ignoring its last chunk: test_segments_forward_adjoint and
    test_lds_fill_modes fail on all eight cases with more than 64 shells;
  - merge_path taking `a <= b` for `a < b`: nothing fails, and nothing can: composite keys carry
    the candidate index in their low bits, so two real keys are never equal and the padding is
    guarded by `ai < S`; the two comparisons choose alike on every list;
  - count_in's second binary search taking `<` for `<=`: nothing fails.  The two differ only
    when a boundary equals the window's end (an angle plus its 1e-6 / 1e-4 margin) bit for bit,
    and the bound adds 2 / 4 on top; no ray here meets that.
"""
import numpy as np
import pytest
import torch as tr

import golden_cases as gc
import trace_cases as tc
from gpu_helpers import exact_stats
from test_gpu_fuzz import _split_nonfinite

pytestmark = pytest.mark.gpu

TOL = {tr.float64: 1e-10, tr.float32: 1e-5}
WIDE_A = [n for n in tc.NAMES if len(tc.build(n)[2]) > 64]
TIE = [c.name for c in tc.CASES if c.tie]
K_EDGE = ['k512_150x60x86', 'k514_150x60x88']
_ENV = ('SPHRT_CONSTRUCT', 'SPHRT_TRACE', 'SPHRT_TRACE_WEDGE')


@pytest.fixture(scope='module')
def ops():
    """name -> (grid, geom, Operator by the default construction): built once, read-only."""
    cache = {}

    def get(name, gpu):
        if name not in cache:
            from sph_raytracer_amd import Operator
            grid, geom = tc.make(name)
            cache[name] = (grid, geom, Operator(grid, geom, device=gpu))
        return cache[name]

    return get


def _csr(op):
    c = op._csr
    assert c['ray_id'] is None
    return tuple(c[k][:c['total'] if k != 'row_ptr' else None] for k in ('row_ptr', 'vox', 'len'))


def _close_max(got, want, tol, what):
    """Within tol x max|reference| (test_gpu_adjoint_paths._assert_close)."""
    got = got.detach().cpu().double().numpy().reshape(-1)
    want = np.asarray(want).reshape(-1)
    assert got.shape == want.shape
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert scale > 0 and err <= tol * scale, f'{what}: {err:.3g} against max {scale:.3g}'


@pytest.mark.parametrize('name', tc.NAMES)
def test_segments_forward_adjoint(name, gpu, ops, monkeypatch):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    grid, geom, op = ops(name, gpu)
    ref = tc.reference(name)
    got = tuple(t.cpu().numpy() for t in op.segments())
    msg = gc.compare_segments(ref.segs, got, tc.SCALE, name)
    assert msg is None, msg
    x = tr.from_numpy(ref.x.copy()).to(gpu)
    have = op(x).cpu().numpy().reshape(-1)
    err = gc.rel_close(have, ref.y, gc.F64_RTOL)
    assert err <= gc.F64_RTOL, f'{name}: f64 forward {err:.3g}'
    have32 = op(x.float()).cpu().numpy().reshape(-1)
    err = gc.rel_close(have32, ref.y, gc.F32_RTOL)
    assert err <= gc.F32_RTOL, f'{name}: f32 forward {err:.3g}'
    have_t = op.T(tr.from_numpy(ref.yt.copy()).to(gpu)).cpu().numpy()
    scale = max(float(np.abs(ref.xt).max()), 1e-300)
    assert float(np.abs(have_t - ref.xt).max()) <= 1e-10 * scale, f'{name}: adjoint'


@pytest.mark.parametrize('name', tc.NAMES)
def test_onepass_twopass_wedge_bitwise(name, gpu, monkeypatch):
    """The one-pass CSR (bound + emit: fill_regs stores straight into the emit slot) equals the
    two-pass one (count + fill) bit for bit, and the CSR without the half-plane wedge."""
    from sph_raytracer_amd import Operator
    grid, geom = tc.make(name)
    monkeypatch.delenv('SPHRT_TRACE_WEDGE', raising=False)
    monkeypatch.setenv('SPHRT_CONSTRUCT', 'python')
    monkeypatch.setenv('SPHRT_TRACE', 'onepass')
    one = _csr(Operator(grid, geom, device=gpu))
    monkeypatch.setenv('SPHRT_TRACE', 'twopass')
    two = _csr(Operator(grid, geom, device=gpu))
    for a, b, k in zip(one, two, ('row_ptr', 'vox', 'len')):
        assert tr.equal(a, b), f'{name}: one-pass {k} differs from two-pass'
    if name in WIDE_A:
        monkeypatch.setenv('SPHRT_TRACE', 'onepass')
        monkeypatch.setenv('SPHRT_TRACE_WEDGE', '0')
        flat = _csr(Operator(grid, geom, device=gpu))
        for a, b, k in zip(one, flat, ('row_ptr', 'vox', 'len')):
            assert tr.equal(a, b), f'{name}: {k} differs without the wedge'


@pytest.mark.parametrize('name', tc.NAMES)
def test_bounds_hold(name, gpu, monkeypatch):
    """segment_bound is an upper bound of every ray's segment count, at most K, and no fill pass
    ran (a failing bound would silently fall back to the two-pass trace)."""
    from sph_raytracer_amd import Operator, raytracer as rt
    grid, geom = tc.make(name)
    seen, fills = [], []
    monkeypatch.delenv('SPHRT_TRACE_WEDGE', raising=False)
    monkeypatch.setenv('SPHRT_CONSTRUCT', 'python')
    monkeypatch.setenv('SPHRT_TRACE', 'onepass')
    monkeypatch.setattr(rt, '_bound_hook', lambda b: seen.append(b.clone()))
    lib = rt._lib.load()
    orig = lib.sphrt_trace_fill
    monkeypatch.setattr(lib, 'sphrt_trace_fill', lambda *a: fills.append(1) or orig(*a))
    op = Operator(grid, geom, device=gpu)
    assert len(seen) == 1 and op._csr['ray_id'] is None
    assert not fills, f'{name}: a segment bound failed, the trace fell back to the fill pass'
    bounds = seen[0].cpu().numpy().astype(np.int64)
    counts = np.diff(op.segments()[0].cpu().numpy())
    xs, d = tc.build(name)[3:]
    assert bounds.shape == counts.shape == (len(xs),)
    low = np.flatnonzero(bounds < counts)
    assert len(low) == 0, (f'{name}: {len(low)} rays over their bound; first ray {low[0]}: start '
                           f'{xs[low[0]].tolist()} direction {d[low[0]].tolist()} bound '
                           f'{bounds[low[0]]} count {counts[low[0]]}')
    K = tc.K_of(name)
    assert int(op._plan.K) == K and bounds.max() <= K and counts.max() > 0
    c = tc.list_classes(name)
    assert (bounds[c.hit & ~c.inside] < K).any(), 'the geometric bound is never below K'


@pytest.mark.parametrize('name', tc.NAMES)
def test_lds_fill_modes(name, gpu, monkeypatch):
    """INTEGRATE, SCATTER, NORMAL and the fixed-point modes (the segments compacted into LDS)."""
    from oracle import oracle as ora
    from sph_raytracer_amd import MatrixFreeOperator, back_project
    from sph_raytracer_amd.raytracer import line_integrals
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    grid, geom = tc.make(name)
    ref = tc.reference(name)
    x = tr.from_numpy(ref.x.copy()).to(gpu)
    y = tr.from_numpy(ref.yt.copy()).to(gpu)
    _close_max(line_integrals(grid, geom, x), ref.y, TOL[tr.float64], f'{name} line_integrals f64')
    _close_max(line_integrals(grid, geom, x.float()), ref.y, TOL[tr.float32],
               f'{name} line_integrals f32')
    _close_max(back_project(grid, geom, y), ref.xt, TOL[tr.float64], f'{name} back_project')
    det = back_project(grid, geom, y, deterministic=True)
    _close_max(det, ref.xt, TOL[tr.float64], f'{name} back_project deterministic')
    assert tr.equal(det, back_project(grid, geom, y, deterministic=True)), \
        f'{name}: two deterministic back-projections differ'
    scale = 0.37
    want = np.asarray(ora.adjoint(*ref.segs, scale * (ref.y - ref.yt), ref.n_vox))
    for deterministic in (False, True):
        op = MatrixFreeOperator(grid, geom, device=gpu, deterministic=deterministic)
        yhat, grad = op.residual_gradient(x, y, scale)
        _close_max(yhat, ref.y, TOL[tr.float64], f'{name} residual_gradient forward')
        _close_max(grad, want, TOL[tr.float64],
                   f'{name} residual_gradient gradient (deterministic={deterministic})')


@pytest.mark.parametrize('name', TIE)
def test_tie_rays_reach_the_exact_path(name, gpu, monkeypatch):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    grid, geom = tc.make(name)
    deferred = exact_stats(grid, geom, gpu)[0]
    hit = int((np.diff(tc.reference(name).segs[0]) > 0).sum())
    print(f'{name}: deferred {deferred} / hit {hit} rays')
    assert 0 < deferred < hit, (deferred, hit)


@pytest.mark.parametrize('mode', ['float32', 'invalid'])
@pytest.mark.parametrize('name', K_EDGE)
def test_reference_modes_across_the_network_limit(name, mode, gpu, monkeypatch):
    """ftype=float32 and invalid=True (the reference-mode trace: network_sort up to kNetworkMaxK
    = 512 candidates, the LDS sorts beyond) on K = 512 and K = 514 with real rays."""
    from sph_raytracer_amd import Operator
    from sph_raytracer_amd.raytracer import find_starts
    from oracle import oracle as ora
    ora.use_mkl_sqrt(False)
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    f32 = mode == 'float32'
    r_b, e_b, a_b, xs, d = (a.copy() for a in tc.build(name))
    grid, geom = tc.make(name)
    kw = dict(ftype=tr.float32) if f32 else dict(invalid=True)
    op = Operator(grid, geom, device=gpu, **kw)
    ptr, vox, seg = (t.cpu().numpy() for t in op.segments())
    g = ora.Grid.from_boundaries(r_b, e_b, a_b, ftype='float32' if f32 else 'float64')
    assert g.K == tc.K_of(name)
    starts = find_starts(grid, tr.from_numpy(xs), ftype=tr.float32 if f32 else tr.float64).numpy()
    optr, ovox, oseg = ora.trace_segments(g, xs, d, starts, invalid=not f32)
    if f32:
        assert np.array_equal(ptr, optr), f'{name} {mode}: segment counts differ'
        assert np.array_equal(vox, ovox), f'{name} {mode}: voxels differ'
        assert np.array_equal(seg, oseg), f'{name} {mode}: lengths differ'
        assert len(ovox) > 1000
        return
    got_f, got_n = _split_nonfinite(ptr, vox, seg)
    ref_f, ref_n = _split_nonfinite(optr, ovox, oseg)
    for a, b, what in zip(got_n, ref_n, ('rays', 'voxels', 'kinds')):
        assert np.array_equal(a, b), f'{name} {mode}: non-finite segments differ ({what})'
    assert len(ref_n[0]) >= len(xs), 'every list ends in an infinite segment'
    msg = gc.compare_segments(ref_f, got_f, tc.SCALE, f'{name} {mode}')
    assert msg is None, msg
