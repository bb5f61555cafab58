"""retrieval.chambolle_pock(precondition='diagonal') on the GPU: cp_cases' configurations (each
fidelity kind, with and without TV, with a tensor mask, on the 72-ray and the 257-ray problem)
through the direct path over the stored Operator and over a MatrixFreeOperator (float64 atomics,
and the deterministic fixed-point trace).  The reference is the generic path on the CPU over the
oracle's matrix for the same number of iterations (dp_cases.ITERATIONS); x, p and q are held to
the bound test_gpu_cp.py holds the scalar iteration to for the same comparison (cp_cases.bounds:
16 x the CPU reference's sensitivity to summation order, at least 1e-13 of the largest
magnitude), the duality gap recomputed from the dense matrix to cp_cases.GAP_LIMIT, the bounds
and dual intervals exactly, the steps in info to their shapes and to the reference's, and the
launches are counted: one sphrt_dp_steps_f64 per solve, sphrt_dp_primal_f64 and
sphrt_dp_ray_dual_f64 once per iteration, never the scalar entries they stand in for."""
import functools
import math

import numpy as np
import pytest
import torch as tr

import cp_cases as cp
import dp_cases as dc
import pd_cases as pc
from test_gpu_fista import _bits, _operator

pytestmark = pytest.mark.gpu
F64 = tr.float64
OPERATORS = ['stored', 'matrix_free', 'matrix_free_deterministic']
CONFIGS = cp.gpu_cases()
IDS = ['-'.join([c[0], c[1], 'tv' if c[2] else 'notv', 'masked' if c[3] else 'unit']) for c in CONFIGS]
K = dc.ITERATIONS


@functools.lru_cache(maxsize=None)
def _reference(cfg):
    """The CPU reference of a configuration: built once, never written."""
    return dc.solve_case(cp.gpu_case(cfg))


def _solve(cfg, kind, gpu, **kw):
    from sph_raytracer_amd.retrieval import chambolle_pock
    name, fid, tv, masked = cfg
    _, y, mask, _ = cp.problem(name)
    kw.setdefault('num_iterations', K)
    return chambolle_pock(_operator(name, kind, gpu), y.to(gpu),
                          cp.terms(fid, tv, mask.to(gpu) if masked else 1), damp=cp.DAMP,
                          lower=cp.LOWER, upper=cp.UPPER, precondition='diagonal', **kw)


def _spy(monkeypatch):
    """Counts of the two paths' runs and of the entries' calls (sphrt_pd.h, sphrt_cp.h,
    sphrt_dp.h)."""
    from sph_raytracer_amd import _lib, retrieval
    seen = {'direct': 0, 'generic': 0}
    for key in ('direct', 'generic'):
        fn = getattr(retrieval, f'_chambolle_pock_{key}')

        def wrapped(*a, _fn=fn, _key=key, **k):
            seen[_key] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(retrieval, f'_chambolle_pock_{key}', wrapped)
    lib = _lib.load()
    for name in _lib.PD_EXPORTED + _lib.CP_EXPORTED + _lib.DP_EXPORTED:
        fn = getattr(lib, name)
        seen[name] = 0

        def counted(*a, _fn=fn, _name=name):
            seen[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counted)
    return seen


def _route(tv, runs=1):
    return {'direct': runs, 'generic': 0, 'sphrt_pd_primal_f64': 0, 'sphrt_cp_ray_dual_f64': 0,
            'sphrt_pd_dual_f64': runs * K if tv else 0, 'sphrt_dp_primal_f64': runs * K,
            'sphrt_dp_ray_dual_f64': runs * K, 'sphrt_dp_steps_f64': runs}


def _check(cfg, x, y_hat, info):
    name, fid, tv, masked = cfg
    op, y, mask, _ = cp.problem(name)
    xr, _, ir = _reference(cfg)
    assert x.shape == tuple(op.grid.shape) and x.dtype == F64 and x.device.type == 'cuda'
    assert y_hat.shape == y.shape
    # the bounds and the dual intervals, exactly
    xn = x.cpu().numpy().reshape(-1)
    assert np.all((xn >= cp.LOWER) & (xn <= cp.UPPER))
    lo_bits, hi_bits = (np.float64(v).view(np.int64) for v in (cp.LOWER, cp.UPPER))
    assert np.all(xn.view(np.int64)[xn == cp.LOWER] == lo_bits)
    assert np.all(xn.view(np.int64)[xn == cp.UPPER] == hi_bits)
    s, _ = cp.ray_factors(y, mask, masked)
    p = info['ray_dual']
    assert p.shape == y.shape and p.dtype == F64
    pn = p.cpu().numpy().reshape(-1)
    zero = s == 0
    assert not pn[zero].any() and not np.signbit(pn[zero]).any()
    if fid == 'abs':
        assert np.all(np.abs(pn) <= s)
    elif fid == 'huber':
        assert np.all(np.abs(pn) <= s * cp.HUBER_DELTA)
    elif fid == 'poisson':
        assert np.all(pn <= s)
    # the documented shapes of the steps, and their values against the reference's
    assert info['norm'] is None and info['sigma_tv'] == cp.LAM_F / y.numel() / 2
    assert info['sigma_tv'] == ir['sigma_tv'] and isinstance(info['sigma_tv'], float)
    tau, sigma = info['tau'], info['sigma']
    assert tau.shape == x.shape and tau.dtype == F64 and tau.device == x.device
    assert sigma.shape == y.shape and sigma.dtype == F64 and sigma.device == x.device
    assert tr.allclose(tau.cpu(), ir['tau'], rtol=1e-12, atol=0)
    assert tr.allclose(sigma.cpu(), ir['sigma'], rtol=1e-12, atol=0)
    assert tr.equal(sigma.cpu() == 0, ir['sigma'] == 0)      # (geometry order: rays that miss)
    # x, p, q against the CPU reference within test_gpu_cp.py's bound
    d_x, d_p, d_q = cp.bounds(cfg, xr, ir['ray_dual'], ir['dual'])
    err_x = float((x.cpu() - xr).abs().max())
    err_p = float((p.cpu() - ir['ray_dual']).abs().max())
    print(f'  x {err_x:.3g} / {d_x:.3g}, p {err_p:.3g} / {d_p:.3g}', end='')
    if tv:
        q = info['dual']
        assert q.shape == (3,) + tuple(x.shape)
        qn = q.cpu().numpy().reshape(3, -1)
        cax = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS) / xn.size
        assert all(np.abs(qn[ax]).max() <= cax[ax] for ax in range(3))
        err_q = float((q.cpu() - ir['dual']).abs().max())
        print(f', q {err_q:.3g} / {d_q:.3g}', end='')
    else:
        assert info['dual'] is None and info['dual_change'] == [0.0] * K
    # the duality gap from info['ray_dual'] and info['dual'], recomputed from the dense matrix
    J, D, gap = cp.gap_of(cp.gpu_case(cfg), x, info)
    print(f', gap {gap:.3g} / {cp.GAP_LIMIT[fid]:.3g}')
    assert err_x <= d_x and err_p <= d_p
    assert not tv or err_q <= d_q
    assert D <= J + cp.WEAK_DUALITY_SLACK * abs(J) and gap <= cp.GAP_LIMIT[fid]
    for key in ('primal_change', 'ray_dual_change', 'fidelity', 'dual_change'):
        assert len(info[key]) == K and all(math.isfinite(v) for v in info[key])
    assert np.allclose(info['fidelity'], ir['fidelity'], rtol=1e-6)


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_direct_path_matches_the_cpu_reference(cfg, kind, gpu, monkeypatch):
    seen = _spy(monkeypatch)
    x, y_hat, info = _solve(cfg, kind, gpu)
    assert seen == _route(cfg[2])
    print(f'chambolle_pock diagonal {cfg} {kind}:', end='')
    _check(cfg, x, y_hat, info)
    assert tr.equal(y_hat, _operator(cfg[0], kind, gpu)(x))


@pytest.mark.parametrize('kind', ['stored', 'matrix_free_deterministic'])
@pytest.mark.parametrize('fid', cp.KINDS)
def test_two_runs_are_bitwise_equal(fid, kind, gpu):
    cfg = ('two_workgroups', fid, True, True)
    (xa, ya, ia), (xb, yb, ib) = (_solve(cfg, kind, gpu) for _ in range(2))
    assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(ya), _bits(yb))
    for key in ('dual', 'ray_dual', 'tau', 'sigma'):
        assert np.array_equal(_bits(ia.pop(key)), _bits(ib.pop(key)))
    assert ia == ib


def test_float32_measurements_and_the_keyword_s_neighbours(gpu, monkeypatch):
    """A float32 y takes the direct path; power_iterations is ignored (no power method runs); a
    given norm is refused; precondition=None on the same inputs launches the scalar entries."""
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.retrieval import chambolle_pock
    cfg = ('tiny', 'huber', True, True)
    _, y, mask, _ = cp.problem('tiny')
    op, fns = _operator('tiny', 'stored', gpu), cp.terms('huber', True, mask.to(gpu))
    kw = dict(damp=cp.DAMP, lower=cp.LOWER, upper=cp.UPPER, num_iterations=K)
    want = _solve(cfg, 'stored', gpu)
    seen = _spy(monkeypatch)
    monkeypatch.setattr(retrieval, '_fista_step', None)          # (any use of it would raise)
    x32, _, i32 = chambolle_pock(op, y.to(gpu).float(), fns, precondition='diagonal',
                                 power_iterations=1, **kw)
    assert seen == _route(True)
    # (y rounded to float32: 6e-8 relative on the measurements, test_cp_cpu's float32 bound)
    assert float((x32 - want[0]).abs().max()) <= 1e-4
    assert np.array_equal(_bits(i32['tau']), _bits(want[2]['tau']))
    with pytest.raises(ValueError, match='norm'):
        chambolle_pock(op, y.to(gpu), fns, precondition='diagonal', norm=5.0, **kw)
    monkeypatch.undo()
    seen = _spy(monkeypatch)
    _, _, info = chambolle_pock(op, y.to(gpu), fns, precondition=None, **kw)
    assert seen['sphrt_pd_primal_f64'] == seen['sphrt_cp_ray_dual_f64'] == K
    assert seen['sphrt_dp_primal_f64'] == seen['sphrt_dp_ray_dual_f64'] == 0
    assert seen['sphrt_dp_steps_f64'] == 0 and isinstance(info['tau'], float)
    assert 'sigma_tv' not in info and info['norm'] > 0


def test_short_runs(gpu):
    """num_iterations = 0, 1, 2: the histories' lengths, the start clamped into the bounds, the
    steps present, and x0 unchanged."""
    from sph_raytracer_amd.retrieval import chambolle_pock
    _, y, _, _ = cp.problem('tiny')
    y, op = y.to(gpu), _operator('tiny', 'stored', gpu)
    x0 = tr.linspace(-1, 2, 72, dtype=F64).reshape(4, 3, 6).to(gpu)
    for k in (0, 1, 2):
        x, _, info = chambolle_pock(op, y, cp.terms('abs', True), x0=x0, num_iterations=k,
                                    lower=cp.LOWER, upper=cp.UPPER, precondition='diagonal')
        assert len(info['primal_change']) == len(info['fidelity']) == k
        assert bool(((x >= cp.LOWER) & (x <= cp.UPPER)).all())
        assert bool((x == cp.LOWER).any()) and bool((x == cp.UPPER).any())
        assert info['tau'].shape == x.shape and bool((info['tau'] > 0).all())
    assert tr.equal(x0, tr.linspace(-1, 2, 72, dtype=F64).reshape(4, 3, 6).to(gpu))
