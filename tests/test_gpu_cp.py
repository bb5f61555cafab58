"""retrieval.chambolle_pock on the GPU: each fidelity kind, with and without TV, with a tensor
mask, on the two small problems of cp_cases (72 rays over 72 voxels; 257 rays over 300 voxels:
two workgroups), through the direct path over the stored Operator and over a MatrixFreeOperator
(float64 atomics, and the deterministic fixed-point trace), and through the generic path on the
same tensors.  The reference is the generic path on the CPU over the oracle's matrix for the same
number of iterations; x, p and q are held to 16 x that reference's own sensitivity to summation
order (cp_cases.SENSITIVITY, measured on the CPU), the duality gap recomputed from the dense
matrix to cp_cases.GAP_LIMIT, and every iterate property exactly."""
import functools
import math

import numpy as np
import pytest
import torch as tr

import cp_cases as cp
import pd_cases as pc
from test_gpu_fista import _bits, _operator

pytestmark = pytest.mark.gpu
F64 = tr.float64
OPERATORS = ['stored', 'matrix_free', 'matrix_free_deterministic']
CONFIGS = cp.gpu_cases()
IDS = ['-'.join([c[0], c[1], 'tv' if c[2] else 'notv', 'masked' if c[3] else 'unit']) for c in CONFIGS]


@functools.lru_cache(maxsize=None)
def _reference(cfg, y32=False):
    """The CPU reference of a configuration (y32: of its measurements rounded to float32): built
    once, never written."""
    return cp.solve_case(cp.gpu_case(cfg), y32=y32)


def _solve(cfg, kind, gpu, y32=False, **kw):
    from sph_raytracer_amd.retrieval import chambolle_pock
    name, fid, tv, masked = cfg
    _, y, mask, _ = cp.problem(name)
    y = y.to(gpu)
    return chambolle_pock(_operator(name, kind, gpu), y.float() if y32 else y,
                          cp.terms(fid, tv, mask.to(gpu) if masked else 1), damp=cp.DAMP,
                          lower=cp.LOWER, upper=cp.UPPER, num_iterations=cp.ITERATIONS, **kw)


def _spy(monkeypatch):
    """Counts of the two paths' runs and of the three entries' calls."""
    from sph_raytracer_amd import _lib, retrieval
    seen = {'direct': 0, 'generic': 0}
    for key in ('direct', 'generic'):
        fn = getattr(retrieval, f'_chambolle_pock_{key}')

        def wrapped(*a, _fn=fn, _key=key, **k):
            seen[_key] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(retrieval, f'_chambolle_pock_{key}', wrapped)
    lib = _lib.load()
    for name in _lib.PD_EXPORTED + _lib.CP_EXPORTED:
        fn = getattr(lib, name)
        seen[name] = 0

        def counted(*a, _fn=fn, _name=name):
            seen[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counted)
    return seen


def _check(cfg, x, y_hat, info, gpu, y32=False):
    """The iterate properties exactly; x, p, q against the CPU reference; the gap."""
    name, fid, tv, masked = cfg
    op, y, mask, _ = cp.problem(name)
    xr, _, ir = _reference(cfg, y32)
    assert x.shape == tuple(op.grid.shape) and x.dtype == F64 and x.device.type == 'cuda'
    assert y_hat.shape == y.shape
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
        assert np.all(np.abs(pn) <= s) and (np.abs(pn) == s)[~zero].any()
    elif fid == 'huber':
        assert np.all(np.abs(pn) <= s * cp.HUBER_DELTA)
    elif fid == 'poisson':
        assert np.all(pn <= s)
    d_x, d_p, d_q = cp.bounds(cfg, xr, ir['ray_dual'], ir['dual'])
    err_x = float((x.cpu() - xr).abs().max())
    err_p = float((p.cpu() - ir['ray_dual']).abs().max())
    print(f'  x {err_x:.3g} / {d_x:.3g}, p {err_p:.3g} / {d_p:.3g}', end='')
    assert err_x <= d_x and err_p <= d_p
    if tv:
        q = info['dual']
        assert q.shape == (3,) + tuple(x.shape)
        qn = q.cpu().numpy().reshape(3, -1)
        cax = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS) / xn.size
        assert all(np.abs(qn[ax]).max() <= cax[ax] for ax in range(3))
        err_q = float((q.cpu() - ir['dual']).abs().max())
        print(f', q {err_q:.3g} / {d_q:.3g}', end='')
        assert err_q <= d_q
    else:
        assert info['dual'] is None and info['dual_change'] == [0.0] * cp.ITERATIONS
    J, D, gap = cp.gap_of(cp.gpu_case(cfg), x, info, y32)
    print(f', gap {gap:.3g}')
    assert D <= J + cp.WEAK_DUALITY_SLACK * abs(J) and gap <= cp.GAP_LIMIT[fid]
    for key in ('primal_change', 'ray_dual_change', 'fidelity', 'dual_change'):
        assert len(info[key]) == cp.ITERATIONS and all(math.isfinite(v) for v in info[key])
    assert np.allclose(info['fidelity'], ir['fidelity'], rtol=1e-6)
    for key in ('norm', 'tau', 'sigma'):
        assert math.isclose(info[key], ir[key], rel_tol=1e-9)


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_direct_path_matches_the_cpu_reference(cfg, kind, gpu, monkeypatch):
    seen = _spy(monkeypatch)
    x, y_hat, info = _solve(cfg, kind, gpu)
    K = cp.ITERATIONS
    assert seen == {'direct': 1, 'generic': 0, 'sphrt_pd_primal_f64': K,
                    'sphrt_pd_dual_f64': K if cfg[2] else 0, 'sphrt_cp_ray_dual_f64': K}
    print(f'chambolle_pock {cfg} {kind}:', end='')
    _check(cfg, x, y_hat, info, gpu)
    assert tr.equal(y_hat, _operator(cfg[0], kind, gpu)(x))


@pytest.mark.parametrize('kind', OPERATORS)
@pytest.mark.parametrize('fid', cp.KINDS)
def test_float32_measurements(fid, kind, gpu, monkeypatch):
    """A float32 y takes the direct path, promoted exactly in the launch: the reference is the
    CPU solve of the same values as float64, and everything `_check` holds the float64
    configurations to — iterate properties, x, p and q within the same bounds, the gap — holds
    here."""
    cfg = ('tiny', fid, True, True)
    seen = _spy(monkeypatch)
    x, y_hat, info = _solve(cfg, kind, gpu, y32=True)
    K = cp.ITERATIONS
    assert seen == {'direct': 1, 'generic': 0, 'sphrt_pd_primal_f64': K, 'sphrt_pd_dual_f64': K,
                    'sphrt_cp_ray_dual_f64': K}
    print(f'chambolle_pock {cfg} {kind} float32 y:', end='')
    _check(cfg, x, y_hat, info, gpu, y32=True)


@pytest.mark.parametrize('kind', ['stored', 'matrix_free_deterministic'])
@pytest.mark.parametrize('fid', cp.KINDS)
def test_two_runs_are_bitwise_equal(fid, kind, gpu):
    cfg = ('two_workgroups', fid, True, True)
    (xa, ya, ia), (xb, yb, ib) = (_solve(cfg, kind, gpu) for _ in range(2))
    assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(ya), _bits(yb))
    for key in ('dual', 'ray_dual'):
        assert np.array_equal(_bits(ia.pop(key)), _bits(ib.pop(key)))
    assert ia == ib


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_generic_path_on_the_gpu_agrees(cfg, gpu, monkeypatch):
    """The same inputs with `_cg_is_direct` false: the plain-torch path on the GPU, held to the
    same bound, and to the direct result within it."""
    from sph_raytracer_amd import retrieval
    xd, _, idir = _solve(cfg, 'stored', gpu)
    seen = _spy(monkeypatch)
    monkeypatch.setattr(retrieval, '_cg_is_direct', lambda *a: False)
    x, y_hat, info = _solve(cfg, 'stored', gpu)
    assert seen == {'direct': 0, 'generic': 1, 'sphrt_pd_primal_f64': 0, 'sphrt_pd_dual_f64': 0,
                    'sphrt_cp_ray_dual_f64': 0}
    print(f'chambolle_pock generic {cfg}:', end='')
    _check(cfg, x, y_hat, info, gpu)
    xr, _, ir = _reference(cfg)
    d_x, d_p, d_q = cp.bounds(cfg, xr, ir['ray_dual'], ir['dual'])
    assert float((x - xd).abs().max()) <= d_x
    assert float((info['ray_dual'] - idir['ray_dual']).abs().max()) <= d_p
    if cfg[2]:
        assert float((info['dual'] - idir['dual']).abs().max()) <= d_q


def test_short_runs_and_the_first_iterations(gpu):
    """num_iterations = 0, 1, 2: the histories' lengths, the start clamped into the bounds with
    the bounds' bits, and x0 unchanged."""
    from sph_raytracer_amd.retrieval import chambolle_pock
    _, y, mask, _ = cp.problem('tiny')
    y, op = y.to(gpu), _operator('tiny', 'stored', gpu)
    x0 = tr.linspace(-1, 2, 72, dtype=F64).reshape(4, 3, 6).to(gpu)
    for k in (0, 1, 2):
        x, _, info = chambolle_pock(op, y, cp.terms('abs', True), x0=x0, num_iterations=k,
                                    lower=cp.LOWER, upper=cp.UPPER)
        assert len(info['primal_change']) == len(info['fidelity']) == k
        assert bool(((x >= cp.LOWER) & (x <= cp.UPPER)).all())
        assert bool((x == cp.LOWER).any()) and bool((x == cp.UPPER).any())
    assert tr.equal(x0, tr.linspace(-1, 2, 72, dtype=F64).reshape(4, 3, 6).to(gpu))
