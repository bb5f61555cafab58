"""Host side of the Poisson fidelity (sphrt_trace_normal_poisson_f64, sphrt_poisson_residual_f64,
MatrixFreeOperator.residual_gradient(loss='poisson', eps=...), loss.PoissonLoss): the entries are
declared, exported and bound; their refusals fire on the host; PoissonLoss over the oracle-backed
CpuOperator equals the formula written out in numpy, value and gradient; bad loss / eps / delta
arguments are refused before any device is looked for; distributed.gd declines the term and cg
names it.  (No compute call of the library: no GPU here.  retrieval._loop_terms asks for
coefficients on a GPU before it looks at a loss term, so its conditions are in
tests/test_gpu_poisson_gradient.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch as tr

from test_matrix_free_gradient_cpu import _host_plan, _operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'sphrt_trace_normal_poisson_f64': 15, 'sphrt_poisson_residual_f64': 11}
BAD_EPS = (0.0, -0.0, -1e-8, float('inf'), -float('inf'), float('nan'))


def test_entries_declared_exported_and_bound():
    from sph_raytracer_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, 'include', 'sphrt.h')).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for entry, n_args in ENTRIES.items():
        m = re.search(r'int\s+' + entry + r'\s*\(([^;]*)\)\s*;', hdr)
        assert m, f'{entry} is not declared in include/sphrt.h'
        assert len(m.group(1).split(',')) == n_args
        assert 'const double *ray_scale' in m.group(1) and 'double eps' in m.group(1)
        assert 'int kind' not in m.group(1) and 'delta' not in m.group(1)
        assert entry in _lib.EXPORTED and hasattr(raw, entry)
        fn = getattr(_lib.load(), entry)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
        # one double by value: eps
        assert fn.argtypes.count(ctypes.c_double) == 1
    lib = _lib.load()
    assert lib.sphrt_trace_normal_poisson_f64.argtypes.index(ctypes.c_double) == 5
    assert lib.sphrt_poisson_residual_f64.argtypes.index(ctypes.c_double) == 4
    # there is no fixed-point entry, and the earlier entries keep their signatures
    assert not hasattr(raw, 'sphrt_trace_normal_poisson_fixed_f64')
    assert len(lib.sphrt_trace_normal_robust_f64.argtypes) == 16
    assert len(lib.sphrt_robust_residual_f64.argtypes) == 12
    assert len(lib.sphrt_trace_normal_weighted_f64.argtypes) == 14
    # the header states the confirmed operation sequence and the two-trace deterministic form
    tail = hdr[hdr.index("The Poisson fidelity's tail"):hdr.index('int sphrt_poisson_residual_f64')]
    assert 's + ((-s) * y[i]) / q' in tail and 'q           = p + eps' in tail
    mode = hdr[hdr.index('Poisson fidelity: sphrt_trace_normal_weighted_f64'):
               hdr.index('int sphrt_trace_normal_poisson_f64')]
    assert 'no fixed-point form' in mode
    for step in ('sphrt_trace_integrate_f64', 'sphrt_poisson_residual_f64',
                 'sphrt_fixed_scale_f64(a = r_scaled', 'sphrt_trace_backproject_fixed_f64',
                 'sphrt_fixed_finalize_f64'):
        assert step in mode, step


def test_poisson_normal_refusals_on_the_host():
    """The weighted entry's refusals and an eps that is not finite and > 0, each with its word in
    sphrt_last_error before the library asks for a device."""
    from sph_raytracer_amd import SphericalGrid, _lib
    lib = _lib.load()
    grid = SphericalGrid(shape=(4, 5, 6))
    plan, _keep = _host_plan(grid)
    vol, n = 4 * 5 * 6, 10
    rays = _lib.RayBatch()
    rays.ndim = 1
    rays.shape[0] = n
    rays.xs_stride[0] = rays.rays_stride[0] = 3
    p = ctypes.c_void_p(16)      # never dereferenced: every call below fails its checks first
    rays.xs = rays.rays = rays.start = 16
    need = lib.sphrt_trace_workspace_bytes(plan.handle, n)

    def call(eps=1e-8, plan=plan.handle, rays=ctypes.byref(rays), d=p, m=p, rs=p, n_chan=1,
             cs=vol, div=0, yhat=p, ycs=n, acc=p, ws=p, ws_size=need):
        return lib.sphrt_trace_normal_poisson_f64(plan, rays, d, m, rs, eps, n_chan, cs, div,
                                                  yhat, ycs, acc, ws, ws_size, None)

    cases = [
        (dict(plan=None), b'null plan'),
        (dict(rays=None), b'null ray batch'),
        (dict(d=None), b'density, m, yhat or acc'),
        (dict(m=None), b'density, m, yhat or acc'),
        (dict(yhat=None), b'density, m, yhat or acc'),
        (dict(acc=None), b'density, m, yhat or acc'),
        (dict(rs=None), b'null ray_scale'),
        (dict(n_chan=0), b'n_chan'),
        (dict(n_chan=3, div=5), b'ray_chan_div'),
        (dict(cs=vol - 1), b'chan_stride'),
        (dict(n_chan=2, ycs=n - 1), b'y_chan_stride'),
        (dict(ws_size=need - 1), b'workspace too small'),
        (dict(ws=None), b'workspace too small'),
    ]
    for eps in (1e-8, 1.0, 5e-324):
        for i, (kw, word) in enumerate(cases):
            assert call(eps, **kw) != 0, (eps, i)
            assert word in lib.sphrt_last_error(), (eps, i, lib.sphrt_last_error())
    for eps in BAD_EPS:
        assert call(eps) != 0, eps
        assert b'eps must be finite and > 0' in lib.sphrt_last_error()


def test_poisson_residual_refusals_on_the_host():
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    p, none = ctypes.c_void_p(16), None
    fn = lib.sphrt_poisson_residual_f64
    for n in (0, -3):
        assert fn(p, p, 1, n, 1e-8, p, p, none, p, p, none) != 0
        assert b'empty' in lib.sphrt_last_error()
    for k in (0, 1, 5, 6, 8, 9):          # yhat, y, ray_scale, weight, r_scaled, partial_sums
        for order in (none, p):
            args = [p, p, 1, 8, 1e-8, p, p, order, p, p, none]
            args[k] = none
            assert fn(*args) != 0 and b'null' in lib.sphrt_last_error(), k
    for eps in BAD_EPS:
        assert fn(p, p, 1, 8, eps, p, p, none, p, p, none) != 0, eps
        assert b'eps must be finite and > 0' in lib.sphrt_last_error()


@pytest.mark.parametrize('ydt', [tr.float64, tr.float32], ids=['y64', 'y32'])
def test_poisson_loss_value_and_gradient_by_hand(ydt):
    """PoissonLoss over the oracle-backed CpuOperator: lam * mean(mask * (p - y log(p + eps)))
    and its gradient A^T((lam / N) * mask * (1 - y / (p + eps))), both written out in numpy, and
    the value equal to torch's poisson_nll_loss under the mask and the mean."""
    from cpu_operator import CpuOperator
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    from sph_raytracer_amd.loss import Loss, PoissonLoss
    grid, geom = SphericalGrid(shape=(6, 5, 8)), ConeRectGeom((9, 7), pos=(5, 0.3, 1), fov=(25, 25))
    op = CpuOperator(grid, geom)
    g = tr.Generator().manual_seed(5)
    d = 0.5 + tr.rand(grid.shape, dtype=tr.float64, generator=g)
    p = op(d).detach()
    y = tr.poisson(20 * p, generator=g).to(ydt)             # counts; 0 where the ray misses
    assert bool((y > 0).any()) and bool((y == 0).any())
    mask = tr.rand(geom.shape, dtype=tr.float64, generator=g) * 2 - 0.5
    mask[0, :3] = 0
    lam = 2.5
    p_np, y_np = p.numpy(), y.double().numpy()
    for eps in (1e-8, 0.5):
        for pm, m_np in ((mask, mask.numpy()), (1, np.ones(p_np.shape))):
            fn = lam * PoissonLoss(eps=eps, projection_mask=pm)
            assert isinstance(fn, Loss) and fn.kind == 'fidelity' and fn.eps == eps
            dd = d.clone().requires_grad_()
            val = fn(op, y, dd, None)
            assert val.dtype == tr.float64
            want = lam * np.mean(m_np * (p_np - y_np * np.log(p_np + eps)))
            assert abs(float(val.detach()) - want) <= 1e-14 * abs(want)
            nll = tr.nn.functional.poisson_nll_loss(p, y.double(), log_input=False, full=False,
                                                    eps=eps, reduction='none')
            masked = nll if isinstance(pm, int) else pm * nll
            assert float(val.detach()) == float(lam * tr.mean(masked))
            val.backward()
            back = (lam / p_np.size) * m_np * (1 - y_np / (p_np + eps))
            gw = op.T(tr.from_numpy(back)).numpy()
            err = np.abs(dd.grad.numpy() - gw).max()
            assert err <= 1e-13 * np.abs(gw).max(), err
    # the default eps is torch's 1e-8; an eps that is not a finite real > 0 is refused
    assert PoissonLoss().eps == 1e-8 and PoissonLoss(volume_mask=2).volume_mask == 2
    assert PoissonLoss(eps=np.float32(0.5)).eps == 0.5 and type(PoissonLoss(eps=2).eps) is float
    for bad in (0, -1.0, float('inf'), float('nan'), None, True, '1', tr.tensor(0.5)):
        with pytest.raises(ValueError, match='eps'):
            PoissonLoss(eps=bad)


def test_distributed_gd_declines_and_cg_names_the_term():
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.distributed import _declined
    from sph_raytracer_amd.loss import NegRegularizer, PoissonLoss, SquareLoss
    assert _declined([PoissonLoss()]) and _declined([PoissonLoss(eps=0.5), NegRegularizer()])
    assert _declined([NegRegularizer(), 2 * PoissonLoss()])
    assert not _declined([SquareLoss(), NegRegularizer()])
    assert retrieval._FIDELITY[-1] is PoissonLoss and retrieval._poisson_of(PoissonLoss(0.5)) == 0.5
    assert retrieval._poisson_of(SquareLoss()) is None

    class MyPoisson(PoissonLoss):
        pass

    assert retrieval._poisson_of(MyPoisson()) is None and type(MyPoisson()) not in retrieval._FIDELITY
    for fns in ([PoissonLoss()], [SquareLoss(), PoissonLoss()]):
        with pytest.raises(ValueError, match='PoissonLoss is neither'):
            retrieval.cg(None, tr.ones(3), loss_fns=fns)


def test_bad_loss_arguments_are_refused_before_any_device(monkeypatch):
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid, _lib
    from sph_raytracer_amd.raytracer import POISSON_EPS, _poisson_args

    def never(*a, **k):
        raise AssertionError('an argument error must come before the device')

    monkeypatch.setattr(_lib, 'require_gpu', never)
    grid, geom = SphericalGrid((4, 4, 4)), ConeRectGeom((4, 5), (5, 0, 0))
    op = _operator(grid, geom)
    x, m = tr.ones(4, 4, 4), tr.ones(4, 5)
    for loss in ('Poisson', 'poisson_nll', '', None, 1, ['poisson']):
        with pytest.raises(ValueError, match="or 'poisson'"):
            op.residual_gradient(x, m, loss=loss)
    for bad in (0, 0.0, -0.5, float('inf'), float('nan'), True, '1e-8', tr.tensor(0.5)):
        with pytest.raises(ValueError, match="needs a finite eps > 0"):
            op.residual_gradient(x, m, loss='poisson', eps=bad)
    for loss, kw in (('square', {}), ('abs', {}), ('huber', dict(delta=0.5))):
        with pytest.raises(ValueError, match="eps belongs to loss='poisson'"):
            op.residual_gradient(x, m, loss=loss, eps=1e-8, **kw)
    with pytest.raises(ValueError, match="delta belongs to loss='huber'"):
        op.residual_gradient(x, m, loss='poisson', delta=0.5)
    with pytest.raises(ValueError, match="delta belongs to loss='huber'"):
        op.residual_gradient(x, m, loss='poisson', delta=0.5, eps=1e-8)
    # a real number is an eps, whatever its type (a tensor is not: reading it could sync)
    for good in (0.5, 1, np.float32(0.5), np.float64(1e-8), np.int64(2)):
        assert _poisson_args('poisson', None, good) == float(good)
    assert POISSON_EPS == 1e-8 and _poisson_args('poisson', None, None) == 1e-8
    assert _poisson_args('square', None, None) is None and _poisson_args('huber', 0.5, None) is None
    for shape in ((4, 6), (5, 4), (3,), (1, 4, 5)):
        with pytest.raises(ValueError, match='do not broadcast'):
            op.residual_gradient(x, m, 0.5, weights=tr.ones(shape), loss='poisson')
    with pytest.raises(TypeError, match='bool, float32 or float64'):
        op.residual_gradient(x, m, weights=tr.ones(4, 5, dtype=tr.int32), loss='poisson')
    with pytest.raises(ValueError, match='ray shape'):
        op.residual_gradient(x, tr.ones(4, 6), loss='poisson', eps=0.5)
