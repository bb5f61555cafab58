"""Cases, inputs and the CPU reference for retrieval.gd's direct loops as assembled (no tests; no
GPU dependency), shared by test_gd_cases_cpu.py (which shows on the reference alone that the
cases cover every pair of factor levels, hold what they claim and have the committed sensitivity)
and test_gpu_gd_matrix.py (which holds `retrieval._gd_direct` to them on the device).

`CASES` is a pairwise covering array over six factors of `_gd_direct`'s branches:

  F  fidelity    square | abs | huber | poisson            (the loss classes of those names)
  M  mask        unit | bool | f32_views | f64_full        (the fidelity term's projection_mask)
  Y  y dtype     f64 | f32
  R  terms       fid | neg | smooth | both                 (both: [fid, neg, smooth])
  O  operator    stored_reordered | stored_in_order | mf_atomic | mf_deterministic
  P  optimiser   adam | adam_fused | adam_wd | sgd

A row also names the smooth term's kind and ring closure (None without one).  The operator picks
the geometry: `stored_reordered` runs on circ16 (the suite's 12-view ConeCirc orbit over a 16^3
grid, a view-tiled trace whose direct loop permutes the measurements once), `stored_in_order` on
rect7 (7 ConeRect views: raytracer._view_tiles gives None, the trace stays in geometry order);
the matrix-free rows alternate.  rect7 has 294 rays over 378 voxels: two workgroups of the loss
kernels each way, neither a multiple of 256.

The reference is `retrieval.gd` itself on the CPU — its autograd loop, the loss classes and
torch's optimisers as they are — over tests/cpu_operator.CpuOperator: the system matrix from the
C oracle's segments of every ray, as float64 triplets, applied by numpy.  No HIP kernel runs.

`D_CASE` holds, per case, how far that reference moves when every row sum and every column sum
of the matrix is formed in the opposite order (`CpuOperator(reverse=True)`): the reference's own
sensitivity to what legitimately differs on the GPU.  `bounds(name)` turns it into the bound the
GPU test holds: 16 x d, at least 1e-13 of the reference's largest magnitude.
tools/gd_sensitivity.py prints the table; test_gd_cases_cpu.py recomputes it and holds it to a factor of two.
"""
import collections
import functools

import numpy as np
import torch as tr

N_IT = 10
F64, F32 = tr.float64, tr.float32

FACTORS = collections.OrderedDict([
    ('F', ('square', 'abs', 'huber', 'poisson')),
    ('M', ('unit', 'bool', 'f32_views', 'f64_full')),
    ('Y', ('f64', 'f32')),
    ('R', ('fid', 'neg', 'smooth', 'both')),
    ('O', ('stored_reordered', 'stored_in_order', 'mf_atomic', 'mf_deterministic')),
    ('P', ('adam', 'adam_fused', 'adam_wd', 'sgd')),
])

Case = collections.namedtuple('Case', 'name F M Y R O P smooth wrap geometry')

# (F, M, Y, R, O, P, smooth kind, wrap_a).  Rows 0-20: a covering array of every pair of levels;
# rows 21-23: two plain loops test_gd_cases_cpu.py restates by hand, and Poisson with a smooth
# term over a reordered stored trace under SGD.
_ROWS = [
    ('square', 'unit', 'f64', 'smooth', 'stored_in_order', 'adam_wd', 'square', None),
    ('square', 'bool', 'f32', 'smooth', 'mf_deterministic', 'adam_fused', 'huber', False),
    ('square', 'f32_views', 'f64', 'both', 'stored_reordered', 'sgd', 'abs', None),
    ('square', 'f32_views', 'f32', 'fid', 'mf_deterministic', 'adam', None, None),
    ('square', 'f64_full', 'f64', 'neg', 'mf_atomic', 'adam', None, None),
    ('abs', 'unit', 'f64', 'both', 'mf_deterministic', 'sgd', 'square', False),
    ('abs', 'unit', 'f32', 'neg', 'mf_deterministic', 'adam', None, None),
    ('abs', 'bool', 'f64', 'fid', 'mf_atomic', 'adam_wd', None, None),
    ('abs', 'f32_views', 'f64', 'both', 'stored_in_order', 'adam_fused', 'huber', None),
    ('abs', 'f64_full', 'f32', 'fid', 'stored_in_order', 'adam_fused', None, None),
    ('abs', 'f64_full', 'f32', 'smooth', 'stored_reordered', 'sgd', 'abs', False),
    ('huber', 'unit', 'f64', 'fid', 'stored_reordered', 'adam', None, None),
    ('huber', 'unit', 'f32', 'both', 'mf_atomic', 'adam_fused', 'square', None),
    ('huber', 'bool', 'f64', 'neg', 'stored_in_order', 'sgd', None, None),
    ('huber', 'f32_views', 'f32', 'smooth', 'mf_atomic', 'adam_wd', 'huber', False),
    ('huber', 'f64_full', 'f64', 'both', 'mf_deterministic', 'adam_wd', 'abs', None),
    ('poisson', 'unit', 'f64', 'smooth', 'mf_deterministic', 'adam', 'square', False),
    ('poisson', 'bool', 'f64', 'neg', 'stored_reordered', 'adam_wd', None, None),
    ('poisson', 'bool', 'f32', 'both', 'stored_in_order', 'adam', 'huber', None),
    ('poisson', 'f32_views', 'f64', 'neg', 'stored_reordered', 'adam_fused', None, None),
    ('poisson', 'f64_full', 'f64', 'fid', 'mf_atomic', 'sgd', None, None),
    ('square', 'unit', 'f64', 'fid', 'stored_reordered', 'sgd', None, None),
    ('huber', 'f32_views', 'f32', 'fid', 'mf_deterministic', 'adam_wd', None, None),
    ('poisson', 'f64_full', 'f32', 'smooth', 'stored_reordered', 'sgd', 'abs', None),
]

SMOOTH_DELTA = 0.25           # the smooth term's delta where its kind is 'huber'
# (no powers of two: a weight applied at another place in the chain then rounds otherwise)
LAM_FID, LAM_NEG, LAM_SMOOTH = 1.5, 3.0, 0.3


def _geometry_of(k, row):
    op = row[4]
    if op.startswith('stored'):
        return 'circ16' if op == 'stored_reordered' else 'rect7'
    return ('circ16', 'rect7')[k % 2]


def _name(k, row):
    return f'{k:02d}-' + '-'.join(str(v) for v in row[:6])


CASES = [Case(_name(k, row), *row, _geometry_of(k, row)) for k, row in enumerate(_ROWS)]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]

# What `_loop_terms` must refuse (the autograd loop runs, and must still give the reference):
# the fidelity term not first among three, a volume_mask, a tensor lam.
Declined = collections.namedtuple('Declined', Case._fields + ('why',))
_BASE = ('square', 'unit', 'f64', 'both', 'stored_reordered', 'adam', 'square', None, 'circ16')
DECLINED = [
    Declined('d0-neg-fid-smooth', *_BASE, 'neg_fid_smooth'),
    Declined('d1-smooth-neg-fid', *_BASE, 'smooth_neg_fid'),
    Declined('d2-volume-mask', *_BASE, 'volume_mask'),
    Declined('d3-tensor-lam', *_BASE, 'tensor_lam'),
]
BY_NAME.update({c.name: c for c in DECLINED})
DECLINED_NAMES = [c.name for c in DECLINED]

# ---- hyper-parameters, chosen on the CPU until test_gd_cases_cpu.py's input conditions hold ------
LR = {'adam': 0.03, 'adam_fused': 0.03, 'adam_wd': 0.03, 'sgd': {'circ16': 40.0, 'rect7': 8.0}}
LR_SGD_POISSON = {'circ16': 5.0, 'rect7': 1.0}  # (steeper near rays of few counts)
HUBER_DELTA = 0.3
POISSON_EPS = 0.1
NOISE = 0.02                  # the measurements' additive noise (not Poisson)
POISSON_FLOOR = 0.3           # background under the Poisson truth: few rays of intensity zero
NEG_FRACTION, NEG_SIZE = 0.10, 0.02
SEEDS = {}                    # case name -> seed, where the default (by position) was re-drawn


def optimiser(case):
    """(torch optimiser class, keyword arguments) of the case's P level."""
    if case.P == 'sgd':
        lr = (LR_SGD_POISSON if case.F == 'poisson' else LR['sgd'])[case.geometry]
        return tr.optim.SGD, dict(lr=lr, momentum=0.9)
    kw = dict(lr=LR[case.P])
    if case.P == 'adam_fused':
        kw['fused'] = True
    if case.P == 'adam_wd':
        kw.update(weight_decay=0.01, betas=(0.8, 0.95))
    return tr.optim.Adam, kw


# ---- geometries ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry(name):
    """(grid, geom) on the CPU."""
    from sph_raytracer_amd import ConeCircGeom, ConeRectGeom, SphericalGrid
    if name == 'circ16':        # test_gpu_weighted_gradient.circ16
        grid = SphericalGrid(shape=(16, 16, 16))
        geom = sum(ConeCircGeom(shape=(20, 16), pos=(5 * tr.cos(th), 5 * tr.sin(th), 1),
                                fov=(0, 45)) for th in tr.linspace(0, 2 * tr.pi, 12))
    else:                       # rect7: the (7, 20, 30) orbit of test_cpu_api.py, cut down
        grid = SphericalGrid(shape=(6, 7, 9))
        geom = sum(ConeRectGeom((6, 7), pos=(5 * tr.cos(th), 5 * tr.sin(th), 1), fov=(25, 25))
                   for th in tr.linspace(0, 2 * tr.pi, 7))
    return grid, geom


@functools.lru_cache(maxsize=None)
def cpu_operator(name, reverse=False):
    """The oracle's system matrix of a geometry behind Operator's call semantics."""
    from oracle import oracle
    from cpu_operator import CpuOperator
    oracle.use_mkl_sqrt(False)
    grid, geom = geometry(name)
    return CpuOperator(grid, geom, reverse=reverse)


def truth(name):
    """The blocky phantom of the suite's circ16 fixture, for either grid."""
    grid, _ = geometry(name)
    _, ne, na = grid.shape
    x = tr.zeros(tuple(grid.shape), dtype=F64)
    x[:, ne // 2:, :na // 2] = 1
    x[:, :ne // 2, na // 2:] = 1
    return x


# ---- inputs --------------------------------------------------------------------------------------
Inputs = collections.namedtuple('Inputs', 'y mask c0')


def _seed(case):
    return SEEDS.get(case.name, 1000 + 17 * (list(BY_NAME).index(case.name)))


def inputs(case):
    """The case's measurements, projection_mask (1 for a unit mask) and starting coefficients, as
    fresh CPU tensors, seeded by the case alone."""
    grid, geom = geometry(case.geometry)
    op = cpu_operator(case.geometry)
    g = tr.Generator().manual_seed(_seed(case))
    shape = tuple(op.ray_shape)
    with tr.no_grad():
        if case.F == 'poisson':
            y = tr.poisson(op._fwd(truth(case.geometry) + POISSON_FLOOR), generator=g)
        else:
            y = op._fwd(truth(case.geometry))
            y = y + NOISE * tr.randn(shape, dtype=F64, generator=g)
    y = y.to(F64 if case.Y == 'f64' else F32)
    u = tr.rand(shape, dtype=F64, generator=g)
    v = tr.rand(shape, dtype=F64, generator=g)
    if case.M == 'unit':
        mask = 1
    elif case.M == 'bool':
        mask = u > 0.3
    elif case.M == 'f32_views':         # (rows, columns), broadcast over the views
        mask = tr.where(u[0] < 0.3, 0.1 + 0.8 * v[0], tr.ones_like(v[0])).to(F32)
    else:
        mask = tr.where(u < 0.3, 0.1 + 0.8 * v, tr.ones_like(v))
    c0 = 0.5 + tr.rand(tuple(grid.shape), dtype=F64, generator=g)
    low = tr.rand(tuple(grid.shape), dtype=F64, generator=g) < NEG_FRACTION
    size = NEG_SIZE * (0.25 + tr.rand(tuple(grid.shape), dtype=F64, generator=g))
    c0 = tr.where(low, -size, c0)
    return Inputs(y, mask, c0)


def terms(case, mask, device='cpu'):
    """-> (loss_fns in the case's order, (fid, neg or None, smooth or None)); fresh objects."""
    from sph_raytracer_amd.loss import (AbsLoss, HuberLoss, NegRegularizer, PoissonLoss,
                                        SmoothRegularizer, SquareLoss)
    why = getattr(case, 'why', None)
    kw = dict(projection_mask=mask, lam=LAM_FID)
    if why == 'volume_mask':
        grid, _ = geometry(case.geometry)
        vm = tr.ones(tuple(grid.shape), dtype=F64, device=device)
        vm[0] = 0.5
        kw['volume_mask'] = vm
    fid = {'square': SquareLoss, 'abs': AbsLoss,
           'huber': functools.partial(HuberLoss, HUBER_DELTA),
           'poisson': functools.partial(PoissonLoss, POISSON_EPS)}[case.F](**kw)
    neg = smooth = None
    if case.R in ('neg', 'both'):
        neg = (tr.tensor(LAM_NEG, dtype=F64, device=device) if why == 'tensor_lam'
               else LAM_NEG) * NegRegularizer()
    if case.R in ('smooth', 'both'):
        smooth = LAM_SMOOTH * SmoothRegularizer(
            kind=case.smooth, delta=SMOOTH_DELTA if case.smooth == 'huber' else None,
            wrap_a=case.wrap)
    order = {'neg_fid_smooth': [neg, fid, smooth], 'smooth_neg_fid': [smooth, neg, fid]}.get(
        why, [fid, neg, smooth])
    return [fn for fn in order if fn is not None], (fid, neg, smooth)


# ---- the reference -------------------------------------------------------------------------------
Result = collections.namedtuple('Result', 'c y hist')     # numpy arrays; hist: one list per term


def run_gd(op, case, inp, device='cpu'):
    """retrieval.gd over `op` with the case's terms and optimiser on copies of `inp` moved to
    `device` -> (Result, the tensors handed in (y, mask, c0), the terms (fid, neg, smooth))."""
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.model import FullyDenseModel
    grid, _ = geometry(case.geometry)
    y = inp.y.clone().to(device)
    mask = inp.mask.clone().to(device) if isinstance(inp.mask, tr.Tensor) else inp.mask
    c0 = inp.c0.clone().to(device)
    fns, parts = terms(case, mask, device)
    optim, kw = optimiser(case)
    c, yhat, hist = retrieval.gd(op, y, FullyDenseModel(grid), coeffs=c0, num_iterations=N_IT,
                                 loss_fns=fns, optim=optim, progress_bar=False, **kw)
    assert list(hist) == fns
    res = Result(c.detach().cpu().numpy().copy(), yhat.detach().cpu().numpy().copy(),
                 [[float(v) for v in hist[fn]] for fn in fns])
    return res, (y, mask, c0), parts


@functools.lru_cache(maxsize=None)
def reference(name, reverse=False):
    """Coefficients, reconstructed stack and loss histories of the case after N_IT iterations of
    retrieval.gd's autograd loop on the CPU over the oracle's matrix.  reverse: the matrix with
    every row and column summed in the opposite order."""
    case = BY_NAME[name]
    res, _, _ = run_gd(cpu_operator(case.geometry, reverse), case, inputs(case))
    return res


def distance(a, b):
    """(max |c_a - c_b|, max |y_a - y_b|, [max |h_a - h_b| per term]) of two Results."""
    return (float(np.abs(a.c - b.c).max()), float(np.abs(a.y - b.y).max()),
            [float(np.abs(np.subtract(p, q)).max()) for p, q in zip(a.hist, b.hist)])


def sensitivity(name):
    """d_case: `distance` of the reference and its reversed-order run."""
    return distance(reference(name), reference(name, True))


FACTOR, FLOOR, ILL = 16, 1e-13, 1e-6


def bounds(name):
    """The bounds the GPU holds for coefficients, stack and each loss history: FACTOR x the
    committed d, at least FLOOR x the reference's largest magnitude of that quantity."""
    ref = reference(name)
    d_c, d_y, d_h = D_CASE[name]
    return (max(FACTOR * d_c, FLOOR * float(np.abs(ref.c).max())),
            max(FACTOR * d_y, FLOOR * float(np.abs(ref.y).max())),
            [max(FACTOR * d, FLOOR * float(np.abs(h).max())) for d, h in zip(d_h, ref.hist)])


# name -> (d of the coefficients, d of the stack, [d of each loss history]), as
# tools/gd_sensitivity.py prints them
D_CASE = {
    '00-square-unit-f64-smooth-stored_in_order-adam_wd':
        (2.220e-16, 4.441e-16, [5.551e-17, 2.776e-17]),
    '01-square-bool-f32-smooth-mf_deterministic-adam_fused':
        (3.261e-16, 4.441e-16, [5.551e-17, 6.939e-18]),
    '02-square-f32_views-f64-both-stored_reordered-sgd':
        (9.437e-16, 8.882e-16, [5.551e-17, 6.939e-18, 5.551e-17]),
    '03-square-f32_views-f32-fid-mf_deterministic-adam': (4.441e-16, 4.441e-16, [1.110e-16]),
    '04-square-f64_full-f64-neg-mf_atomic-adam': (1.110e-15, 1.110e-15, [2.776e-17, 8.674e-19]),
    '05-abs-unit-f64-both-mf_deterministic-sgd':
        (4.441e-16, 4.441e-16, [5.551e-17, 1.388e-17, 1.388e-17]),
    '06-abs-unit-f32-neg-mf_deterministic-adam': (4.441e-16, 1.110e-15, [5.551e-17, 8.674e-19]),
    '07-abs-bool-f64-fid-mf_atomic-adam_wd': (2.220e-16, 4.441e-16, [2.776e-17]),
    '08-abs-f32_views-f64-both-stored_in_order-adam_fused':
        (3.331e-16, 6.661e-16, [1.110e-16, 2.168e-19, 0.000e+00]),
    '09-abs-f64_full-f32-fid-stored_in_order-adam_fused': (3.331e-16, 8.882e-16, [5.551e-17]),
    '10-abs-f64_full-f32-smooth-stored_reordered-sgd':
        (8.882e-16, 8.882e-16, [5.551e-17, 5.551e-17]),
    '11-huber-unit-f64-fid-stored_reordered-adam': (2.887e-15, 8.882e-16, [1.388e-17]),
    '12-huber-unit-f32-both-mf_atomic-adam_fused':
        (6.106e-16, 1.554e-15, [2.776e-17, 0.000e+00, 0.000e+00]),
    '13-huber-bool-f64-neg-stored_in_order-sgd': (4.441e-16, 4.441e-16, [1.388e-17, 1.193e-18]),
    '14-huber-f32_views-f32-smooth-mf_atomic-adam_wd':
        (2.220e-16, 8.882e-16, [2.776e-17, 0.000e+00]),
    '15-huber-f64_full-f64-both-mf_deterministic-adam_wd':
        (2.220e-16, 4.441e-16, [1.388e-17, 0.000e+00, 0.000e+00]),
    '16-poisson-unit-f64-smooth-mf_deterministic-adam':
        (1.638e-15, 1.110e-15, [1.110e-16, 0.000e+00]),
    '17-poisson-bool-f64-neg-stored_reordered-adam_wd':
        (2.220e-16, 1.110e-15, [5.551e-17, 5.421e-20]),
    '18-poisson-bool-f32-both-stored_in_order-adam':
        (6.939e-16, 4.441e-16, [1.110e-16, 1.097e-19, 1.388e-17]),
    '19-poisson-f32_views-f64-neg-stored_reordered-adam_fused':
        (3.775e-15, 1.332e-15, [1.110e-16, 4.066e-20]),
    '20-poisson-f64_full-f64-fid-mf_atomic-sgd': (2.220e-16, 1.110e-15, [1.110e-16]),
    '21-square-unit-f64-fid-stored_reordered-sgd': (7.772e-16, 1.332e-15, [1.110e-16]),
    '22-huber-f32_views-f32-fid-mf_deterministic-adam_wd': (1.867e-15, 8.882e-16, [1.388e-17]),
    '23-poisson-f64_full-f32-smooth-stored_reordered-sgd':
        (4.441e-16, 1.332e-15, [5.551e-17, 1.110e-16]),
    'd0-neg-fid-smooth': (5.759e-16, 8.882e-16, [6.505e-19, 5.551e-17, 5.551e-17]),
    'd1-smooth-neg-fid': (6.661e-16, 1.110e-15, [2.776e-17, 5.421e-19, 1.110e-16]),
    'd2-volume-mask': (8.882e-16, 8.882e-16, [1.110e-16, 4.337e-19, 1.388e-17]),
    'd3-tensor-lam': (1.110e-15, 1.110e-15, [5.551e-17, 6.505e-19, 2.776e-17]),
}
