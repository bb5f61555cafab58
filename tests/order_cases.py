"""Small named geometries for the trace-order layer, and their oracle references (no tests here).

The layer between a geometry and the kernels (raytracer._view_tiles, _trace_order / _wedge_order,
SPHRT_RAY_ORDER, the ray generators and the ray_id map) decides the order rays are traced in and
maps every CSR row back to its geometry ray.  Each case below is a deterministic (grid, geom,
env) picked for one decision of that layer; `reference(name)` is the C oracle's answer for it in
geometry order: the segments of `geom.rays` flattened as they stand (starts by find_starts, IEEE
square roots as in test_gpu_fuzz.py), and its forward and adjoint on those segments.

Nothing here is symmetric, so that a ray paired with the wrong pixel, view or time slice changes
the answer (tests/test_order_cases_cpu.py asserts it on the references alone): the grids have
irregular boundary vectors (test_gpu_fuzz._bounds) of 6-12 voxels per axis, one with a partial
azimuth range and one hollow; the viewpoints sit on an open, tilted path of varying radius and
height, so no two views mirror each other; the densities are uniform random numbers.
"""
import contextlib
import functools
import math
import os
from collections import namedtuple

import numpy as np
import torch as tr

Case = namedtuple('Case', 'name kind shape grid env dynamic')
Case.__new__.__defaults__ = (None, False)

# kind: 'rect' / 'circ' (one detector, or an orbit when the shape has three entries), 'mixed'
# (ConeRect and ConeCirc views alternating), 'parallel'.  grid: 'full' / 'partial' / 'hollow'.
CASES = [
    Case('rect_8x3x6', 'rect', (8, 3, 6), 'full'),              # tile (8, 2)
    Case('rect_9x4x5', 'rect', (9, 4, 5), 'partial'),           # odd width: tw = 1
    Case('rect_7x4x6', 'rect', (7, 4, 6), 'hollow'),            # fewer than 8 views: natural
    Case('rect_67x2x4', 'rect', (67, 2, 4), 'partial'),         # prime above 64: no tile
    Case('rect_130x1x2', 'rect', (130, 1, 2), 'full'),          # tv = 26, h = 1
    Case('rect_128x1x2', 'rect', (128, 1, 2), 'hollow'),        # tv = 64
    Case('rect_16x2x1', 'rect', (16, 2, 1), 'full'),            # w = 1
    Case('circ_5x7', 'circ', (5, 7), 'partial'),                # wedge with remainder
    Case('circ_6x9', 'circ', (6, 9), 'hollow'),                 # wedge
    Case('circ_4x3', 'circ', (4, 3), 'full'),                   # no wedge
    Case('circ_1x8', 'circ', (1, 8), 'partial'),                # h = 1
    Case('circ_8x5x7', 'circ', (8, 5, 7), 'hollow'),            # tile and wedge compete
    Case('circ_5x4x8', 'circ', (5, 4, 8), 'full'),              # no tile, wedge per view
    Case('mixed_6x4x7', 'mixed', (6, 4, 7), 'partial'),         # not all ConeCirc: no wedge
    Case('parallel_5x6', 'parallel', (5, 6), 'hollow'),
    Case('dyn_rect_8x3x6', 'rect', (8, 3, 6), 'full', None, True),
    Case('dyn_circ_8x5x7', 'circ', (8, 5, 7), 'partial', None, True),
    Case('natural_circ_8x5x7', 'circ', (8, 5, 7), 'full', 'natural'),
    Case('vtile_rect_12x2x6', 'rect', (12, 2, 6), 'hollow', 'vtile:4,1,3'),
    Case('vtile_refused_rect_12x2x6', 'rect', (12, 2, 6), 'partial', 'vtile:5,1,4'),
]
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
STATIC = [c.name for c in CASES if not c.dynamic]
DYNAMIC = [c.name for c in CASES if c.dynamic]
STATIC_ORBITS = [c.name for c in CASES if not c.dynamic and len(c.shape) == 3]

SCALE = 4.0     # compare_segments' length scale: above the outer radius and every viewpoint


def _seed(case):
    return 1000 + NAMES.index(case.name)


def _bounds(rng, n, lo, hi):
    """n + 1 ascending boundaries from lo to hi, gaps random but at least (hi - lo) / (8 n)
    (test_gpu_fuzz._bounds)."""
    w = rng.uniform(1.0, 8.0, n)
    w = w / w.sum() * (hi - lo)
    return np.concatenate([[lo], lo + np.cumsum(w)[:-1], [hi]])


def _boundaries(case, rng):
    nr, ne, na = (int(v) for v in rng.integers(6, 13, 3))
    r0 = 0.3 if case.grid == 'hollow' else 0.0
    a_lo, a_hi = (-2.0, 1.3) if case.grid == 'partial' else (-math.pi, math.pi)
    return (_bounds(rng, nr, r0, 1.0), _bounds(rng, ne, 0.0, math.pi), _bounds(rng, na, a_lo, a_hi))


def _path(n, rng):
    """n viewpoints on an open arc (under a full turn) of varying radius and height, tilted about
    the x axis: no rotation or reflection maps one viewpoint to another."""
    phi = 0.3 + 5.1 * (np.arange(n) + 0.37 * np.sin(1.9 * np.arange(n))) / max(n, 2)
    rad = 3.0 + 0.4 * np.sin(1.7 * phi + 0.4) + rng.uniform(-0.2, 0.2, n)
    z = 0.5 * np.cos(1.3 * phi + 1.0) + 0.25 + rng.uniform(-0.2, 0.2, n)
    p = np.stack([rad * np.cos(phi), rad * np.sin(phi), z], 1)
    t = 0.35
    rot = np.array([[1, 0, 0], [0, math.cos(t), -math.sin(t)], [0, math.sin(t), math.cos(t)]])
    return p @ rot.T


def _view(kind, det, pos):
    from sph_raytracer_amd import ConeCircGeom, ConeRectGeom, ParallelGeom
    pos = tuple(float(v) for v in pos)
    if kind == 'rect':      # the unit sphere spans +-19.5 degrees from 3 away
        return ConeRectGeom(det, pos=pos, fov=(22, 25))
    if kind == 'circ':      # a hollow cone: no degenerate ring of equal rays on the axis
        return ConeCircGeom(det, pos=pos, fov=(6, 34))
    return ParallelGeom(det, pos=pos, size=(1.5, 1.3))


def build(case):
    """-> (grid, geom, env): env holds the environment the Operator is built and run under."""
    from sph_raytracer_amd import SphericalGrid
    if isinstance(case, str):
        case = BY_NAME[case]
    rng = np.random.default_rng(_seed(case))
    kw = dict(zip(('r_b', 'e_b', 'a_b'), (tr.from_numpy(b) for b in _boundaries(case, rng))))
    orbit = len(case.shape) == 3
    if case.dynamic:        # as make_golden.py's dynamic_obs: one time slice per view
        kw['t'] = tr.arange(case.shape[0], dtype=tr.float64)
    grid = SphericalGrid(**kw)
    det = tuple(case.shape[-2:])
    pts = _path(case.shape[0] if orbit else 1, rng)
    kinds = ('rect', 'circ') if case.kind == 'mixed' else (case.kind,)
    views = [_view(kinds[i % len(kinds)], det, p) for i, p in enumerate(pts)]
    geom = sum(views) if orbit else views[0]
    env = {'SPHRT_RAY_ORDER': case.env} if case.env else {}
    return grid, geom, env


@contextlib.contextmanager
def applied(env):
    """SPHRT_RAY_ORDER as the case asks (unset for an empty env), restored afterwards."""
    old = os.environ.pop('SPHRT_RAY_ORDER', None)
    os.environ.update(env)
    try:
        yield
    finally:
        os.environ.pop('SPHRT_RAY_ORDER', None)
        if old is not None:
            os.environ['SPHRT_RAY_ORDER'] = old


def decisions(case):
    """What the trace-order layer decides for a case under its env, by the library's own pure
    Python rules as Operator._trace_on applies them: (view tile or None, wedge order or None)."""
    from sph_raytracer_amd import raytracer as rt
    grid, geom, env = build(case)
    shape = tuple(geom.shape)
    with applied(env):
        tiles = None
        if rt._ConeRays.of(geom) is not None and len(shape) == 3 and shape[0] > 1:
            tiles = rt._view_tiles(shape, grid.dynamic)
        wedge = None
        if tiles is None:
            wedge = rt._trace_order(geom, tr.empty(shape + (3,), device='meta'), grid.dynamic)
    return tiles, wedge


def _oracle():
    from oracle import oracle
    oracle.use_mkl_sqrt(False)
    return oracle


Reference = namedtuple('Reference', 'segs n_vox x x3 y y3 yt xt view_segs')


def view_forward(ref, v, density):
    """The oracle's forward of view v alone (a dynamic case) on a (nr, ne, na) density."""
    return np.asarray(_oracle().forward(*ref.view_segs[v], density, ref.n_vox))[0]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's answer for a case, in geometry order, computed once:

    segs      (ptr, vox, len) of every ray of geom.rays, flattened as it stands
    x, x3     the case's random densities: grid.shape, and three channels (static cases)
    y, y3     the oracle's forward of x (geom.shape) and x3 ((3,) + geom.shape); for a dynamic
              case view v integrates time slice v (the oracle called once per view on its slice)
    yt, xt    a random y of geom.shape and the oracle's adjoint of it (grid.shape; dynamic: slice
              t holds view t's back-projection alone)
    view_segs the segments of each view alone (dynamic cases), else None
    Arrays are numpy float64; treat them as read-only."""
    from sph_raytracer_amd.raytracer import find_starts
    case = BY_NAME[name]
    ora = _oracle()
    grid, geom, _ = build(case)
    shape = tuple(int(v) for v in geom.shape)
    gshape = tuple(int(v) for v in grid.shape)
    n_vox = math.prod(gshape[-3:])
    xs, rays = geom.ray_starts, geom.rays
    starts = find_starts(grid, xs).numpy()
    g = ora.Grid.from_boundaries(grid.r_b.numpy(), grid.e_b.numpy(), grid.a_b.numpy())
    xs, rays = xs.numpy(), rays.numpy()
    segs = ora.trace_segments(g, xs, rays, starts)
    gen = tr.Generator().manual_seed(_seed(case))
    x = tr.rand(gshape, dtype=tr.float64, generator=gen).numpy()
    yt = tr.rand(shape, dtype=tr.float64, generator=gen).numpy()
    if not case.dynamic:
        x3 = tr.rand((3,) + gshape, dtype=tr.float64, generator=gen).numpy()
        y = np.asarray(ora.forward(*segs, x, n_vox)).reshape(shape)
        y3 = np.asarray(ora.forward(*segs, x3, n_vox)).reshape((3,) + shape)
        xt = np.asarray(ora.adjoint(*segs, yt, n_vox)).reshape(gshape)
        view_segs = None
    else:
        x3 = y3 = None
        view_segs = [ora.trace_segments(g, xs[v], rays[v], starts[:, v]) for v in range(shape[0])]
        y = np.stack([np.asarray(ora.forward(*view_segs[v], x[v], n_vox)).reshape(shape[1:])
                      for v in range(shape[0])])
        xt = np.stack([np.asarray(ora.adjoint(*view_segs[v], yt[v], n_vox)).reshape(gshape[1:])
                       for v in range(shape[0])])
    for a in (x, x3, y, y3, yt, xt):
        if a is not None:
            a.setflags(write=False)
    return Reference(segs, n_vox, x, x3, y, y3, yt, xt, view_segs)
