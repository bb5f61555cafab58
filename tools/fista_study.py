#!/usr/bin/env python3
"""The two CPU studies behind `retrieval.fista`'s constants, on dense systems taken from the loss
classes over the oracle-backed CpuOperator (tests/cpu_operator.py, tests/cg_cases.dense_system):

  step size   lambda_max / (Rayleigh quotient of the power method from the all-ones volume) after
              5, 10, 20, 30 and 50 steps — what `_fista_step` computes — on the two test problems
              (4 x 3 x 6, two views of 6 x 6 rays; 5 x 6 x 10, 257 rays), the four mask / smooth
              variants of each, and two larger oracle systems (8 x 6 x 8, six views of 8 x 8 rays;
              12 x 8 x 12, eight views of 10 x 10 rays).  The defaults of `power_iterations` and
              the margin follow from this table ("Bound-constrained solver").
  iterations  fista_dense against bounded_minimiser on the test problems with the bounds of the
              tests and without bounds: the iteration count at which the relative error first
              stays under 1e-12, and the error at the count the tests run
              (tests/fista_cases.py: ITERATIONS, LIMIT, MEASURED).

    python tools/fista_study.py [--large]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
F64 = tr.float64
STEPS = (5, 10, 20, 30, 50)
HORIZON = 3000


def problem(name):
    from cpu_operator import CpuOperator
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    if name == 'tiny':
        grid = SphericalGrid(shape=(4, 3, 6))
        geom = ConeRectGeom((6, 6), pos=(5, 0.3, 1), fov=(25, 25)) + \
            ConeRectGeom((6, 6), pos=(-1, 4.5, -2), fov=(25, 25))
    elif name == 'two_workgroups':
        grid = SphericalGrid(shape=(5, 6, 10))
        geom = ConeRectGeom((257, 1), pos=(4, 1, 0.5), fov=(50, 1))
    else:
        shape, views, side = ((8, 6, 8), 6, 8) if name == 'oracle_8x6x8' else ((12, 8, 12), 8, 10)
        grid = SphericalGrid(shape=shape)
        geom = None
        for v in range(views):
            a = 2 * math.pi * v / views
            one = ConeRectGeom((side, side), pos=(5 * math.cos(a), 5 * math.sin(a), 1.5 - 0.4 * v),
                               fov=(30, 30))
            geom = one if geom is None else geom + one
    op = CpuOperator(grid, geom)
    g = tr.Generator().manual_seed(11)
    truth = tr.rand(tuple(grid.shape), dtype=F64, generator=g)
    y = op(truth).detach()
    y = y + 0.01 * tr.randn(y.shape, dtype=F64, generator=g)
    mask = tr.rand(y.shape, dtype=F64, generator=g) + 0.25
    mask.view(-1)[3] = 0.0
    return op, y, mask


def terms(mask, masked, wrap):
    from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
    fns = [1.5 * SquareLoss(projection_mask=mask if masked else 1)]
    if wrap is not None:
        fns.append(0.3 * SmoothRegularizer(weights=(1, 0.5, 2), wrap_a=wrap))
    return fns


def system(name, masked, wrap):
    import cg_cases as cc
    op, y, mask = problem(name)
    fns, shape = terms(mask, masked, wrap), tuple(op.grid.shape)
    N0, _, _ = cc.dense_system(op, y, fns, 0.0, shape)
    damp = cc.damp_for(N0, math.prod(shape))
    N, b, _ = cc.dense_system(op, y, fns, damp, shape)
    return N, b


def rayleigh(N, steps):
    """_fista_step's estimate after each count of `steps` (numpy)."""
    v, out = np.ones(len(N)), {}
    for k in range(1, max(steps) + 1):
        w = N @ v
        rho = (v @ w) / (v @ v)
        v = w / np.linalg.norm(w)
        if k in steps:
            out[k] = rho
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--large', action='store_true', help='the two larger oracle systems too')
    args = ap.parse_args()
    import fista_cases as fc
    variants = [(False, None), (True, None), (False, True), (True, False)]
    names = [(n, m, w) for n in ('tiny', 'two_workgroups') for m, w in variants]
    if args.large:
        names += [('oracle_8x6x8', False, None), ('oracle_8x6x8', True, True),
                  ('oracle_12x8x12', False, None), ('oracle_12x8x12', True, True)]
    print('lambda_max / estimate after', STEPS, 'power steps')
    worst = {k: 0.0 for k in STEPS}
    systems = {}
    for key in names:
        N, b = system(*key)
        systems[key] = (N, b)
        lmax = float(np.linalg.eigvalsh(N)[-1])
        est = rayleigh(N, STEPS)
        ratio = {k: lmax / est[k] for k in STEPS}
        for k in STEPS:
            worst[k] = max(worst[k], ratio[k])
        print(key, ' '.join(f'{ratio[k]:.6f}' for k in STEPS), flush=True)
    print('worst', ' '.join(f'{worst[k]:.6f}' for k in STEPS))
    from sph_raytracer_amd import retrieval
    p, margin = retrieval._FISTA_POWER_ITERATIONS, retrieval._FISTA_MARGIN
    print(f'iterations to stay under {fc.STAYS_UNDER:g} (L as fista estimates it: {p} steps, '
          f'margin {margin})')
    rows = {}
    for key in names[:8]:
        N, b = systems[key]
        L = rayleigh(N, (p,))[p] * (1 + margin)
        for bounds in ((fc.LOWER, fc.UPPER), (-math.inf, math.inf)):
            want = fc.bounded_minimiser(N, b, *bounds)
            xs, restarts, _ = fc.fista_dense(N, b, L, *bounds, HORIZON)
            errs = [fc.cc.rel_err(x, want) for x in xs]
            rows[key + bounds] = (fc.first_stays_under(errs), errs, fc.shares(want, *bounds),
                                  restarts)
    K = max(r[0] for r in rows.values())
    for key, (k, errs, share, restarts) in rows.items():
        print(key, f'K {k}  error at K {errs[k]:.3g}  error at {K}: {errs[K]:.3g}  shares '
              f'{share[0]:.2f} / {share[1]:.2f} / {share[2]:.2f}  restarts {len(restarts)} '
              f'(first {restarts[:3]})', flush=True)
    worst_err = max(r[1][K] for r in rows.values())
    print(f'ITERATIONS = {K}; largest error at {K}: {worst_err:.3g}; LIMIT = '
          f'{max(100 * worst_err, 1e-12):.3g}')


if __name__ == '__main__':
    main()
