#!/usr/bin/env python3
"""The CPU study behind the constants of tests/pd_cases.py (ITERATIONS, LIMIT, MEASURED), on the
dense systems of the solver tests — the loss classes over the oracle-backed CpuOperator
(tests/cpu_operator.py, tests/cg_cases.dense_system), D from pd_cases.tv_matrix:

  certificate  pd_cases.certify on every case: the relative radius sqrt(2 gap / lam_min) / |x*|
               of the ball that holds the true minimiser, and the shares of edges that are flat
               (|q| < c) and that carry a jump at the minimiser (both must be non-zero: lam_tv);
  iterations   pd_dense against the certified minimiser: the iteration count at which the
               relative error first stays under pd_cases.STAYS_UNDER, and the error at the count
               the tests run.

Prints the MEASURED table as it stands in pd_cases.py (the case builders are test_pd_cpu.py's).

    python tools/pd_study.py [--horizon N] [--ratio R ...]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import numpy as np

    import cg_cases as cc
    import pd_cases as pc
    import test_pd_cpu as tp
    ap = argparse.ArgumentParser()
    ap.add_argument('--horizon', type=int, default=pc.K_CAP + 2000)
    ap.add_argument('--ratio', type=float, nargs='*', default=[],
                    help='also: the iteration count under other dual_ratio values')
    args = ap.parse_args()
    rows = {}
    for name in ('tiny', 'two_workgroups'):
        for masked, wrap in pc.VARIANTS:
            for lower, upper in tp.BOUNDS:
                key = (name, masked, wrap, lower is not None)
                k, at, radius, (flat, jump) = tp.measure(name, masked, wrap, lower, upper,
                                                         horizon=args.horizon)
                rows[key] = (k, at, radius)
                extra = ''
                if args.ratio:
                    _, _, N, b, D, c, B, L = tp._system(name, masked, wrap)
                    want = tp._certified(name, masked, wrap, lower, upper)[0]
                    for r in args.ratio:
                        xs, _, _, _ = pc.pd_dense(N, b, D, c, *tp._inf(lower, upper), L, r,
                                                  args.horizon, B)
                        kr = pc.first_stays_under([cc.rel_err(x, want) for x in xs],
                                                  pc.STAYS_UNDER)
                        extra += f'  ratio {r:g}: K {kr}'
                print(f'# {key}: K {k}, radius {radius:.3g}, flat {flat:.2f}, jump {jump:.2f}'
                      f'{extra}', flush=True)
    ks = [v[0] for v in rows.values()]
    print(f'# largest K {max(ks) if None not in ks else None}; errors below are at '
          f'pd_cases.ITERATIONS = {pc.ITERATIONS}')
    print('MEASURED = {')
    for key, (k, at, radius) in rows.items():
        at_s = 'None' if at is None else f'{at:.3g}'
        print(f'    {key!r}: ({k}, {at_s}, {radius:.3g}),')
    print('}')
    if None not in [v[1] for v in rows.values()]:
        print(f'# 100 x the largest error: {100 * max(v[1] for v in rows.values()):.3g}')


if __name__ == '__main__':
    main()
