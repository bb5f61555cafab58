#!/usr/bin/env python3
"""The CPU study behind the constants of tests/cp_cases.py and the default dual_ratio of
retrieval.chambolle_pock, on the solver tests' problems — the loss classes over the oracle-backed
CpuOperator (tests/cpu_operator.py), the generic path of the solver itself:

  ratio        for each candidate dual_ratio, the relative duality gap (J - D) / |J| of every
               case of cp_cases.solver_cases after cp_cases.ITERATIONS iterations, J and D
               recomputed from the dense matrix (cp_cases.gap_of): the worst and the geometric
               mean per ratio (DESIGN §5's table);
  measured     the MEASURED table of cp_cases.py at the default ratio, and 100 x its maximum;
  prox         PROX_MEASURED: the largest violation of p in d phi(z) that `_cp_prox` shows;
  sensitivity  SENSITIVITY: the CPU reference against the matrix with its sums reversed.

    python tools/cp_study.py [--ratio R ...] [--measured] [--prox] [--sensitivity]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import numpy as np
    import torch as tr

    import cp_cases as cp
    from sph_raytracer_amd import retrieval
    ap = argparse.ArgumentParser()
    ap.add_argument('--ratio', type=float, nargs='*', default=[])
    ap.add_argument('--measured', action='store_true')
    ap.add_argument('--prox', action='store_true')
    ap.add_argument('--sensitivity', action='store_true')
    args = ap.parse_args()
    cases = cp.solver_cases()
    for r in args.ratio:
        gaps = [cp.gap_of(case, *cp.solve_case(case, dual_ratio=r)[::2])[2] for case in cases]
        worst = int(np.argmax(gaps))
        print(f'# ratio {r:g}: worst gap {max(gaps):.3g} ({cp.case_id(cases[worst])}), '
              f'geometric mean {math.exp(np.mean(np.log(np.maximum(gaps, 1e-17)))):.3g}',
              flush=True)
    if args.measured:
        print(f'# dual_ratio {retrieval._CP_DUAL_RATIO:g}, {cp.ITERATIONS} iterations')
        print('MEASURED = {')
        worst = 0.0
        for case in cases:
            x, _, info = cp.solve_case(case)
            J, D, gap = cp.gap_of(case, x, info)
            assert D <= J + cp.WEAK_DUALITY_SLACK * abs(J), (cp.case_id(case), J, D)
            worst = max(worst, gap)
            print(f'    {cp.case_id(case)!r}: {gap:.3g},', flush=True)
        print('}')
        print(f'# 100 x the largest gap: {100 * worst:.3g}')
    if args.prox:
        out = {}
        for kind in cp.KINDS:
            a, sg, s, y = cp.prox_draws(kind)
            p = retrieval._cp_prox(cp.KIND_ID[kind], cp.par_of(kind), *(tr.from_numpy(v) for v in
                                                                       (a, sg, s, y))).numpy()
            out[kind] = float(cp.prox_violation(kind, a, sg, s, y, p).max())
        print('PROX_MEASURED = {' + ', '.join(f'{k!r}: {v:.2e}' for k, v in out.items()) + '}')
    if args.sensitivity:
        print('SENSITIVITY = {')
        for cfg in cp.gpu_cases():
            d = cp.sensitivity(cfg)
            print(f'    {cfg!r}: ({d[0]:.2e}, {d[1]:.2e}, {d[2]:.2e}),', flush=True)
        print('}')


if __name__ == '__main__':
    main()
