#!/usr/bin/env python3
"""Per-iteration time of `retrieval.chambolle_pock` at C5 (64^3 grid, 64-view ConeCirc (100,50)
orbit; bench.CONFIGS['c5']) with lower = 0, for AbsLoss + 0.1 * SmoothRegularizer(kind='abs') and
for PoissonLoss alone, over the stored Operator and over a MatrixFreeOperator, beside its generic
(plain torch) path and `primal_dual` (SquareLoss + the same TV term) from the same run.  Writes
profiles/cp_times.json.

    python tools/cp_times.py [--reps 5] [--out profiles/cp_times.json]

What is timed, all in this one process (warm-up calls of every shape first), as tools/pd_times.py
times:
  per iteration   whole calls of K = 50 and K = 150 iterations, a host clock around a call that
                  ends in a device synchronise, the solvers alternating within every repetition;
                  the per-iteration time is (median t(150) - median t(50)) / 100, which leaves
                  out each call's set-up (the power iterations among it), its last forward and
                  its one readback.
  to gd's total   the total of the same terms (evaluated by the loss classes, plus a
                  NegRegularizer for gd, which has no bounds) that gd(100) ends on, and the first
                  k at which chambolle_pock's k-th iterate (non-negative: its NegRegularizer term
                  is zero) is at or under it, k up to --horizon (None: not within it).
These are records, not gates.  If the direct path is not faster than the generic one, the record
says so ('direct_faster_than_generic')."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
K_LO, K_HI, GD_ITERS = 50, 150, 100


def main():
    from pd_times import timed
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--horizon', type=int, default=400)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cp_times.json'))
    ap.add_argument('--only', choices=['stored', 'matrix_free'], default=None)
    args = ap.parse_args()
    import bench
    from sph_raytracer_amd import MatrixFreeOperator, Operator, retrieval
    from sph_raytracer_amd.loss import (AbsLoss, NegRegularizer, PoissonLoss, SmoothRegularizer,
                                        SquareLoss)
    from sph_raytracer_amd.model import FullyDenseModel
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    grid, geom = bench.build_geometry(bench.CONFIGS['c5'], 0, 1)
    stored = Operator(grid, geom, device=dev)
    truth = torch.zeros(grid.shape, dtype=torch.float64, device=dev)   # static_retrieval.py's
    truth[:, 32:, :32] = 1
    truth[:, :32, 32:] = 1
    y = stored(truth).detach()
    model = FullyDenseModel(grid)
    start = torch.ones(tuple(grid.shape), dtype=torch.float64, device=dev)
    tv = lambda: 0.1 * SmoothRegularizer(kind='abs')                   # noqa: E731
    TERMS = {'abs_tv': lambda: [AbsLoss(), tv()], 'poisson': lambda: [PoissonLoss()]}

    rec = {'config': 'C5: 64^3 grid, 64-view ConeCirc (100,50) orbit, float64; lower = 0, the '
                     "default dual_ratio, start at ones; abs_tv: AbsLoss + 0.1 * SmoothRegularizer("
                     "kind='abs'); poisson: PoissonLoss; primal_dual: SquareLoss + the same TV "
                     'term; gd: Adam lr 0.1 with a NegRegularizer',
           'method': f'per iteration: (median t({K_HI}) - median t({K_LO})) / {K_HI - K_LO} over '
                     f'{args.reps} repetitions of whole calls, host clock around a synchronised '
                     'call, solvers alternating; one process',
           'operators': {}}
    for kind in ([args.only] if args.only else ['stored', 'matrix_free']):
        op = stored if kind == 'stored' else MatrixFreeOperator(grid, geom, device=dev)
        norm = retrieval.chambolle_pock(op, y, [AbsLoss()], x0=start, num_iterations=1)[2]['norm']
        L = retrieval.primal_dual(op, y, [SquareLoss(), tv()], x0=start,
                                  num_iterations=1)[2]['lipschitz']

        def cp_direct(k, which):
            assert retrieval._cg_is_direct(op, y, start)
            return retrieval.chambolle_pock(op, y, TERMS[which](), x0=start, num_iterations=k,
                                            norm=norm)

        def cp_generic(k, which):
            keep = retrieval._cg_is_direct
            retrieval._cg_is_direct = lambda *a: False
            try:
                return retrieval.chambolle_pock(op, y, TERMS[which](), x0=start, num_iterations=k,
                                                norm=norm)
            finally:
                retrieval._cg_is_direct = keep

        def pd_direct(k):
            return retrieval.primal_dual(op, y, [SquareLoss(), tv()], x0=start, num_iterations=k,
                                         lipschitz=L)

        def gd(k, which):
            c = start.clone().requires_grad_()
            fns = TERMS[which]() + [NegRegularizer()]
            plan = retrieval._direct_plan(op, y, model, c, fns, [c]) or \
                retrieval._fused_plan(op, y, model, c, fns, [c])
            assert plan is not None, 'gd would not take its direct loop'
            return retrieval.gd(op, y, model, coeffs=c, num_iterations=k, loss_fns=fns, lr=1e-1,
                                progress_bar=False)

        def total(which, x):
            with torch.no_grad():
                return float(sum(fn(op, y, x, x) for fn in TERMS[which]() + [NegRegularizer()]))

        solvers = {'pd_direct': pd_direct}
        for which in TERMS:
            solvers[f'cp_{which}_direct'] = lambda k, w=which: cp_direct(k, w)
            solvers[f'cp_{which}_generic'] = lambda k, w=which: cp_generic(k, w)
        for fn in solvers.values():           # every shape the timed window uses, once
            fn(3)
        times = {name: {K_LO: [], K_HI: []} for name in solvers}
        for _ in range(args.reps):
            for k in (K_LO, K_HI):
                for name, fn in solvers.items():
                    times[name][k].append(timed(lambda: fn(k)))
        out = {'norm': norm, 'lipschitz': L}
        for name in solvers:
            lo, hi = (statistics.median(times[name][k]) for k in (K_LO, K_HI))
            out[f'{name}_ms_per_iteration'] = (hi - lo) / (K_HI - K_LO)
            out[f'{name}_call_ms'] = {str(k): sorted(times[name][k]) for k in (K_LO, K_HI)}
        for which in TERMS:
            d, g = (out[f'cp_{which}_{p}_ms_per_iteration'] for p in ('direct', 'generic'))
            out[f'cp_{which}_generic_over_direct'] = g / d
            out[f'cp_{which}_direct_over_pd_direct'] = d / out['pd_direct_ms_per_iteration']
            out[f'cp_{which}_direct_faster_than_generic'] = d < g
            # the total gd(100) ends on, and where chambolle_pock first reaches it
            j_gd = total(which, gd(GD_ITERS, which)[0].detach())
            out[f'{which}_total_at_start'] = total(which, start)
            out[f'{which}_gd100_total'] = j_gd
            reached, k_total = None, None
            for k in list(range(0, GD_ITERS + 1, 10)) + list(range(GD_ITERS + 50, args.horizon + 1,
                                                                  50)):
                k_total = total(which, cp_direct(k, which)[0])
                if k == GD_ITERS:
                    out[f'{which}_cp100_total'] = k_total
                if reached is None and k_total <= j_gd:
                    reached = k
            out[f'{which}_cp_total_at_horizon'] = {'iterations': args.horizon, 'total': k_total}
            out[f'{which}_cp_iterations_to_gd100_total'] = reached   # (to the step: 10, then 50)
        rec['operators'][kind] = out
        print(kind, json.dumps({k: v for k, v in out.items() if not k.endswith('_call_ms')}),
              flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def finite(v):
        """JSON has no NaN: a total that is not finite (gd diverged) is recorded as null."""
        if isinstance(v, dict):
            return {k: finite(u) for k, u in v.items()}
        if isinstance(v, list):
            return [finite(u) for u in v]
        return None if isinstance(v, float) and not math.isfinite(v) else v
    with open(args.out, 'w') as f:
        json.dump(finite(rec), f, indent=1, allow_nan=False)
        f.write('\n')


if __name__ == '__main__':
    main()
