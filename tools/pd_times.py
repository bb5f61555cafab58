#!/usr/bin/env python3
"""Per-iteration time of `retrieval.primal_dual` at C5 (64^3 grid, 64-view ConeCirc (100,50)
orbit; bench.CONFIGS['c5']) with SquareLoss + 0.1 * SmoothRegularizer(kind='abs') and lower = 0,
over the stored Operator and over a MatrixFreeOperator, beside its generic path and `fista` with
the same terms but kind='square', from the same run.  Writes profiles/pd_times.json.

    python tools/pd_times.py [--reps 5] [--out profiles/pd_times.json]

What is timed, all in this one process (warm-up calls of every shape first), as
tools/fista_times.py times:
  per iteration   whole calls of K = 50 and K = 150 iterations, a host clock around a call that
                  ends in a device synchronise, the solvers alternating within every repetition;
                  the per-iteration time is (median t(150) - median t(50)) / 100, which leaves
                  out each call's set-up (the power iterations among it), its last forward and
                  its one readback.
  to gd's total   the total (SquareLoss + 0.1 * abs smoothness + NegRegularizer, evaluated by the
                  loss classes) that gd(100) with a NegRegularizer ends on, and the first k at
                  which primal_dual's k-th iterate (non-negative, so its NegRegularizer term is
                  zero) is at or under it, k up to --horizon (None: not within it).
These are records, not gates.  If the direct path is not faster than the generic one, the record
says so ('direct_faster_than_generic')."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K_LO, K_HI, GD_ITERS = 50, 150, 100


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--horizon', type=int, default=400)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pd_times.json'))
    ap.add_argument('--only', choices=['stored', 'matrix_free'], default=None)
    args = ap.parse_args()
    import bench
    from sph_raytracer_amd import MatrixFreeOperator, Operator, retrieval
    from sph_raytracer_amd.loss import NegRegularizer, SmoothRegularizer, SquareLoss
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

    def terms(kind='abs', neg=False):
        return [SquareLoss(), 0.1 * SmoothRegularizer(kind=kind)] + \
            ([NegRegularizer()] if neg else [])

    def total(op, x):
        with torch.no_grad():
            return float(sum(fn(op, y, x, x) for fn in terms(neg=True)))

    rec = {'config': 'C5: 64^3 grid, 64-view ConeCirc (100,50) orbit, float64; SquareLoss + 0.1 * '
                     "SmoothRegularizer(kind='abs'), lower = 0, dual_ratio = 1, start at ones; "
                     "fista: the same with kind='square'; gd: Adam lr 0.1",
           'method': f'per iteration: (median t({K_HI}) - median t({K_LO})) / {K_HI - K_LO} over '
                     f'{args.reps} repetitions of whole calls, host clock around a synchronised '
                     'call, solvers alternating; one process',
           'operators': {}}
    for kind in ([args.only] if args.only else ['stored', 'matrix_free']):
        op = stored if kind == 'stored' else MatrixFreeOperator(grid, geom, device=dev)
        L = retrieval.primal_dual(op, y, terms(), x0=start, num_iterations=1)[2]['lipschitz']

        def pd_direct(k):
            assert retrieval._cg_is_direct(op, y, start)
            return retrieval.primal_dual(op, y, terms(), x0=start, num_iterations=k, lipschitz=L)

        def pd_generic(k):
            keep = retrieval._cg_is_direct
            retrieval._cg_is_direct = lambda *a: False
            try:
                return retrieval.primal_dual(op, y, terms(), x0=start, num_iterations=k,
                                             lipschitz=L)
            finally:
                retrieval._cg_is_direct = keep

        def fista_direct(k):
            return retrieval.fista(op, y, loss_fns=terms('square'), x0=start, num_iterations=k,
                                   lipschitz=L)

        def gd(k, neg=False):
            c = start.clone().requires_grad_()
            fns = terms(neg=neg)
            plan = retrieval._direct_plan(op, y, model, c, fns, [c]) or \
                retrieval._fused_plan(op, y, model, c, fns, [c])
            assert plan is not None, 'gd would not take its direct loop'
            return retrieval.gd(op, y, model, coeffs=c, num_iterations=k, loss_fns=fns, lr=1e-1,
                                progress_bar=False)

        solvers = {'pd_direct': pd_direct, 'pd_generic': pd_generic, 'fista_direct': fista_direct}
        for fn in solvers.values():           # every shape the timed window uses, once
            fn(3)
        times = {name: {K_LO: [], K_HI: []} for name in solvers}
        for _ in range(args.reps):
            for k in (K_LO, K_HI):
                for name, fn in solvers.items():
                    times[name][k].append(timed(lambda: fn(k)))
        out = {'lipschitz': L}
        for name in solvers:
            lo, hi = (statistics.median(times[name][k]) for k in (K_LO, K_HI))
            out[f'{name}_ms_per_iteration'] = (hi - lo) / (K_HI - K_LO)
            out[f'{name}_call_ms'] = {str(k): sorted(times[name][k]) for k in (K_LO, K_HI)}
        out['pd_direct_over_fista_direct'] = out['pd_direct_ms_per_iteration'] / \
            out['fista_direct_ms_per_iteration']
        out['pd_generic_over_pd_direct'] = out['pd_generic_ms_per_iteration'] / \
            out['pd_direct_ms_per_iteration']
        out['direct_faster_than_generic'] = out['pd_direct_ms_per_iteration'] < \
            out['pd_generic_ms_per_iteration']
        # the total gd(100) with a NegRegularizer ends on, and where primal_dual first reaches it
        j_gd = total(op, gd(GD_ITERS, neg=True)[0].detach())
        out['total_at_start'] = total(op, start)
        out['gd100_total'] = j_gd
        reached, k_total = None, None
        for k in list(range(0, GD_ITERS + 1, 5)) + list(range(GD_ITERS + 25, args.horizon + 1, 25)):
            k_total = total(op, pd_direct(k)[0])
            if k == GD_ITERS:
                out['pd100_total'] = k_total
            if reached is None and k_total <= j_gd:
                reached = k
        out['pd_total_at_horizon'] = {'iterations': args.horizon, 'total': k_total}
        out['pd_iterations_to_gd100_total'] = reached    # (to the sampling step: 5, then 25)
        rec['operators'][kind] = out
        print(kind, json.dumps({k: v for k, v in out.items() if not k.endswith('_call_ms')}),
              flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
