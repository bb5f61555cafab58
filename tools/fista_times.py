#!/usr/bin/env python3
"""Per-iteration time of `retrieval.fista` at C5 (64^3 grid, 64-view ConeCirc (100,50) orbit;
bench.CONFIGS['c5']) with SquareLoss + 0.1 * SmoothRegularizer and lower = 0, over the stored
Operator and over a MatrixFreeOperator, beside `cg`, `gd`'s direct loop and `fista`'s generic
path from the same run.  Writes profiles/fista_times.json.

    python tools/fista_times.py [--reps 5] [--out profiles/fista_times.json]

What is timed, all in this one process (warm-up calls of every shape first):
  per iteration   whole calls of K = 50 and K = 150 iterations, a host clock around a call that
                  ends in a device synchronise, the solvers alternating within every repetition;
                  the per-iteration time is (median t(150) - median t(50)) / 100, which leaves
                  out each call's set-up (the power iterations among it), its last forward and
                  its one readback.
  power method    median t(fista, K = 50, lipschitz=None) - median t(fista, K = 50, lipschitz
                  given): the one-time cost of the default step-size estimate.
  to gd's total   the total J + NegRegularizer that gd(100) with a NegRegularizer ends on
                  (evaluated by the loss classes), and the first k at which fista's k-th iterate
                  (non-negative, so its NegRegularizer term is zero) is at or under it.
"""
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fista_times.json'))
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

    def terms(neg=False):
        return [SquareLoss(), 0.1 * SmoothRegularizer()] + ([NegRegularizer()] if neg else [])

    def total(op, x):
        with torch.no_grad():
            return float(sum(fn(op, y, x, x) for fn in terms(neg=True)))

    rec = {'config': 'C5: 64^3 grid, 64-view ConeCirc (100,50) orbit, float64; SquareLoss + 0.1 * '
                     'SmoothRegularizer, lower = 0, start at ones; gd: Adam lr 0.1',
           'method': f'per iteration: (median t({K_HI}) - median t({K_LO})) / {K_HI - K_LO} over '
                     f'{args.reps} repetitions of whole calls, host clock around a synchronised '
                     'call, solvers alternating; one process',
           'operators': {}}
    for kind in ([args.only] if args.only else ['stored', 'matrix_free']):
        op = stored if kind == 'stored' else MatrixFreeOperator(grid, geom, device=dev)
        L = retrieval.fista(op, y, loss_fns=terms(), x0=start, num_iterations=1)[2]['lipschitz']

        def fista_direct(k, lipschitz=L):
            assert retrieval._cg_is_direct(op, y, start)
            return retrieval.fista(op, y, loss_fns=terms(), x0=start, num_iterations=k,
                                   lipschitz=lipschitz)

        def fista_generic(k):
            keep = retrieval._cg_is_direct
            retrieval._cg_is_direct = lambda *a: False
            try:
                return retrieval.fista(op, y, loss_fns=terms(), x0=start, num_iterations=k,
                                       lipschitz=L)
            finally:
                retrieval._cg_is_direct = keep

        def cg_direct(k):
            return retrieval.cg(op, y, loss_fns=terms(), x0=start, num_iterations=k)

        def gd(k, neg=False):
            c = start.clone().requires_grad_()
            fns = terms(neg)
            plan = retrieval._direct_plan(op, y, model, c, fns, [c]) or \
                retrieval._fused_plan(op, y, model, c, fns, [c])
            assert plan is not None, 'gd would not take its direct loop'
            return retrieval.gd(op, y, model, coeffs=c, num_iterations=k, loss_fns=fns, lr=1e-1,
                                progress_bar=False)

        solvers = {'fista_direct': fista_direct, 'fista_generic': fista_generic,
                   'cg_direct': cg_direct, 'gd_direct': gd}
        for fn in solvers.values():           # every shape the timed window uses, once
            fn(3)
        fista_direct(3, None)
        times = {name: {K_LO: [], K_HI: []} for name in solvers}
        power = []
        for _ in range(args.reps):
            for k in (K_LO, K_HI):
                for name, fn in solvers.items():
                    times[name][k].append(timed(lambda: fn(k)))
            power.append(timed(lambda: fista_direct(K_LO, None)))
        out = {'lipschitz': L}
        for name in solvers:
            lo, hi = (statistics.median(times[name][k]) for k in (K_LO, K_HI))
            out[f'{name}_ms_per_iteration'] = (hi - lo) / (K_HI - K_LO)
            out[f'{name}_call_ms'] = {str(k): sorted(times[name][k]) for k in (K_LO, K_HI)}
        out['fista_direct_over_cg_direct'] = out['fista_direct_ms_per_iteration'] / \
            out['cg_direct_ms_per_iteration']
        out['fista_direct_over_gd_direct'] = out['fista_direct_ms_per_iteration'] / \
            out['gd_direct_ms_per_iteration']
        out['fista_generic_over_fista_direct'] = out['fista_generic_ms_per_iteration'] / \
            out['fista_direct_ms_per_iteration']
        out['power_iterations'] = retrieval._FISTA_POWER_ITERATIONS
        out['power_iterations_ms'] = statistics.median(power) - \
            statistics.median(times['fista_direct'][K_LO])
        out['power_call_ms'] = sorted(power)
        # the total gd(100) with a NegRegularizer ends on, and where fista first reaches it
        j_gd = total(op, gd(GD_ITERS, neg=True)[0].detach())
        totals = [total(op, fista_direct(k)[0]) for k in range(GD_ITERS + 1)]
        out['total_at_start'] = total(op, start)
        out['gd100_total'] = j_gd
        out['fista100_total'] = totals[-1]
        out['fista_iterations_to_gd100_total'] = next(
            (k for k, v in enumerate(totals) if v <= j_gd), None)
        rec['operators'][kind] = out
        print(kind, json.dumps({k: v for k, v in out.items() if not k.endswith('_call_ms')}),
              flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
