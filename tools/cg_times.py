#!/usr/bin/env python3
"""Per-iteration time of `retrieval.cg` against `gd`'s direct loop at C5 (64^3 grid, 64-view
ConeCirc (100,50) orbit; bench.CONFIGS['c5']), over the stored Operator and over a
MatrixFreeOperator, with the same terms in both solvers: SquareLoss + 0.1 * SmoothRegularizer
(no damping: `gd` has no such term).  Writes profiles/cg_times.json.

    python tools/cg_times.py [--reps 5] [--out profiles/cg_times.json]

What is timed, all in this one process (warm-up calls of every shape first):
  per iteration   whole calls of K = 50 and K = 150 iterations, a host clock around a call that
                  ends in a device synchronise, the three solvers alternating within every
                  repetition; the per-iteration time is (median t(150) - median t(50)) / 100,
                  which leaves out each call's set-up, its last forward and its one readback.
                  `cg` on its direct path, `cg` forced onto its generic (plain torch) path, and
                  `gd` (Adam, lr 0.1) on its direct loop — the code this solver leaves untouched,
                  the yardstick.
  to gd's total   the total J that gd's 100th iterate has (evaluated by the loss classes), the
                  first k at which cg's k-th iterate from the same start is at or under it (J
                  falls monotonically along cg's iterates: bisection over k), and the wall time
                  of that cg call and of gd(100), each a median of whole calls.
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cg_times.json'))
    ap.add_argument('--only', choices=['stored', 'matrix_free'], default=None)
    ap.add_argument('--trace-only', action='store_true',
                    help='run 20 direct cg iterations per operator and exit (for a kernel trace)')
    args = ap.parse_args()
    import bench
    from sph_raytracer_amd import MatrixFreeOperator, Operator, retrieval
    from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
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

    def terms():
        return [SquareLoss(), 0.1 * SmoothRegularizer()]

    def total(op, x):
        with torch.no_grad():
            return float(sum(fn(op, y, x, x) for fn in terms()))

    rec = {'config': 'C5: 64^3 grid, 64-view ConeCirc (100,50) orbit, float64; SquareLoss + 0.1 * '
                     'SmoothRegularizer, start at ones; gd: Adam lr 0.1',
           'method': f'per iteration: (median t({K_HI}) - median t({K_LO})) / {K_HI - K_LO} over '
                     f'{args.reps} repetitions of whole calls, host clock around a synchronised '
                     'call, solvers alternating; one process',
           'operators': {}}
    kinds = [args.only] if args.only else ['stored', 'matrix_free']
    for kind in kinds:
        op = stored if kind == 'stored' else MatrixFreeOperator(grid, geom, device=dev)

        def cg_direct(k):
            assert retrieval._cg_is_direct(op, y, start)
            return retrieval.cg(op, y, loss_fns=terms(), x0=start, num_iterations=k)

        def cg_generic(k):
            keep = retrieval._cg_is_direct
            retrieval._cg_is_direct = lambda *a: False
            try:
                return retrieval.cg(op, y, loss_fns=terms(), x0=start, num_iterations=k)
            finally:
                retrieval._cg_is_direct = keep

        def gd(k):
            c = start.clone().requires_grad_()
            fns = terms()
            plan = retrieval._direct_plan(op, y, model, c, fns, [c]) or \
                retrieval._fused_plan(op, y, model, c, fns, [c])
            assert plan is not None, 'gd would not take its direct loop'
            return retrieval.gd(op, y, model, coeffs=c, num_iterations=k, loss_fns=fns, lr=1e-1,
                                progress_bar=False)

        if args.trace_only:
            cg_direct(20)
            torch.cuda.synchronize()
            continue
        solvers = {'cg_direct': cg_direct, 'cg_generic': cg_generic, 'gd_direct': gd}
        for fn in solvers.values():           # every shape the timed window uses, once
            fn(3)
        times = {name: {K_LO: [], K_HI: []} for name in solvers}
        for _ in range(args.reps):
            for k in (K_LO, K_HI):
                for name, fn in solvers.items():
                    times[name][k].append(timed(lambda: fn(k)))
        out = {}
        for name in solvers:
            lo, hi = (statistics.median(times[name][k]) for k in (K_LO, K_HI))
            out[f'{name}_ms_per_iteration'] = (hi - lo) / (K_HI - K_LO)
            out[f'{name}_call_ms'] = {str(k): sorted(times[name][k]) for k in (K_LO, K_HI)}
        out['cg_direct_over_gd_direct'] = out['cg_direct_ms_per_iteration'] / \
            out['gd_direct_ms_per_iteration']
        out['cg_generic_over_cg_direct'] = out['cg_generic_ms_per_iteration'] / \
            out['cg_direct_ms_per_iteration']
        out['within_1p3x_of_gd'] = out['cg_direct_over_gd_direct'] <= 1.3
        # the total gd(100) ends on, and where cg first reaches it
        c100 = gd(GD_ITERS)[0].detach()
        j_gd = total(op, c100)
        lo, hi = 0, GD_ITERS                  # J(x_lo) > j_gd >= J(x_hi), if cg gets there at all
        j_hi = total(op, cg_direct(hi)[0])
        if total(op, start) <= j_gd:
            hi = 0
        elif j_hi > j_gd:
            hi = None
        else:
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if total(op, cg_direct(mid)[0]) <= j_gd:
                    hi = mid
                else:
                    lo = mid
        out['total_at_start'] = total(op, start)
        out['gd100_total'] = j_gd
        out['cg100_total'] = j_hi
        out['cg_iterations_to_gd100_total'] = hi
        out['gd100_wall_ms'] = statistics.median(timed(lambda: gd(GD_ITERS))
                                                 for _ in range(args.reps))
        if hi is not None:
            out['cg_total_there'] = total(op, cg_direct(hi)[0])
            out['cg_wall_ms_to_gd100_total'] = statistics.median(
                timed(lambda: cg_direct(hi)) for _ in range(args.reps))
        rec['operators'][kind] = out
        print(kind, json.dumps({k: v for k, v in out.items() if not k.endswith('_call_ms')}),
              flush=True)
    if args.trace_only:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
