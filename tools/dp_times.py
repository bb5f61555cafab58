#!/usr/bin/env python3
"""`retrieval.chambolle_pock` with precondition='diagonal' beside precondition=None at C5 (64^3
grid, 64-view ConeCirc (100,50) orbit; bench.CONFIGS['c5']) with lower = 0, for AbsLoss + 0.1 *
SmoothRegularizer(kind='abs') and for PoissonLoss + the same TV term, over the stored Operator and
over a MatrixFreeOperator.  Writes profiles/dp_times.json.

    python tools/dp_times.py [--reps 5] [--out profiles/dp_times.json]

What is recorded, all in this one process (warm-up calls of every shape first), timed as
tools/cp_times.py times:
  per iteration   whole calls of K = 50 and K = 150 iterations, a host clock around a call that
                  ends in a device synchronise, the two variants alternating within every
                  repetition; per repetition (t(150) - t(50)) / 100, which leaves out each call's
                  set-up, its last forward and its one readback; the median of the repetitions
                  and their spread (largest - smallest) per variant.
  set-up          whole calls of K = 0 iterations: 'diagonal' forms its steps from one forward and
                  one adjoint of ones and one sphrt_dp_steps_f64 launch, None runs the power
                  method (ten forward and adjoint pairs); median of the repetitions.
  the total J     of the same terms (evaluated by the loss classes) at the k-th iterate, k = 0,
                  50, ..., --horizon, for both variants; the total gd(100) ends on (with a
                  NegRegularizer: gd has no bounds) as profiles/cp_times.json records it, and the
                  first sample of each variant at or under it (None: not within the horizon).
These are records, not gates: whether the preconditioned iteration converges in fewer iterations
here is what the record is for."""
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
K_LO, K_HI, GD_ITERS, STEP = 50, 150, 100, 50
VARIANTS = {'diagonal': 'diagonal', 'none': None}


def main():
    from pd_times import timed
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--horizon', type=int, default=400)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dp_times.json'))
    ap.add_argument('--only', choices=['stored', 'matrix_free'], default=None)
    args = ap.parse_args()
    import bench
    from sph_raytracer_amd import MatrixFreeOperator, Operator, retrieval
    from sph_raytracer_amd.loss import AbsLoss, NegRegularizer, PoissonLoss, SmoothRegularizer
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
    TERMS = {'abs_tv': lambda: [AbsLoss(), tv()], 'poisson_tv': lambda: [PoissonLoss(), tv()]}

    rec = {'config': 'C5: 64^3 grid, 64-view ConeCirc (100,50) orbit, float64; lower = 0, the '
                     "default dual_ratio, start at ones; abs_tv: AbsLoss + 0.1 * SmoothRegularizer("
                     "kind='abs'); poisson_tv: PoissonLoss + the same TV term; gd: Adam lr 0.1 "
                     'with a NegRegularizer',
           'method': f'per iteration: (t({K_HI}) - t({K_LO})) / {K_HI - K_LO} per repetition of '
                     f'whole calls, median and spread over {args.reps} repetitions, host clock '
                     'around a synchronised call, the variants alternating; set-up: whole calls '
                     'of 0 iterations; one process',
           'operators': {}}
    for kind in ([args.only] if args.only else ['stored', 'matrix_free']):
        op = stored if kind == 'stored' else MatrixFreeOperator(grid, geom, device=dev)

        def solve(k, which, variant):
            assert retrieval._cg_is_direct(op, y, start)
            return retrieval.chambolle_pock(op, y, TERMS[which](), x0=start, num_iterations=k,
                                            precondition=VARIANTS[variant])

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

        out = {}
        info = solve(1, 'abs_tv', 'diagonal')[2]
        tau, sigma = info['tau'], info['sigma']
        live_t, live_s = tau[tau > 0], sigma[sigma > 0]
        out['steps'] = {'tau_min': float(live_t.min()), 'tau_max': float(live_t.max()),
                        'tau_zero': int((tau == 0).sum()), 'sigma_min': float(live_s.min()),
                        'sigma_max': float(live_s.max()), 'sigma_zero': int((sigma == 0).sum()),
                        'sigma_tv': info['sigma_tv']}
        scalar = solve(1, 'abs_tv', 'none')[2]
        out['scalar_steps'] = {'norm': scalar['norm'], 'tau': scalar['tau'],
                               'sigma': scalar['sigma']}
        for which in TERMS:
            for variant in VARIANTS:          # every shape the timed window uses, once
                solve(3, which, variant)
            times = {v: {0: [], K_LO: [], K_HI: []} for v in VARIANTS}
            for _ in range(args.reps):
                for k in (0, K_LO, K_HI):
                    for variant in VARIANTS:
                        times[variant][k].append(
                            timed(lambda k=k, variant=variant: solve(k, which, variant)))
            w = {}
            for variant in VARIANTS:
                per = [(hi - lo) / (K_HI - K_LO)
                       for lo, hi in zip(times[variant][K_LO], times[variant][K_HI])]
                w[f'{variant}_ms_per_iteration'] = statistics.median(per)
                w[f'{variant}_ms_per_iteration_spread'] = max(per) - min(per)
                w[f'{variant}_ms_per_iteration_reps'] = per
                w[f'{variant}_setup_ms'] = statistics.median(times[variant][0])
                w[f'{variant}_call_ms'] = {str(k): times[variant][k] for k in (0, K_LO, K_HI)}
            diff = abs(w['diagonal_ms_per_iteration'] - w['none_ms_per_iteration'])
            w['per_iteration_difference_ms'] = diff
            w['difference_within_the_spread_of_none'] = diff <= w['none_ms_per_iteration_spread']
            # the totals along the iteration, and gd(100)'s
            j_gd = total(which, gd(GD_ITERS, which)[0].detach())
            w['total_at_start'] = total(which, start)
            w['gd100_total'] = j_gd
            for variant in VARIANTS:
                ks = list(range(0, args.horizon + 1, STEP))
                totals = [total(which, solve(k, which, variant)[0]) for k in ks]
                w[f'{variant}_totals'] = {str(k): v for k, v in zip(ks, totals)}
                w[f'{variant}_iterations_to_gd100_total'] = next(
                    (k for k, v in zip(ks, totals) if v <= j_gd), None)      # (to the step: 50)
            out[which] = w
            print(kind, which, json.dumps({k: v for k, v in w.items()
                                           if not k.endswith(('_call_ms', '_reps'))}), flush=True)
        rec['operators'][kind] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def finite(v):
        """JSON has no NaN: a total that is not finite is recorded as null."""
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
