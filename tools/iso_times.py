#!/usr/bin/env python3
"""Per-iteration time of `retrieval.primal_dual` and `retrieval.chambolle_pock` with an
IsoTVRegularizer at C5 (64^3 grid, 64-view ConeCirc (100,50) orbit; bench.CONFIGS['c5']),
lower = 0, over the stored Operator and over a MatrixFreeOperator: primal_dual with SquareLoss +
0.1 * IsoTV and chambolle_pock with AbsLoss + 0.1 * IsoTV, each beside the same solve with
0.1 * SmoothRegularizer(kind='abs') in its place and beside its own plain-torch path, from the same
run.  Writes profiles/iso_times.json.

    python tools/iso_times.py [--reps 5] [--out profiles/iso_times.json]

As tools/pd_times.py times: whole calls of K = 50 and K = 150 iterations, a host clock around a
call that ends in a device synchronise, every leg alternating within every repetition, all in
this one process (warm-up calls of every shape first); the per-iteration time is (median t(150) -
median t(50)) / 100, and the spread recorded with it is that of the repetitions' own differences
t(150) - t(50), as (largest - smallest) / 100.  These are records, not gates: the two iso launches
move the bytes of the abs launches and add one square root and one division per voxel, so parity
is what is expected; the record states the ratio and the spread.  No kernel trace is taken: no
throughput is claimed."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K_LO, K_HI = 50, 150


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'iso_times.json'))
    ap.add_argument('--only', choices=['stored', 'matrix_free'], default=None)
    args = ap.parse_args()
    import bench
    from sph_raytracer_amd import MatrixFreeOperator, Operator, retrieval
    from sph_raytracer_amd.loss import AbsLoss, IsoTVRegularizer, SmoothRegularizer, SquareLoss
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    grid, geom = bench.build_geometry(bench.CONFIGS['c5'], 0, 1)
    stored = Operator(grid, geom, device=dev)
    truth = torch.zeros(grid.shape, dtype=torch.float64, device=dev)   # static_retrieval.py's
    truth[:, 32:, :32] = 1
    truth[:, :32, 32:] = 1
    y = stored(truth).detach()
    start = torch.ones(tuple(grid.shape), dtype=torch.float64, device=dev)

    def tv(iso):
        return 0.1 * (IsoTVRegularizer() if iso else SmoothRegularizer(kind='abs'))

    rec = {'config': 'C5: 64^3 grid, 64-view ConeCirc (100,50) orbit, float64; primal_dual: '
                     'SquareLoss + 0.1 * TV; chambolle_pock: AbsLoss + 0.1 * TV; TV = '
                     "IsoTVRegularizer() or SmoothRegularizer(kind='abs'); lower = 0, start at ones",
           'method': f'per iteration: (median t({K_HI}) - median t({K_LO})) / {K_HI - K_LO} over '
                     f'{args.reps} repetitions of whole calls, host clock around a synchronised '
                     'call, legs alternating; spread: (max - min) of the repetitions\' own '
                     f't({K_HI}) - t({K_LO}), / {K_HI - K_LO}; one process; no kernel trace: no '
                     'throughput is claimed',
           'operators': {}}
    for kind in ([args.only] if args.only else ['stored', 'matrix_free']):
        op = stored if kind == 'stored' else MatrixFreeOperator(grid, geom, device=dev)
        L = retrieval.primal_dual(op, y, [SquareLoss(), tv(True)], x0=start,
                                  num_iterations=1)[2]['lipschitz']
        norm = retrieval.chambolle_pock(op, y, [AbsLoss(), tv(True)], x0=start,
                                        num_iterations=1)[2]['norm']

        def pd(k, iso):
            return retrieval.primal_dual(op, y, [SquareLoss(), tv(iso)], x0=start,
                                         num_iterations=k, lipschitz=L)

        def cp(k, iso):
            return retrieval.chambolle_pock(op, y, [AbsLoss(), tv(iso)], x0=start,
                                            num_iterations=k, norm=norm)

        def generic(fn):
            def run(k):
                keep = retrieval._cg_is_direct
                retrieval._cg_is_direct = lambda *a: False
                try:
                    return fn(k, True)
                finally:
                    retrieval._cg_is_direct = keep
            return run

        assert retrieval._cg_is_direct(op, y, start)
        legs = {'pd_iso': lambda k: pd(k, True), 'pd_abs': lambda k: pd(k, False),
                'pd_iso_generic': generic(pd), 'cp_iso': lambda k: cp(k, True),
                'cp_abs': lambda k: cp(k, False), 'cp_iso_generic': generic(cp)}
        for fn in legs.values():           # every shape the timed window uses, once
            fn(3)
        times = {name: {K_LO: [], K_HI: []} for name in legs}
        for _ in range(args.reps):
            for k in (K_LO, K_HI):
                for name, fn in legs.items():
                    times[name][k].append(timed(lambda: fn(k)))
        out = {'lipschitz': L, 'norm': norm}
        for name in legs:
            lo, hi = (statistics.median(times[name][k]) for k in (K_LO, K_HI))
            diffs = [b - a for a, b in zip(times[name][K_LO], times[name][K_HI])]
            out[f'{name}_ms_per_iteration'] = (hi - lo) / (K_HI - K_LO)
            out[f'{name}_spread_ms_per_iteration'] = (max(diffs) - min(diffs)) / (K_HI - K_LO)
            out[f'{name}_call_ms'] = {str(k): sorted(times[name][k]) for k in (K_LO, K_HI)}
        for s in ('pd', 'cp'):
            out[f'{s}_iso_over_abs'] = out[f'{s}_iso_ms_per_iteration'] / \
                out[f'{s}_abs_ms_per_iteration']
            out[f'{s}_generic_over_direct'] = out[f'{s}_iso_generic_ms_per_iteration'] / \
                out[f'{s}_iso_ms_per_iteration']
        rec['operators'][kind] = out
        print(kind, json.dumps({k: v for k, v in out.items() if not k.endswith('_call_ms')}),
              flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
