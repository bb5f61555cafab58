#!/usr/bin/env python3
"""Times of the Poisson fidelity on one GPU, all in this one process.  Writes
profiles/matrix_free_poisson_times.json.

    python tools/poisson_times.py [--reps 20] [--out profiles/matrix_free_poisson_times.json]

  C3 (bench.CONFIGS['c3']: 128^3, 128 views of 128x256 pixels), float64, a fifth of the rays
     masked: MatrixFreeOperator.residual_gradient(loss='poisson') against the two calls (op(x),
     then op.T of the weight formed in torch) and against loss='huber' — atomic and
     deterministic, the legs interleaved, REPEATS rounds of `reps` calls between two events.
     The Poisson call is compared with the Huber call of the same run (its margin: this run's
     own spread over the repeats) and with the medians the parent commit recorded in
     profiles/matrix_free_robust_times.json.  The deterministic Poisson call is two traces by
     design (no bound on its weight before the forward), the deterministic Huber call one.
  C5 (64^3, 64 views): gd per iteration, PoissonLoss + NegRegularizer, the direct loop against
     the autograd loop, over the stored Operator, the MatrixFreeOperator and its deterministic
     form; measurements are counts of 10 x the line integrals of 1 + the bench phantom, the start
     all ones, Adam at lr 0.01 (every density stays positive).
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
REPEATS = 3
HUBER_DELTA = 0.25
EPS = 1e-8


def events_ms(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _spread(*lists):
    return max(max(v) - min(v) for v in lists)


def leg_c3(reps):
    import bench
    from sph_raytracer_amd import MatrixFreeOperator
    cfg = bench.CONFIGS['c3']
    grid, geom = bench.build_geometry(cfg, 0, 1)
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    x = 0.5 + torch.rand(cfg[0], dtype=torch.float64, device=dev, generator=g)
    op = MatrixFreeOperator(grid, geom, device=dev)
    m = torch.poisson(4 * op(x), generator=g)
    w = torch.rand(m.shape, dtype=torch.float64, device=dev, generator=g)
    w[torch.rand(m.shape, device=dev, generator=g) < 0.2] = 0
    rec = {'config': 'c3', 'rays': int(op._parts[1].n), 'reps': reps, 'repeats': REPEATS,
           'dtype': 'float64', 'masked_fraction': float((w == 0).double().mean()),
           'huber_delta': HUBER_DELTA, 'eps': EPS}

    def mode(det, fn):
        def run():
            op.deterministic = det
            return fn()
        return run

    def two_calls():
        ax = op(x)
        rs = w * 0.5
        return ax, op.T(rs + ((-rs) * m) / (ax + EPS))

    legs = []
    for det, tag in ((False, 'atomic'), (True, 'deterministic')):
        legs += [(f'poisson_fused_ms_{tag}', mode(det, lambda: op.residual_gradient(
                      x, m, 0.5, weights=w, loss='poisson', eps=EPS))),
                 (f'poisson_two_calls_ms_{tag}', mode(det, two_calls)),
                 (f'huber_fused_ms_{tag}', mode(det, lambda: op.residual_gradient(
                      x, m, 0.5, weights=w, loss='huber', delta=HUBER_DELTA)))]
    for name, fn in legs:
        fn()                                                     # warm-up
        rec[name] = []
    for _ in range(REPEATS):                                   # interleaved: one of each per round
        for name, fn in legs:
            rec[name].append(events_ms(fn, reps))
    return rec


def derive_c3(g, parent):
    d = {}
    med = statistics.median
    for tag in ('atomic', 'deterministic'):
        p, t, h = (g[f'{k}_ms_{tag}'] for k in ('poisson_fused', 'poisson_two_calls',
                                                 'huber_fused'))
        spread = _spread(p, t, h)
        d[tag] = {'poisson_fused_ms': med(p), 'poisson_two_calls_ms': med(t),
                  'huber_fused_ms': med(h), 'spread_ms': spread,
                  'gain_over_two_calls_ms': med(t) - med(p),
                  'minus_huber_ms': med(p) - med(h),
                  'within_spread_of_huber': bool(med(p) - med(h) <= spread)}
        key = f'huber_fused_ms_{tag}'
        if parent and key in parent:
            d[tag]['parent_huber_fused_ms'] = med(parent[key])
            d[tag]['minus_parent_huber_ms'] = med(p) - med(parent[key])
            d[tag]['huber_minus_parent_huber_ms'] = med(h) - med(parent[key])
    return d


def leg_c5(iterations):
    import bench
    from sph_raytracer_amd import MatrixFreeOperator, Operator, retrieval
    from sph_raytracer_amd.loss import NegRegularizer, PoissonLoss
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom = bench.build_geometry(bench.CONFIGS['c5'], 0, 1)
    dev = torch.device('cuda', 0)
    truth = torch.ones(tuple(grid.shape), dtype=torch.float64, device=dev)
    truth[:, 32:, :32] = 2                       # 1 + bench.py's C5 retrieval phantom
    truth[:, :32, 32:] = 2
    model = FullyDenseModel(grid)
    ops = {'stored': Operator(grid, geom, device=dev),
           'matrix_free': MatrixFreeOperator(grid, geom, device=dev),
           'matrix_free_deterministic': MatrixFreeOperator(grid, geom, device=dev,
                                                           deterministic=True)}
    y = torch.poisson(10 * ops['stored'](truth),
                      generator=torch.Generator(device=dev).manual_seed(0))
    plans = retrieval._direct_plan, retrieval._fused_plan

    def none(*a, **k):
        return None

    rec = {'config': 'c5', 'iterations': iterations, 'repeats': REPEATS, 'eps': EPS, 'lr': 0.01}
    for kind, op in ops.items():
        direct, auto, final = [], [], {}
        for rnd in range(REPEATS + 1):                     # (round 0 warms up, untimed)
            for name, into, (dp, fp) in (('direct', direct, plans),
                                         ('autograd', auto, (none, none))):
                retrieval._direct_plan, retrieval._fused_plan = dp, fp
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    _, _, losses = retrieval.gd(
                        op, y.clone(), model, num_iterations=iterations if rnd else 3, lr=1e-2,
                        loss_fns=[PoissonLoss(eps=EPS), NegRegularizer()], progress_bar=False)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    retrieval._direct_plan, retrieval._fused_plan = plans
                if rnd:
                    into.append(dt * 1e3 / iterations)
                    final[name] = [v[-1] for v in losses.values()]
        rec[f'{kind}_direct_ms_per_iteration'] = direct
        rec[f'{kind}_autograd_ms_per_iteration'] = auto
        rec[f'{kind}_final_losses_direct'] = final['direct']
        rec[f'{kind}_final_losses_autograd'] = final['autograd']
    return rec


def derive_c5(g):
    d = {}
    for kind in ('stored', 'matrix_free', 'matrix_free_deterministic'):
        f, a = g[f'{kind}_direct_ms_per_iteration'], g[f'{kind}_autograd_ms_per_iteration']
        gain = statistics.median(a) - statistics.median(f)
        d[kind] = {'direct_ms_per_iteration': statistics.median(f),
                   'autograd_ms_per_iteration': statistics.median(a), 'gain_ms': gain,
                   'spread_ms': _spread(f, a),
                   'faster_by_more_than_spread': bool(gain > _spread(f, a))}
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles',
                                                  'matrix_free_poisson_times.json'))
    ap.add_argument('--parent', default=os.path.join(ROOT, 'profiles',
                                                     'matrix_free_robust_times.json'),
                    help="the parent commit's record of the Huber call at C3")
    args = ap.parse_args()
    parent = None
    if os.path.exists(args.parent):
        with open(args.parent) as fh:
            parent = json.load(fh).get('c3', {}).get('robust')
    out = {}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')

    rec = leg_c3(args.reps)
    out['c3'] = {'poisson': rec, 'derived': derive_c3(rec, parent)}
    save()
    rec = leg_c5(args.iterations)
    out['gd_c5'] = {'gd_poisson': rec, 'derived': derive_c5(rec)}
    save()
    print(json.dumps({k: v['derived'] for k, v in out.items()}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
