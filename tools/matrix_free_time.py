#!/usr/bin/env python3
"""Time and memory of the matrix-free pair (MatrixFreeOperator: fused trace + integrate, fused
trace + scatter) beside the stored-trace Operator, on one GPU.

    python tools/matrix_free_time.py [--configs c2 c3] [--out profiles/matrix_free_times.json]
    python tools/matrix_free_time.py --gradient [--configs c2 c3] [--gd-config c5]
                                     [--out profiles/matrix_free_gradient_times.json]
    python tools/matrix_free_time.py --deterministic [--configs c2 c3]
                                     [--out profiles/matrix_free_deterministic_times.json]

Per config (bench.py's CONFIGS) two legs, each in a fresh child process with its own time limit
(a leg that fails or runs out of time ends the run: nothing more is started):
  matrix_free  ms per forward and per back-projection (float32 and float64 calls, HIP events
               around `reps` calls), torch.cuda.max_memory_allocated over one forward plus one
               back-projection, the bytes the operator holds;
  operator     Operator construction + first forward + first op.T (wall clock), its peak and
               resident memory, its segment count, steady forward / T (transposed) / T (float64
               atomics over the stored CSR) per call.
Derived: back-projection against forward (the same trace with atomics against gathers) and the
float64-atomic byte rate that difference implies (segments x 8 B / difference), beside the rate
of the stored CSR's atomic adjoint (segments x 8 B / its time: atomics without the trace).

--gradient measures the fused residual back-projection instead (one leg per config, then one gd
leg; the same child processes and limits):
  gradient     float64, in one process: ms per op(x), per op.T(r) and per
               op.residual_gradient(x, m) (HIP events around `reps` calls, REPEATS times each,
               all kept), torch.cuda.max_memory_allocated over one fused call, the bytes held.
               Derived: the fused call against the sum of the two separate calls (medians), and
               whether the gain exceeds the spread (max - min) of the repeats of either side;
  gd           ms per iteration of gd(..., 100) over a MatrixFreeOperator on bench.py's C5
               retrieval problem, through the fused loop (retrieval._fused_plan) and through the
               autograd loop (the plan function made to return None), REPEATS times each.

--deterministic measures the fixed-point adjoint beside the float64-atomic one (one leg per
config, the same child processes and limits):
  deterministic  float64, in one process: ms per op.T(r) and per op.residual_gradient(x, m) with
               op.deterministic False and True (HIP events around `reps` calls, REPEATS
               interleaved rounds, all kept), and the peak of one fused call in each mode.
               Derived: medians, the ratio of the modes and the spread of the repeats.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_LIMIT_S = 300
REPEATS = 3          # timings of the --gradient legs


def events_ms(fn, reps):
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _problem(config):
    import torch
    import bench
    cfg = bench.CONFIGS[config]
    grid, geom = bench.build_geometry(cfg, 0, 1)
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xs = {dt: torch.rand(cfg[0], dtype=dt, device=dev, generator=g)
          for dt in (torch.float32, torch.float64)}
    ys = {dt: torch.rand(tuple(geom.shape), dtype=dt, device=dev, generator=g)
          for dt in (torch.float32, torch.float64)}
    return grid, geom, dev, xs, ys


def leg_matrix_free(config, reps):
    import torch
    from sph_raytracer_amd import MatrixFreeOperator
    grid, geom, dev, xs, ys = _problem(config)
    ts = dict(time_slices=True) if grid.dynamic else {}
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    op = MatrixFreeOperator(grid, geom, dynamic=grid.dynamic, device=dev)
    rec = {'config': config, 'rays': int(op._parts[1].n), 'reps': reps, 'inputs_bytes': base}
    for dt, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
        x, y = xs[dt], ys[dt]
        op(x), op.T(y, **ts)                                    # warm-up
        torch.cuda.synchronize()
        rec[f'held_bytes_{tag}'] = torch.cuda.memory_allocated(dev) - base
        torch.cuda.reset_peak_memory_stats(dev)
        a, b = op(x), op.T(y, **ts)
        torch.cuda.synchronize()
        # (the peak counts the four input tensors too: inputs_bytes)
        rec[f'peak_bytes_{tag}'] = torch.cuda.max_memory_allocated(dev)
        del a, b
        rec[f'forward_ms_{tag}'] = events_ms(lambda: op(x), reps)
        rec[f'backproject_ms_{tag}'] = events_ms(lambda: op.T(y, **ts), reps)
    return rec


def leg_operator(config, reps):
    import torch
    from sph_raytracer_amd import Operator
    grid, geom, dev, xs, ys = _problem(config)
    ts = dict(time_slices=True) if grid.dynamic else {}
    import bench
    dt = bench.CONFIGS[config][4]
    x, y = xs[dt], ys[dt]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    op = Operator(grid, geom, dynamic=grid.dynamic, device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    a = op(x)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    b = op.T(y, **ts)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    del a, b
    rec = {'config': config, 'dtype': str(dt).split('.')[-1], 'reps': reps,
           'rays': int(op._csr['n']), 'segments': int(op._csr['total']),
           'construct_ms': (t1 - t0) * 1e3, 'first_forward_ms': (t2 - t1) * 1e3,
           'first_T_ms': (t3 - t2) * 1e3, 'construct_forward_T_ms': (t3 - t0) * 1e3,
           'peak_gb_resident': torch.cuda.max_memory_allocated(dev) / 1e9,
           'held_bytes': torch.cuda.memory_allocated(dev) - base}
    op(x), op.T(y, **ts)
    rec['forward_ms'] = events_ms(lambda: op(x), reps)
    rec['T_transposed_ms'] = events_ms(lambda: op.T(y, **ts), reps)
    y64 = ys[torch.float64]
    op.adjoint_mode = 'atomic'
    op.T(y64, **ts)
    rec['T_atomic_f64_ms'] = events_ms(lambda: op.T(y64, **ts), reps)
    return rec


def leg_gradient(config, reps):
    import torch
    from sph_raytracer_amd import MatrixFreeOperator
    grid, geom, dev, xs, ys = _problem(config)
    ts = dict(time_slices=True) if grid.dynamic else {}
    x, m = xs[torch.float64], ys[torch.float64]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    op = MatrixFreeOperator(grid, geom, dynamic=grid.dynamic, device=dev)
    r = 0.5 * (op(x) - m)
    op.T(r, **ts), op.residual_gradient(x, m, 0.5)             # warm-up
    torch.cuda.synchronize()
    rec = {'config': config, 'rays': int(op._parts[1].n), 'reps': reps, 'repeats': REPEATS,
           'dtype': 'float64', 'inputs_bytes': base + r.numel() * r.element_size(),
           'held_bytes': torch.cuda.memory_allocated(dev) - base - r.numel() * r.element_size()}
    torch.cuda.reset_peak_memory_stats(dev)
    a = op.residual_gradient(x, m, 0.5)
    torch.cuda.synchronize()
    # (the peak counts x, m and r too: inputs_bytes)
    rec['fused_peak_bytes'] = torch.cuda.max_memory_allocated(dev)
    del a
    legs = (('forward_ms', lambda: op(x)), ('backproject_ms', lambda: op.T(r, **ts)),
            ('fused_ms', lambda: op.residual_gradient(x, m, 0.5)))
    for name, _ in legs:
        rec[name] = []
    for _ in range(REPEATS):                                   # interleaved: one of each per round
        for name, fn in legs:
            rec[name].append(events_ms(fn, reps))
    return rec


def leg_deterministic(config, reps):
    import torch
    from sph_raytracer_amd import MatrixFreeOperator
    grid, geom, dev, xs, ys = _problem(config)
    ts = dict(time_slices=True) if grid.dynamic else {}
    x, m = xs[torch.float64], ys[torch.float64]
    op = MatrixFreeOperator(grid, geom, dynamic=grid.dynamic, device=dev)
    r = 0.5 * (op(x) - m)
    rec = {'config': config, 'rays': int(op._parts[1].n), 'reps': reps, 'repeats': REPEATS,
           'dtype': 'float64', 'density_elements': x.numel()}
    legs = []
    for det, tag in ((False, 'atomic'), (True, 'deterministic')):
        def back(det=det):
            op.deterministic = det
            return op.T(r, **ts)

        def fused(det=det):
            op.deterministic = det
            return op.residual_gradient(x, m, 0.5)

        back(), fused()                                          # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        a = fused()
        torch.cuda.synchronize()
        rec[f'fused_peak_over_resident_bytes_{tag}'] = torch.cuda.max_memory_allocated(dev) - base
        del a
        legs += [(f'backproject_ms_{tag}', back), (f'fused_ms_{tag}', fused)]
    for name, _ in legs:
        rec[name] = []
    for _ in range(REPEATS):                                   # interleaved: one of each per round
        for name, fn in legs:
            rec[name].append(events_ms(fn, reps))
    return rec


def derive_deterministic(g):
    d = {}
    for what in ('backproject', 'fused'):
        a, f = g[f'{what}_ms_atomic'], g[f'{what}_ms_deterministic']
        d[f'{what}_ms_atomic'], d[f'{what}_ms_deterministic'] = _median(a), _median(f)
        d[f'{what}_deterministic_over_atomic'] = _median(f) / _median(a)
        d[f'{what}_spread_ms'] = max(max(a) - min(a), max(f) - min(f))
    return d


def main_deterministic(args):
    out = {}
    for config in args.configs:
        rec = _child('deterministic', config, args.reps)
        if rec is None:
            return 1
        out[config] = {'deterministic': rec, 'derived': derive_deterministic(rec)}
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')
    print(json.dumps({c: out[c]['derived'] for c in out}))
    return 0


def leg_gd(config, iterations=100):
    import torch
    import bench
    from sph_raytracer_amd import MatrixFreeOperator, retrieval
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom = bench.build_geometry(bench.CONFIGS[config], 0, 1)
    dev = torch.device('cuda', 0)
    truth = torch.zeros(tuple(grid.shape), dtype=torch.float64, device=dev)
    truth[:, 32:, :32] = 1                       # bench.py's C5 retrieval problem
    truth[:, :32, 32:] = 1
    model = FullyDenseModel(grid)
    op = MatrixFreeOperator(grid, geom, device=dev)
    y = op(truth)
    fused_plan = retrieval._fused_plan

    def run(k):
        return retrieval.gd(op, y.clone(), model, num_iterations=k, lr=1e-1,
                            loss_fns=[SquareLoss(), NegRegularizer()], progress_bar=False)

    rec = {'config': config, 'rays': int(op._parts[1].n), 'iterations': iterations,
           'repeats': REPEATS, 'fused_ms_per_iteration': [], 'autograd_ms_per_iteration': []}
    final = {}
    for rnd in range(REPEATS + 1):                             # (round 0 warms up, untimed)
        for name, plan in (('fused', fused_plan), ('autograd', lambda *a, **k: None)):
            retrieval._fused_plan = plan
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, _, losses = run(iterations if rnd else 3)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            finally:
                retrieval._fused_plan = fused_plan
            if rnd:
                rec[f'{name}_ms_per_iteration'].append(dt * 1e3 / iterations)
                final[name] = [v[-1] for v in losses.values()]
    rec['final_losses_fused'], rec['final_losses_autograd'] = final['fused'], final['autograd']
    return rec


def _median(v):
    return sorted(v)[len(v) // 2]


def derive_gradient(g):
    f, b, u = g['forward_ms'], g['backproject_ms'], g['fused_ms']
    pair = [fi + bi for fi, bi in zip(f, b)]
    spread = max(max(pair) - min(pair), max(u) - min(u))
    gain = _median(pair) - _median(u)
    return {'separate_ms': _median(pair), 'fused_ms': _median(u), 'gain_ms': gain,
            'spread_ms': spread, 'fused_over_separate': _median(u) / _median(pair),
            'faster_by_more_than_spread': bool(gain > spread)}


def derive_gd(g):
    f, a = g['fused_ms_per_iteration'], g['autograd_ms_per_iteration']
    spread = max(max(f) - min(f), max(a) - min(a))
    gain = _median(a) - _median(f)
    return {'fused_ms_per_iteration': _median(f), 'autograd_ms_per_iteration': _median(a),
            'gain_ms': gain, 'spread_ms': spread,
            'faster_by_more_than_spread': bool(gain > spread)}


def _child(leg, config, reps):
    """One leg in a fresh process -> its record, or None (reported) when it failed or ran out of
    time: the caller starts nothing more."""
    cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--configs', config]
    if reps:
        cmd += ['--reps', str(reps)]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(f'{config} {leg}: no result within {LEG_LIMIT_S} s; stopping', file=sys.stderr)
        return None
    if res.returncode != 0:
        print(f'{config} {leg}: exit {res.returncode}; stopping\n{res.stderr[-2000:]}',
              file=sys.stderr)
        return None
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    print(f'{config} {leg}: {rec}', file=sys.stderr, flush=True)
    return rec


def main_gradient(args):
    out = {}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')

    for config in args.configs:
        rec = _child('gradient', config, args.reps)
        if rec is None:
            return 1
        out[config] = {'gradient': rec, 'derived': derive_gradient(rec)}
        save()
    rec = _child('gd', args.gd_config, None)
    if rec is None:
        return 1
    out[f'gd_{args.gd_config}'] = {'gd': rec, 'derived': derive_gd(rec)}
    save()
    print(json.dumps({c: out[c]['derived'] for c in out}))
    return 0


def derive(mf, opr):
    seg = opr['segments']
    d = {}
    for tag in ('f32', 'f64'):
        f, b = mf[f'forward_ms_{tag}'], mf[f'backproject_ms_{tag}']
        d[f'backproject_over_forward_{tag}'] = b / f
        d[f'scatter_minus_gather_ms_{tag}'] = b - f
        d[f'implied_atomic_gb_per_s_{tag}'] = seg * 8 / ((b - f) * 1e-3) / 1e9 if b > f else None
    d['csr_atomic_gb_per_s'] = seg * 8 / (opr['T_atomic_f64_ms'] * 1e-3) / 1e9
    d['segment_csr_bytes_at_12'] = seg * 12
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', nargs='+', default=['c2', 'c3'])
    ap.add_argument('--reps', type=int, default=None, help='calls per timing (default: by size)')
    ap.add_argument('--out', default=None,
                    help='default: profiles/matrix_free_times.json, or with --gradient '
                         'profiles/matrix_free_gradient_times.json')
    ap.add_argument('--gradient', action='store_true',
                    help='measure the fused residual back-projection and gd over it instead')
    ap.add_argument('--deterministic', action='store_true',
                    help='measure the fixed-point adjoint beside the float64-atomic one instead')
    ap.add_argument('--gd-config', default='c5', help='the gd leg\'s problem (--gradient)')
    ap.add_argument('--leg', choices=('matrix_free', 'operator', 'gradient', 'gd', 'deterministic'),
                    help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'matrix_free_deterministic_times.json'
                                if args.deterministic else 'matrix_free_gradient_times.json'
                                if args.gradient else 'matrix_free_times.json')
    if args.leg == 'gd':
        print(json.dumps(leg_gd(args.configs[0])))
        return 0
    if args.leg:
        reps = args.reps or (5 if args.configs[0] == 'c3' else 20)
        fn = {'matrix_free': leg_matrix_free, 'operator': leg_operator,
              'gradient': leg_gradient, 'deterministic': leg_deterministic}[args.leg]
        print(json.dumps(fn(args.configs[0], reps)))
        return 0
    if args.deterministic:
        return main_deterministic(args)
    if args.gradient:
        return main_gradient(args)
    out = {}
    for config in args.configs:
        recs = {}
        for leg in ('matrix_free', 'operator'):
            recs[leg] = _child(leg, config, args.reps)
            if recs[leg] is None:
                return 1
        recs['derived'] = derive(recs['matrix_free'], recs['operator'])
        out[config] = recs
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')
    print(json.dumps({c: out[c]['derived'] for c in out}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
