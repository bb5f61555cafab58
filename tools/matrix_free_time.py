#!/usr/bin/env python3
"""Time and memory of the matrix-free pair (MatrixFreeOperator: fused trace + integrate, fused
trace + scatter) beside the stored-trace Operator, on one GPU.

    python tools/matrix_free_time.py [--configs c2 c3] [--out profiles/matrix_free_times.json]

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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matrix_free_times.json'))
    ap.add_argument('--leg', choices=('matrix_free', 'operator'), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        reps = args.reps or (5 if args.configs[0] == 'c3' else 20)
        fn = leg_matrix_free if args.leg == 'matrix_free' else leg_operator
        print(json.dumps(fn(args.configs[0], reps)))
        return 0
    out = {}
    for config in args.configs:
        recs = {}
        for leg in ('matrix_free', 'operator'):
            cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--configs', config]
            if args.reps:
                cmd += ['--reps', str(args.reps)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_LIMIT_S)
            except subprocess.TimeoutExpired:
                print(f'{config} {leg}: no result within {LEG_LIMIT_S} s; stopping',
                      file=sys.stderr)
                return 1
            if res.returncode != 0:
                print(f'{config} {leg}: exit {res.returncode}; stopping\n{res.stderr[-2000:]}',
                      file=sys.stderr)
                return 1
            recs[leg] = json.loads(res.stdout.strip().splitlines()[-1])
            print(f'{config} {leg}: {recs[leg]}', file=sys.stderr, flush=True)
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
