#!/usr/bin/env python3
"""Time and memory of the matrix-free pair (MatrixFreeOperator: fused trace + integrate, fused
trace + scatter) beside the stored-trace Operator, on one GPU.

    python tools/matrix_free_time.py [--configs c2 c3] [--out profiles/matrix_free_times.json]
    python tools/matrix_free_time.py --gradient [--configs c2 c3] [--gd-config c5]
                                     [--out profiles/matrix_free_gradient_times.json]
    python tools/matrix_free_time.py --deterministic [--configs c2 c3]
                                     [--out profiles/matrix_free_deterministic_times.json]
    python tools/matrix_free_time.py --weighted [--configs c3] [--gd-config c5] [--base DIR]
                                     [--out profiles/matrix_free_weighted_times.json]
    python tools/matrix_free_time.py --robust [--configs c3] [--gd-config c5] [--base DIR]
                                     [--gd-only] [--out profiles/matrix_free_robust_times.json]

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

--weighted measures weighted least squares (one leg per config, then one gd leg; the same child
processes and limits):
  weighted     float64, in one process, interleaved rounds: ms per unweighted
               op.residual_gradient(x, m, s), per weighted call
               op.residual_gradient(x, m, s, weights=w) with op.deterministic False and True, and
               per two-call path it replaces, op(x) then op.T(w * s * (op(x) - m)), in both modes.
               With --base DIR (a checkout of the parent commit with its library built), that
               tree's own --leg gradient runs in child processes before and after: the unweighted
               call there, the same box and session.  Derived: the unweighted call here against
               the parent's repeats and their spread; the weighted call against the two calls;
  gd_masked    ms per iteration of gd(..., 100) on bench.py's C5 retrieval problem with
               SquareLoss(projection_mask=a 0/1 mask) + NegRegularizer, over a stored Operator
               and over a MatrixFreeOperator, through the direct loop and through the autograd
               loop (the plan functions made to return None), REPEATS times each.

--robust measures the robust fidelity terms (one leg per config beside this tree's own weighted
leg, then one gd leg; the same child processes and limits):
  robust       float64, in one process, interleaved rounds: ms per
               op.residual_gradient(x, m, s, weights=w, loss='abs') and loss='huber' with
               op.deterministic False and True, and per two-call path each replaces, op(x) then
               op.T(w * s * psi(op(x) - m)), in both modes.
               With --base DIR (a checkout of the parent commit with its library built), that
               tree's own --leg weighted runs in child processes before and after: the weighted
               and the unweighted call there, the same box and session.  Derived: each robust
               call against the parent's weighted call in the same mode and the parent's own
               run-to-run spread; this tree's weighted and unweighted calls against the
               parent's likewise (the segment sink they share was edited); each robust call
               against its two calls;
  gd_robust    ms per iteration of gd(..., 100) on bench.py's C5 retrieval problem with an
               AbsLoss and with a HuberLoss (+ NegRegularizer), over a stored Operator and over a
               MatrixFreeOperator (float64 atomics, and deterministic=True), through the direct
               loop and through the autograd loop (the plan functions made to return None),
               REPEATS times each.  --gd-only re-measures this leg alone and keeps the other
               records of the output file.
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


def leg_weighted(config, reps):
    import torch
    from sph_raytracer_amd import MatrixFreeOperator
    grid, geom, dev, xs, ys = _problem(config)
    ts = dict(time_slices=True) if grid.dynamic else {}
    x, m = xs[torch.float64], ys[torch.float64]
    g = torch.Generator(device=dev).manual_seed(1)
    w = torch.rand(m.shape, dtype=torch.float64, device=dev, generator=g)
    w[torch.rand(m.shape, device=dev, generator=g) < 0.2] = 0      # a fifth of the rays masked
    op = MatrixFreeOperator(grid, geom, dynamic=grid.dynamic, device=dev)
    rec = {'config': config, 'rays': int(op._parts[1].n), 'reps': reps, 'repeats': REPEATS,
           'dtype': 'float64', 'masked_fraction': float((w == 0).double().mean())}

    def mode(det, fn):
        def run():
            op.deterministic = det
            return fn()
        return run

    def two_calls():
        ax = op(x)
        return ax, op.T((w * 0.5) * (ax - m), **ts)

    legs = [('unweighted_fused_ms', mode(False, lambda: op.residual_gradient(x, m, 0.5)))]
    for det, tag in ((False, 'atomic'), (True, 'deterministic')):
        legs += [(f'weighted_fused_ms_{tag}',
                  mode(det, lambda: op.residual_gradient(x, m, 0.5, weights=w))),
                 (f'two_calls_ms_{tag}', mode(det, two_calls))]
    for name, fn in legs:
        fn()                                                     # warm-up
        rec[name] = []
    for _ in range(REPEATS):                                   # interleaved: one of each per round
        for name, fn in legs:
            rec[name].append(events_ms(fn, reps))
    return rec


def derive_weighted(g, parent):
    d = {'unweighted_fused_ms': _median(g['unweighted_fused_ms'])}
    if parent:
        p = [v for rec in parent for v in rec['fused_ms']]
        d['parent_unweighted_fused_ms'] = _median(p)
        d['parent_spread_ms'] = max(p) - min(p)
        d['unweighted_minus_parent_ms'] = d['unweighted_fused_ms'] - _median(p)
        d['unweighted_within_parent_spread'] = bool(
            min(p) <= d['unweighted_fused_ms'] <= max(p)
            or abs(d['unweighted_minus_parent_ms']) <= d['parent_spread_ms'])
    for tag in ('atomic', 'deterministic'):
        f, t = g[f'weighted_fused_ms_{tag}'], g[f'two_calls_ms_{tag}']
        spread = max(max(f) - min(f), max(t) - min(t))
        gain = _median(t) - _median(f)
        d[f'weighted_fused_ms_{tag}'], d[f'two_calls_ms_{tag}'] = _median(f), _median(t)
        d[f'gain_ms_{tag}'], d[f'spread_ms_{tag}'] = gain, spread
        d[f'faster_by_more_than_spread_{tag}'] = bool(gain > spread)
    return d


HUBER_DELTA = 0.25      # (the --robust legs: with m, A x in [0, ~1) both branches are taken)


def leg_robust(config, reps):
    import torch
    from sph_raytracer_amd import MatrixFreeOperator
    grid, geom, dev, xs, ys = _problem(config)
    ts = dict(time_slices=True) if grid.dynamic else {}
    x, m = xs[torch.float64], ys[torch.float64]
    g = torch.Generator(device=dev).manual_seed(1)
    w = torch.rand(m.shape, dtype=torch.float64, device=dev, generator=g)
    w[torch.rand(m.shape, device=dev, generator=g) < 0.2] = 0      # a fifth of the rays masked
    op = MatrixFreeOperator(grid, geom, dynamic=grid.dynamic, device=dev)
    r0 = op(x) - m
    rec = {'config': config, 'rays': int(op._parts[1].n), 'reps': reps, 'repeats': REPEATS,
           'dtype': 'float64', 'masked_fraction': float((w == 0).double().mean()),
           'huber_delta': HUBER_DELTA,
           'huber_inner_fraction': float((r0.abs() < HUBER_DELTA).double().mean())}
    losses = {'abs': (dict(loss='abs'), torch.sign),
              'huber': (dict(loss='huber', delta=HUBER_DELTA),
                        lambda r: torch.clamp(r, -HUBER_DELTA, HUBER_DELTA))}

    def mode(det, fn):
        def run():
            op.deterministic = det
            return fn()
        return run

    def fused(kw):
        return lambda: op.residual_gradient(x, m, 0.5, weights=w, **kw)

    def two_calls(psi):
        def run():
            ax = op(x)
            return ax, op.T((w * 0.5) * psi(ax - m), **ts)
        return run

    legs = []
    for det, tag in ((False, 'atomic'), (True, 'deterministic')):
        for loss, (kw, psi) in losses.items():
            legs += [(f'{loss}_fused_ms_{tag}', mode(det, fused(kw))),
                     (f'{loss}_two_calls_ms_{tag}', mode(det, two_calls(psi)))]
    for name, fn in legs:
        fn()                                                     # warm-up
        rec[name] = []
    for _ in range(REPEATS):                                   # interleaved: one of each per round
        for name, fn in legs:
            rec[name].append(events_ms(fn, reps))
    return rec


def derive_robust(g, own_weighted, parent):
    """`parent`: the parent tree's weighted-leg records (before and after), `own_weighted`: this
    tree's.  Every comparison with the parent: the medians, the parent's own spread (max - min
    over all its repeats) and whether the excess over the parent stays within it."""
    d = {}

    def against_parent(name, mine, key):
        p = [v for rec in parent for v in rec[key]]
        d[name] = {'ms': _median(mine), 'parent_ms': _median(p), 'parent_key': key,
                   'parent_spread_ms': max(p) - min(p),
                   'minus_parent_ms': _median(mine) - _median(p),
                   'no_slower_beyond_parent_spread':
                       bool(_median(mine) - _median(p) <= max(p) - min(p))}

    for tag in ('atomic', 'deterministic'):
        for loss in ('abs', 'huber'):
            f, t = g[f'{loss}_fused_ms_{tag}'], g[f'{loss}_two_calls_ms_{tag}']
            spread = max(max(f) - min(f), max(t) - min(t))
            gain = _median(t) - _median(f)
            d[f'{loss}_{tag}'] = {'fused_ms': _median(f), 'two_calls_ms': _median(t),
                                  'gain_ms': gain, 'spread_ms': spread,
                                  'faster_by_more_than_spread': bool(gain > spread)}
            if parent:
                against_parent(f'{loss}_{tag}_against_parent_weighted', f,
                               f'weighted_fused_ms_{tag}')
        if parent:
            against_parent(f'weighted_{tag}_against_parent',
                           own_weighted[f'weighted_fused_ms_{tag}'], f'weighted_fused_ms_{tag}')
    if parent:
        against_parent('unweighted_against_parent', own_weighted['unweighted_fused_ms'],
                       'unweighted_fused_ms')
    return d


def leg_gd_robust(config, iterations=100):
    import torch
    import bench
    from sph_raytracer_amd import MatrixFreeOperator, Operator, retrieval
    from sph_raytracer_amd.loss import AbsLoss, HuberLoss, NegRegularizer
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom = bench.build_geometry(bench.CONFIGS[config], 0, 1)
    dev = torch.device('cuda', 0)
    truth = torch.zeros(tuple(grid.shape), dtype=torch.float64, device=dev)
    truth[:, 32:, :32] = 1                       # bench.py's C5 retrieval problem
    truth[:, :32, 32:] = 1
    model = FullyDenseModel(grid)
    ops = {'stored': Operator(grid, geom, device=dev),
           'matrix_free': MatrixFreeOperator(grid, geom, device=dev),
           'matrix_free_deterministic': MatrixFreeOperator(grid, geom, device=dev,
                                                           deterministic=True)}
    y = ops['stored'](truth)
    plans = retrieval._direct_plan, retrieval._fused_plan
    terms = {'abs': AbsLoss, 'huber': lambda: HuberLoss(delta=HUBER_DELTA)}

    def none(*a, **k):
        return None

    rec = {'config': config, 'iterations': iterations, 'repeats': REPEATS,
           'huber_delta': HUBER_DELTA}
    for loss, make in terms.items():
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
                            op, y.clone(), model, num_iterations=iterations if rnd else 3,
                            lr=1e-1, loss_fns=[make(), NegRegularizer()], progress_bar=False)
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                    finally:
                        retrieval._direct_plan, retrieval._fused_plan = plans
                    if rnd:
                        into.append(dt * 1e3 / iterations)
                        final[name] = [v[-1] for v in losses.values()]
            rec[f'{loss}_{kind}_direct_ms_per_iteration'] = direct
            rec[f'{loss}_{kind}_autograd_ms_per_iteration'] = auto
            rec[f'{loss}_{kind}_final_losses_direct'] = final['direct']
            rec[f'{loss}_{kind}_final_losses_autograd'] = final['autograd']
    return rec


def derive_gd_robust(g):
    d = {}
    for loss in ('abs', 'huber'):
        for kind in ('stored', 'matrix_free', 'matrix_free_deterministic'):
            f = g[f'{loss}_{kind}_direct_ms_per_iteration']
            a = g[f'{loss}_{kind}_autograd_ms_per_iteration']
            spread = max(max(f) - min(f), max(a) - min(a))
            gain = _median(a) - _median(f)
            d[f'{loss}_{kind}'] = {'direct_ms_per_iteration': _median(f),
                                   'autograd_ms_per_iteration': _median(a), 'gain_ms': gain,
                                   'spread_ms': spread,
                                   'faster_by_more_than_spread': bool(gain > spread)}
    return d


def main_robust(args):
    out = {}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')

    base_tool = os.path.join(os.path.abspath(args.base), 'tools', os.path.basename(__file__)) \
        if args.base else None
    if args.gd_only:
        with open(args.out) as fh:
            out.update(json.load(fh))
    for config in () if args.gd_only else args.configs:
        parent = []
        if base_tool:
            before = _child('weighted', config, args.reps, base_tool)
            if before is None:
                return 1
            parent.append(before)
        own = _child('weighted', config, args.reps)
        rec = _child('robust', config, args.reps) if own is not None else None
        if rec is None:
            return 1
        if base_tool:
            again = _child('weighted', config, args.reps, base_tool)
            if again is None:
                return 1
            parent.append(again)
        out[config] = {'robust': rec, 'weighted': own, 'parent_weighted': parent,
                       'derived': derive_robust(rec, own, parent)}
        save()
    rec = _child('gd_robust', args.gd_config, None)
    if rec is None:
        return 1
    out[f'gd_{args.gd_config}'] = {'gd_robust': rec, 'derived': derive_gd_robust(rec)}
    save()
    print(json.dumps({c: out[c]['derived'] for c in out}))
    return 0


def leg_gd_masked(config, iterations=100):
    import torch
    import bench
    from sph_raytracer_amd import MatrixFreeOperator, Operator, retrieval
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom = bench.build_geometry(bench.CONFIGS[config], 0, 1)
    dev = torch.device('cuda', 0)
    truth = torch.zeros(tuple(grid.shape), dtype=torch.float64, device=dev)
    truth[:, 32:, :32] = 1                       # bench.py's C5 retrieval problem
    truth[:, :32, 32:] = 1
    model = FullyDenseModel(grid)
    ops = {'stored': Operator(grid, geom, device=dev),
           'matrix_free': MatrixFreeOperator(grid, geom, device=dev)}
    y = ops['stored'](truth)
    g = torch.Generator(device=dev).manual_seed(1)
    mask = (torch.rand(y.shape, device=dev, generator=g) > 0.2).to(torch.float64)
    plans = retrieval._direct_plan, retrieval._fused_plan

    def none(*a, **k):
        return None

    rec = {'config': config, 'iterations': iterations, 'repeats': REPEATS,
           'masked_fraction': float((mask == 0).double().mean())}
    for kind, op in ops.items():
        direct, auto, final = [], [], {}
        for rnd in range(REPEATS + 1):                         # (round 0 warms up, untimed)
            for name, into, (dp, fp) in (('direct', direct, plans), ('autograd', auto, (none, none))):
                retrieval._direct_plan, retrieval._fused_plan = dp, fp
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    _, _, losses = retrieval.gd(
                        op, y.clone(), model, num_iterations=iterations if rnd else 3, lr=1e-1,
                        loss_fns=[SquareLoss(projection_mask=mask), NegRegularizer()],
                        progress_bar=False)
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


def derive_gd_masked(g):
    d = {}
    for kind in ('stored', 'matrix_free'):
        f, a = g[f'{kind}_direct_ms_per_iteration'], g[f'{kind}_autograd_ms_per_iteration']
        spread = max(max(f) - min(f), max(a) - min(a))
        gain = _median(a) - _median(f)
        d[kind] = {'direct_ms_per_iteration': _median(f), 'autograd_ms_per_iteration': _median(a),
                   'gain_ms': gain, 'spread_ms': spread,
                   'faster_by_more_than_spread': bool(gain > spread)}
    return d


def main_weighted(args):
    out = {}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')

    base_tool = os.path.join(os.path.abspath(args.base), 'tools', os.path.basename(__file__)) \
        if args.base else None
    for config in args.configs:
        parent = []
        if base_tool:
            before = _child('gradient', config, args.reps, base_tool)
            if before is None:
                return 1
            parent.append(before)
        rec = _child('weighted', config, args.reps)
        if rec is None:
            return 1
        if base_tool:
            again = _child('gradient', config, args.reps, base_tool)
            if again is None:
                return 1
            parent.append(again)
        out[config] = {'weighted': rec, 'parent_gradient': parent,
                       'derived': derive_weighted(rec, parent)}
        save()
    rec = _child('gd_masked', args.gd_config, None)
    if rec is None:
        return 1
    out[f'gd_{args.gd_config}'] = {'gd_masked': rec, 'derived': derive_gd_masked(rec)}
    save()
    print(json.dumps({c: out[c]['derived'] for c in out}))
    return 0


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


def _child(leg, config, reps, tool=None):
    """One leg in a fresh process -> its record, or None (reported) when it failed or ran out of
    time: the caller starts nothing more.  `tool`: another checkout's copy of this script (it
    imports its own tree)."""
    cmd = [sys.executable, tool or os.path.abspath(__file__), '--leg', leg, '--configs', config]
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
    ap.add_argument('--weighted', action='store_true',
                    help='measure the weighted gradient and gd with a projection mask instead')
    ap.add_argument('--robust', action='store_true',
                    help='measure the robust (abs, huber) gradient and gd with those terms instead')
    ap.add_argument('--gd-only', action='store_true',
                    help='--robust: the gd leg alone, into the existing output file')
    ap.add_argument('--base', default=None,
                    help='--weighted, --robust: a checkout of the parent commit, its library built')
    ap.add_argument('--gd-config', default='c5',
                    help='the gd leg\'s problem (--gradient, --weighted, --robust)')
    ap.add_argument('--leg', choices=('matrix_free', 'operator', 'gradient', 'gd', 'deterministic',
                                      'weighted', 'gd_masked', 'robust', 'gd_robust'),
                    help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'matrix_free_robust_times.json'
                                if args.robust else 'matrix_free_weighted_times.json'
                                if args.weighted else 'matrix_free_deterministic_times.json'
                                if args.deterministic else 'matrix_free_gradient_times.json'
                                if args.gradient else 'matrix_free_times.json')
    if args.leg in ('gd', 'gd_masked', 'gd_robust'):
        fn = {'gd': leg_gd, 'gd_masked': leg_gd_masked, 'gd_robust': leg_gd_robust}[args.leg]
        print(json.dumps(fn(args.configs[0])))
        return 0
    if args.leg:
        reps = args.reps or (5 if args.configs[0] == 'c3' else 20)
        fn = {'matrix_free': leg_matrix_free, 'operator': leg_operator,
              'gradient': leg_gradient, 'deterministic': leg_deterministic,
              'weighted': leg_weighted, 'robust': leg_robust}[args.leg]
        print(json.dumps(fn(args.configs[0], reps)))
        return 0
    if args.robust:
        return main_robust(args)
    if args.weighted:
        return main_weighted(args)
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
