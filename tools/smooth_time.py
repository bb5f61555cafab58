#!/usr/bin/env python3
"""Time of the smoothness regulariser (sphrt_smooth_reg_f64, loss.SmoothRegularizer) on one GPU.

    python tools/smooth_time.py [--base DIR] [--out profiles/smooth_reg_times.json]

Legs, each in a fresh child process with its own time limit (a leg that fails or runs out of time
ends the run: nothing more is started):
  kernel   the entry alone on a 64^3 and a 128^3 float64 volume, per kind, stand-alone (g_out = G)
           and folded (g_in = g_out, the NegRegularizer's term and partials): ms per launch from
           HIP events around `reps` back-to-back launches, REPEATS interleaved rounds, all kept;
           beside each median the bytes it must move (stand-alone 16 B / voxel: d and g_out;
           folded 24 B / voxel: d, g_in and g_out) and the rate that implies;
  gd       ms per iteration of gd(..., 100) on bench.py's C5 retrieval problem over a stored
           Operator, REPEATS interleaved rounds: the direct loop with [SquareLoss,
           NegRegularizer, SmoothRegularizer]; the direct loop with [SquareLoss, NegRegularizer]
           (the path this term leaves untouched); and the autograd loop with the smooth term
           written as the plain-torch formula (a subclass that computes `formula`: what a user
           had to write before), per kind;
  gd_pair  with --base DIR (a checkout of the parent commit with its library built): the
           [SquareLoss, NegRegularizer] direct loop with that tree's package, before and after
           the gd leg, the same box and session.
Derived: medians, the spread (max - min) of the repeats, the three-term direct loop against the
autograd loop, the two-term loop here against the parent's repeats and their spread.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEG_LIMIT_S = 300
REPEATS = 5
KINDS = (('square', None), ('abs', None), ('huber', 0.25))


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


def _median(v):
    return sorted(v)[len(v) // 2]


def leg_kernel(reps):
    import torch
    from sph_raytracer_amd import _lib
    from sph_raytracer_amd.loss import SmoothRegularizer
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    rec = {'reps': reps, 'repeats': REPEATS, 'dtype': 'float64'}
    for n in (64, 128):
        g = torch.Generator(device=dev).manual_seed(0)
        d = torch.randn((n, n, n), dtype=torch.float64, device=dev, generator=g)
        grad = torch.randn((n, n, n), dtype=torch.float64, device=dev, generator=g)
        out = torch.empty_like(d)
        n_part = lib.sphrt_loss_partials(d.numel())
        part = torch.empty(n_part, dtype=torch.float64, device=dev)
        part_neg = torch.empty(n_part, dtype=torch.float64, device=dev)
        legs = []
        for kind, delta in KINDS:
            reg = SmoothRegularizer(kind=kind, delta=delta)
            legs += [(f'{kind}_alone', 16,
                      lambda reg=reg: reg._launch(d, True, 0.5, 0.0, None, out, part, None)),
                     (f'{kind}_folded', 24,
                      lambda reg=reg: reg._launch(d, True, 0.5, 1e-6, grad, grad, part, part_neg))]
        times = {name: [] for name, _, _ in legs}
        for name, _, fn in legs:
            for _ in range(20):
                fn()                                                # warm-up
        for _ in range(REPEATS):                                   # interleaved rounds
            for name, _, fn in legs:
                times[name].append(events_ms(fn, reps))
        for name, bpv, _ in legs:
            ms = _median(times[name])
            rec[f'{n}^3_{name}'] = {
                'ms': times[name], 'median_ms': ms, 'spread_ms': max(times[name]) - min(times[name]),
                'bytes_per_voxel': bpv, 'bytes': bpv * d.numel(),
                'implied_gb_per_s': bpv * d.numel() / (ms * 1e-3) / 1e9}
    return rec


def _c5(dev):
    import torch
    import bench
    from sph_raytracer_amd import Operator
    from sph_raytracer_amd.model import FullyDenseModel
    grid, geom = bench.build_geometry(bench.CONFIGS['c5'], 0, 1)
    truth = torch.zeros(tuple(grid.shape), dtype=torch.float64, device=dev)
    truth[:, 32:, :32] = 1                       # bench.py's C5 retrieval problem
    truth[:, :32, 32:] = 1
    op = Operator(grid, geom, device=dev)
    return op, op(truth), FullyDenseModel(grid)


def _time_gd(op, y, model, make_terms, iterations, expect_direct):
    import torch
    from sph_raytracer_amd import retrieval
    calls = []
    direct = retrieval._gd_direct
    retrieval._gd_direct = lambda *a, **k: calls.append(1) or direct(*a, **k)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, losses = retrieval.gd(op, y.clone(), model, num_iterations=iterations, lr=1e-1,
                                    loss_fns=make_terms(), progress_bar=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        retrieval._gd_direct = direct
    if bool(calls) != expect_direct:
        raise RuntimeError(f'expected the {"direct" if expect_direct else "autograd"} loop')
    return dt * 1e3 / iterations, [v[-1] for v in losses.values()]


def leg_gd_pair(iterations=100):
    """The [SquareLoss, NegRegularizer] direct loop alone (any tree of this package)."""
    import torch
    from sph_raytracer_amd.loss import NegRegularizer, SquareLoss
    op, y, model = _c5(torch.device('cuda', 0))
    rec = {'iterations': iterations, 'repeats': REPEATS, 'direct2_ms_per_iteration': []}
    for rnd in range(REPEATS + 1):                                 # (round 0 warms up, untimed)
        ms, final = _time_gd(op, y, model, lambda: [SquareLoss(), NegRegularizer()],
                             iterations if rnd else 3, True)
        if rnd:
            rec['direct2_ms_per_iteration'].append(ms)
            rec['final_losses'] = final
    return rec


def leg_gd(iterations=100):
    import torch
    from sph_raytracer_amd.loss import NegRegularizer, SmoothRegularizer, SquareLoss
    op, y, model = _c5(torch.device('cuda', 0))

    class FormulaSmooth(SmoothRegularizer):
        """The term as a user writes it in torch (a subclass: the autograd loop)."""

        def compute(self, f, y, d, c):
            return self.formula(d, self.wraps(f))

    variants = [('direct2', True, lambda: [SquareLoss(), NegRegularizer()])]
    for kind, delta in KINDS:
        variants += [
            (f'direct3_{kind}', True, lambda kind=kind, delta=delta: [
                SquareLoss(), NegRegularizer(), 0.5 * SmoothRegularizer(kind=kind, delta=delta)]),
            (f'autograd_formula_{kind}', False, lambda kind=kind, delta=delta: [
                SquareLoss(), NegRegularizer(), 0.5 * FormulaSmooth(kind=kind, delta=delta)])]
    rec = {'iterations': iterations, 'repeats': REPEATS}
    for name, _, _ in variants:
        rec[f'{name}_ms_per_iteration'] = []
    for rnd in range(REPEATS + 1):                                 # (round 0 warms up, untimed)
        for name, is_direct, make in variants:
            ms, final = _time_gd(op, y, model, make, iterations if rnd else 3, is_direct)
            if rnd:
                rec[f'{name}_ms_per_iteration'].append(ms)
                rec[f'{name}_final_losses'] = final
    return rec


def derive_gd(g, parent):
    d = {}
    two = g['direct2_ms_per_iteration']
    d['direct2'] = {'ms_per_iteration': _median(two), 'spread_ms': max(two) - min(two)}
    if parent:
        p = [v for rec in parent for v in rec['direct2_ms_per_iteration']]
        d['direct2'].update({
            'parent_ms_per_iteration': _median(p), 'parent_spread_ms': max(p) - min(p),
            'minus_parent_ms': _median(two) - _median(p),
            'no_slower_beyond_parent_spread': bool(_median(two) - _median(p) <= max(p) - min(p))})
    for kind, _ in KINDS:
        f, a = g[f'direct3_{kind}_ms_per_iteration'], g[f'autograd_formula_{kind}_ms_per_iteration']
        spread = max(max(f) - min(f), max(a) - min(a))
        gain = _median(a) - _median(f)
        d[kind] = {'direct3_ms_per_iteration': _median(f),
                   'autograd_formula_ms_per_iteration': _median(a),
                   'smooth_term_cost_ms': _median(f) - _median(two), 'gain_ms': gain,
                   'spread_ms': spread, 'faster_by_more_than_spread': bool(gain > spread)}
    return d


def _child(leg, reps=None, tree=None):
    """One leg in a fresh process -> its record, or None (reported) when it failed or ran out of
    time: the caller starts nothing more.  `tree`: the checkout whose package the leg imports."""
    cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg]
    if reps:
        cmd += ['--reps', str(reps)]
    if tree:
        cmd += ['--tree', tree]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(f'{leg}: no result within {LEG_LIMIT_S} s; stopping', file=sys.stderr)
        return None
    if res.returncode != 0:
        print(f'{leg}: exit {res.returncode}; stopping\n{res.stderr[-2000:]}', file=sys.stderr)
        return None
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    print(f'{leg}: {rec}', file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200, help='launches per kernel timing')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'smooth_reg_times.json'))
    ap.add_argument('--base', default=None,
                    help='a checkout of the parent commit (its package, its library built)')
    ap.add_argument('--leg', choices=('kernel', 'gd', 'gd_pair'), help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        # (bench.py comes from this tree; the package from --tree when given)
        sys.path.insert(0, ROOT)
        if args.tree:
            sys.path.insert(0, os.path.abspath(args.tree))
        import sph_raytracer_amd       # (before bench.py, which puts its own tree first)
        if args.tree and not sph_raytracer_amd.__file__.startswith(os.path.abspath(args.tree)):
            raise RuntimeError(f'the package came from {sph_raytracer_amd.__file__}')
        rec = leg_kernel(args.reps) if args.leg == 'kernel' else \
            leg_gd() if args.leg == 'gd' else leg_gd_pair()
        print(json.dumps(rec))
        return 0
    out = {}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')

    out['kernel'] = _child('kernel', args.reps)
    if out['kernel'] is None:
        return 1
    save()
    parent = []
    if args.base:
        parent.append(_child('gd_pair', tree=args.base))
        if parent[-1] is None:
            return 1
    rec = _child('gd')
    if rec is None:
        return 1
    if args.base:
        parent.append(_child('gd_pair', tree=args.base))
        if parent[-1] is None:
            return 1
    out['gd_c5'] = {'gd': rec, 'parent_gd_pair': parent, 'derived': derive_gd(rec, parent)}
    save()
    print(json.dumps(out['gd_c5']['derived']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
