"""The stream-order rows of the isotropic-TV branch of retrieval.primal_dual and
retrieval.chambolle_pock (no tests; importing it needs no GPU): what pd_stream_cases.ROWS is for
include/sphrt_pd.h, for the two entries of include/sphrt_iso.h.  test_gpu_iso_stream.py runs every
row behind the gate of stream_gate.py; test_iso_cpu.py holds the table to the header: every entry
of sphrt_iso.h that takes a stream is reached by every row, and there is no exempt list.

One row per operator kind and solver: the first of pd_stream_cases' rows over that operator, and
the first of cp_stream_cases' rows over it that carries a TV term, with the TV term exchanged for
an IsoTVRegularizer of the same weight (weights 1, 0.5, 2, the ring closed) — the same operators,
inputs, damp, iteration count and bounds.  The rows name sphrt_iso_primal_f64 and
sphrt_iso_dual_f64 where the originals name the two entries of sphrt_pd.h."""
import cp_stream_cases as csc
import pd_stream_cases as psc
import stream_cases as sc

ISO_ENTRIES = ['sphrt_iso_primal_f64', 'sphrt_iso_dual_f64']
WEIGHTS = (1.0, 0.5, 2.0)


def _rows():
    rows = []
    for source, prefix, pick in ((psc.ROWS, 'pd', lambda r: True),
                                 (csc.ROWS, 'cp', lambda r: r.params['tv'])):
        seen = set()
        for row in source:
            kind = row.params['kind']
            if kind in seen or not pick(row):
                continue
            seen.add(kind)
            entries = [e for e in row.entries if e not in psc.PD_ENTRIES] + ISO_ENTRIES
            rows.append(row._replace(name=f'iso-{row.name}', recipe=f'iso_{prefix}_solve',
                                     entries=tuple(entries)))
    return rows


ROWS = _rows()
BY_NAME = {r.name: r for r in ROWS}
NAMES = [r.name for r in ROWS]


def _iso(lam):
    from sph_raytracer_amd.loss import IsoTVRegularizer
    return lam * IsoTVRegularizer(weights=WEIGHTS, wrap_a=True)


class IsoPdSolve(sc.Solve):
    @staticmethod
    def call(row, ctx, y, x0, mask=1):
        from sph_raytracer_amd import retrieval
        from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
        p = row.params
        fns = [1.5 * SquareLoss(projection_mask=mask)]
        if p['wrap'] is not None:
            fns.append(0.3 * SmoothRegularizer(weights=(1, 0.5, 2), wrap_a=p['wrap']))
        fns.append(_iso(psc.LAM_TV))
        x, yhat, info = retrieval.primal_dual(ctx['op'], y, fns, x0=x0, damp=ctx['damp'],
                                              num_iterations=sc.SOLVE_ITERATIONS, lower=0.0,
                                              upper=0.9)
        return [x, yhat, list(info['primal_change']), list(info['dual_change']),
                [info['lipschitz'], info['tau'], info['sigma']], info['dual']]


class IsoCpSolve(csc.CpSolve):
    @staticmethod
    def call(row, ctx, y, x0, mask=1):
        from sph_raytracer_amd import retrieval
        from sph_raytracer_amd.loss import AbsLoss, HuberLoss, PoissonLoss, SquareLoss
        p = row.params
        kind = p['fidelity']
        fid = {'square': SquareLoss, 'abs': AbsLoss, 'poisson': PoissonLoss,
               'huber': lambda **kw: HuberLoss(delta=0.05, **kw)}[kind](projection_mask=mask)
        fns = [1.5 * fid, _iso(csc.LAM_TV)]
        if kind == 'poisson':
            y = y.abs() + 0.1
        x, yhat, info = retrieval.chambolle_pock(ctx['op'], y, fns, x0=x0, damp=ctx['damp'],
                                                 num_iterations=sc.SOLVE_ITERATIONS, lower=0.0,
                                                 upper=0.9)
        return [x, yhat, info['ray_dual'], list(info['primal_change']),
                list(info['ray_dual_change']), list(info['fidelity']),
                [info['norm'], info['tau'], info['sigma']], info['dual'],
                list(info['dual_change'])]


RECIPES = {'iso_pd_solve': IsoPdSolve, 'iso_cp_solve': IsoCpSolve}
