"""The stream-order rows of retrieval.chambolle_pock (no tests; importing it needs no GPU): what
stream_cases.ROWS is for include/sphrt.h, for the entry of include/sphrt_cp.h.
test_gpu_cp_stream.py runs every row behind the gate of stream_gate.py; test_cp_cpu.py holds the
table to the header: every entry of sphrt_cp.h that takes a stream is reached by every row, and
there is no exempt list.

The rows are stream_cases' fista solve rows with the solver exchanged: the tiny problem in the
four mask / smooth variants over the three operators, and the two-workgroup problem over the
stored operator; the same operators, inputs and damp (stream_cases.Solve), twenty iterations,
bounds 0 / 0.9.  The fidelity kind cycles through square, abs, huber and poisson over the rows
(the Poisson rows solve for |y| + 0.1, formed on the stream: counts are positive); a row whose
fista variant has a smooth term carries a TV term of weight 0.05 over all three axes with the
ring closed, the others none, so the loop is gated with and without its TV-dual launch.  No row
reads anything back before the solve's single Tensor.cpu(): the power method runs unweighted,
and the deterministic back-projection takes its scale on the device."""
import stream_cases as sc

CP_ENTRIES = ['sphrt_cp_ray_dual_f64']
KINDS = ['square', 'abs', 'huber', 'poisson']
LAM_TV = 0.05


def _rows():
    rows = []
    picked = [r for r in sc.ROWS if r.recipe == 'solve' and r.params['solver'] == 'fista']
    for k, row in enumerate(picked):
        p = row.params
        kind, tv = KINDS[k % 4], p['wrap'] is not None
        if p['kind'] == 'stored':
            entries = ['sphrt_forward_f64', 'sphrt_sq_residual_f64']
        elif p['kind'] == 'matrix_free':
            entries = ['sphrt_trace_integrate_f64', 'sphrt_trace_normal_f64',
                       'sphrt_trace_backproject_f64']
        else:
            entries = ['sphrt_trace_integrate_f64', 'sphrt_trace_normal_fixed_f64',
                       'sphrt_trace_backproject_fixed_f64', 'sphrt_fixed_scale_f64',
                       'sphrt_fixed_finalize_f64']
        entries += ['sphrt_pd_primal_f64'] + (['sphrt_pd_dual_f64'] if tv else []) + CP_ENTRIES
        rows.append(row._replace(name=f'cp-{kind}' + row.name[len('fista'):], recipe='cp_solve',
                                 params=dict(p, solver='chambolle_pock', fidelity=kind, tv=tv),
                                 entries=tuple(entries), nosync='readback', readbacks=1))
    return rows


ROWS = _rows()
BY_NAME = {r.name: r for r in ROWS}
NAMES = [r.name for r in ROWS]


class CpSolve(sc.Solve):
    @staticmethod
    def call(row, ctx, y, x0, mask=1):
        from sph_raytracer_amd import retrieval
        from sph_raytracer_amd.loss import (AbsLoss, HuberLoss, PoissonLoss, SmoothRegularizer,
                                            SquareLoss)
        p = row.params
        kind = p['fidelity']
        fid = {'square': SquareLoss, 'abs': AbsLoss, 'poisson': PoissonLoss,
               'huber': lambda **kw: HuberLoss(delta=0.05, **kw)}[kind](projection_mask=mask)
        fns = [1.5 * fid]
        if p['tv']:
            fns.append(LAM_TV * SmoothRegularizer(kind='abs', wrap_a=True))
        if kind == 'poisson':
            y = y.abs() + 0.1
        x, yhat, info = retrieval.chambolle_pock(ctx['op'], y, fns, x0=x0, damp=ctx['damp'],
                                                 num_iterations=sc.SOLVE_ITERATIONS, lower=0.0,
                                                 upper=0.9)
        out = [x, yhat, info['ray_dual'], list(info['primal_change']),
               list(info['ray_dual_change']), list(info['fidelity']),
               [info['norm'], info['tau'], info['sigma']]]
        # (without TV 'dual' is None and 'dual_change' all zeros: nothing to compare)
        return out + ([info['dual'], list(info['dual_change'])] if p['tv'] else [])


RECIPES = {'cp_solve': CpSolve}
