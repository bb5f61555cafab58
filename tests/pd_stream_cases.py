"""The stream-order rows of retrieval.primal_dual (no tests; importing it needs no GPU): what
stream_cases.ROWS is for include/sphrt.h, for the entries of include/sphrt_pd.h.
test_gpu_pd_stream.py runs every row behind the gate of stream_gate.py; test_pd_cpu.py holds the
table to the header: every entry of sphrt_pd.h that takes a stream is reached by a row, and
there is no exempt list.

The rows are stream_cases' solve rows with the solver exchanged: the tiny problem in the four
mask / smooth variants over the three operators, and the two-workgroup problem over the stored
operator; the same operators, inputs and damp (stream_cases.Solve), twenty iterations, a TV term
of weight 0.05 over all three axes with the ring closed, bounds 0 / 0.9."""
import stream_cases as sc

PD_ENTRIES = ['sphrt_pd_primal_f64', 'sphrt_pd_dual_f64']
LAM_TV = 0.05


def _rows():
    rows = []
    for row in sc.ROWS:
        if row.recipe != 'solve' or row.params['solver'] != 'fista':
            continue
        entries = [e for e in row.entries if not e.startswith('sphrt_pg_')] + PD_ENTRIES
        rows.append(row._replace(name='pd' + row.name[len('fista'):], recipe='pd_solve',
                                 params=dict(row.params, solver='primal_dual'),
                                 entries=tuple(entries)))
    return rows


ROWS = _rows()
BY_NAME = {r.name: r for r in ROWS}
NAMES = [r.name for r in ROWS]


class PdSolve(sc.Solve):
    @staticmethod
    def call(row, ctx, y, x0, mask=1):
        from sph_raytracer_amd import retrieval
        from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
        p = row.params
        fns = [1.5 * SquareLoss(projection_mask=mask)]
        if p['wrap'] is not None:
            fns.append(0.3 * SmoothRegularizer(weights=(1, 0.5, 2), wrap_a=p['wrap']))
        fns.append(LAM_TV * SmoothRegularizer(kind='abs', wrap_a=True))
        x, yhat, info = retrieval.primal_dual(ctx['op'], y, fns, x0=x0, damp=ctx['damp'],
                                              num_iterations=sc.SOLVE_ITERATIONS, lower=0.0,
                                              upper=0.9)
        return [x, yhat, list(info['primal_change']), list(info['dual_change']),
                [info['lipschitz'], info['tau'], info['sigma']], info['dual']]


RECIPES = {'pd_solve': PdSolve}
