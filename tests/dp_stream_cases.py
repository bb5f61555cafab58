"""The stream-order rows of retrieval.chambolle_pock(precondition='diagonal') (no tests; importing
it needs no GPU): what cp_stream_cases.ROWS is for include/sphrt_cp.h, for the three entries of
include/sphrt_dp.h.  test_gpu_dp_stream.py runs every row behind the gate of stream_gate.py;
test_dp_cpu.py holds the table to the header: every entry of sphrt_dp.h that takes a stream is
reached by every row, and there is no exempt list.

The rows are cp_stream_cases' rows with the keyword set: the same operators, inputs, damp,
fidelity kinds, TV terms and bounds (the terms are built as cp_stream_cases.CpSolve builds them).  The set-up differs — one forward
and one adjoint of ones and the sphrt_dp_steps_f64 launch instead of the power method, so the
rows no longer name the normal-equation entries — and the loop launches sphrt_dp_primal_f64 and
sphrt_dp_ray_dual_f64 once per iteration, sphrt_dp_steps_f64 once per solve.  No row reads
anything back before the solve's single Tensor.cpu(): rho and c are host numbers, and tau and
sigma stay on the device."""
import cp_stream_cases as csc
import stream_cases as sc

DP_ENTRIES = ['sphrt_dp_primal_f64', 'sphrt_dp_ray_dual_f64', 'sphrt_dp_steps_f64']
# how often a solve of sc.SOLVE_ITERATIONS iterations launches each entry of the loop's own
PER_SOLVE = {'sphrt_dp_steps_f64': 1}
DROPPED = ('sphrt_sq_residual_f64', 'sphrt_trace_normal_f64', 'sphrt_trace_normal_fixed_f64',
           'sphrt_pd_primal_f64', 'sphrt_cp_ray_dual_f64')


def _rows():
    rows = []
    for row in csc.ROWS:
        entries = [e for e in row.entries if e not in DROPPED] + DP_ENTRIES
        rows.append(row._replace(name='dp-' + row.name[len('cp-'):], recipe='dp_solve',
                                 entries=tuple(entries)))
    return rows


ROWS = _rows()
BY_NAME = {r.name: r for r in ROWS}
NAMES = [r.name for r in ROWS]


def launches(entry):
    return PER_SOLVE.get(entry, sc.SOLVE_ITERATIONS)


class DpSolve(csc.CpSolve):
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
            fns.append(csc.LAM_TV * SmoothRegularizer(kind='abs', wrap_a=True))
        if kind == 'poisson':
            y = y.abs() + 0.1
        x, yhat, info = retrieval.chambolle_pock(ctx['op'], y, fns, x0=x0, damp=ctx['damp'],
                                                 num_iterations=sc.SOLVE_ITERATIONS, lower=0.0,
                                                 upper=0.9, precondition='diagonal')
        assert info['norm'] is None
        out = [x, yhat, info['ray_dual'], info['tau'], info['sigma'], [info['sigma_tv']],
               list(info['primal_change']), list(info['ray_dual_change']), list(info['fidelity'])]
        # (without TV 'dual' is None and 'dual_change' all zeros: nothing to compare)
        return out + ([info['dual'], list(info['dual_change'])] if p['tv'] else [])


RECIPES = {'dp_solve': DpSolve}
