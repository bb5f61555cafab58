"""retrieval.gd's direct loops as assembled, on the GPU: every row of gd_cases.CASES (a pairwise
covering array over fidelity x mask x y dtype x regularisers x operator x optimiser) against a
reference that runs no HIP kernel — retrieval.gd's autograd loop on the CPU over the C oracle's
system matrix (gd_cases.reference) — within the bound gd_cases.bounds derives from that
reference's own sensitivity to summation order; the route each case's factors name (the loop, the
optimiser split, the C entries and how often, the permuted measurements); the autograd loop over
the same operator on the device, bitwise where `_gd_direct`'s docstring promises equal iterates
(the stored operators, and the deterministic matrix-free operator's two-trace Poisson form) and
within the reference bound everywhere; bit reproducibility on the deterministic operators; and
the side effects on the caller's tensors and the optimiser.  The rows of gd_cases.DECLINED take
the autograd loop and meet the same bound."""
import numpy as np
import pytest
import torch as tr

import gd_cases as gc

pytestmark = pytest.mark.gpu

F64 = tr.float64
N = gc.N_IT

ENTRIES = ['sphrt_sq_residual_f64', 'sphrt_wsq_residual_f64', 'sphrt_robust_residual_f64',
           'sphrt_poisson_residual_f64', 'sphrt_neg_reg_f64', 'sphrt_smooth_reg_f64',
           'sphrt_adam_neg_f64', 'sphrt_adam_foreach_neg_f64', 'sphrt_trace_normal_f64',
           'sphrt_trace_normal_fixed_f64', 'sphrt_trace_normal_weighted_f64',
           'sphrt_trace_normal_weighted_fixed_f64', 'sphrt_trace_normal_robust_f64',
           'sphrt_trace_normal_robust_fixed_f64', 'sphrt_trace_normal_poisson_f64',
           'sphrt_trace_backproject_fixed_f64', 'sphrt_trace_integrate_f64']


def expected_entries(case):
    """How often a direct run of N iterations (and the returned forward) calls each C entry."""
    want = dict.fromkeys(ENTRIES, 0)
    kind = {'square': 'sq' if case.M == 'unit' else 'wsq', 'abs': 'robust', 'huber': 'robust',
            'poisson': 'poisson'}[case.F]
    want[f'sphrt_{kind}_residual_f64'] = N
    if case.R in ('smooth', 'both'):
        want['sphrt_smooth_reg_f64'] = N
    elif case.R == 'neg' and case.P == 'sgd':
        want['sphrt_neg_reg_f64'] = N
    if case.P == 'adam_fused':
        want['sphrt_adam_neg_f64'] = N
    elif case.P != 'sgd':
        want['sphrt_adam_foreach_neg_f64'] = N
    if case.O.startswith('mf'):
        want['sphrt_trace_integrate_f64'] = 1                      # the returned forward
        det = case.O == 'mf_deterministic'
        if case.F == 'poisson' and det:                            # two traces per iteration
            want['sphrt_trace_integrate_f64'] += N
            want['sphrt_trace_backproject_fixed_f64'] = N
        else:
            trace = {'sq': 'normal', 'wsq': 'normal_weighted'}.get(kind, 'normal_' + kind)
            want[f'sphrt_trace_{trace}{"_fixed" if det else ""}_f64'] = N
    return want


_OPERATORS = {}


def _operator(case, gpu, monkeypatch):
    from sph_raytracer_amd import MatrixFreeOperator, Operator
    for var in ('SPHRT_RAY_ORDER', 'SPHRT_TCOLS'):
        monkeypatch.delenv(var, raising=False)
    key = (case.geometry, case.O.startswith('mf'))
    if key not in _OPERATORS:
        grid, geom = gc.geometry(case.geometry)
        _OPERATORS[key] = (MatrixFreeOperator if key[1] else Operator)(grid, geom, device=gpu)
    op = _OPERATORS[key]
    if key[1]:
        monkeypatch.setattr(op, 'deterministic', case.O == 'mf_deterministic')
    return op


class _Spy:
    """Counts of `_gd_direct`'s runs (with their optimisers), `_split_adam`'s answers and the C
    entries' calls."""

    def __init__(self, monkeypatch):
        from sph_raytracer_amd import _lib, retrieval
        self.direct, self.split, self.opts = 0, [], []
        self.entries = dict.fromkeys(ENTRIES, 0)
        direct, split, lib = retrieval._gd_direct, retrieval._split_adam, _lib.load()

        def gd_direct(*a, **k):
            self.direct += 1
            self.opts.append(a[4])
            return direct(*a, **k)

        def split_adam(*a, **k):
            step = split(*a, **k)
            self.split.append(step is not None)
            return step
        monkeypatch.setattr(retrieval, '_gd_direct', gd_direct)
        monkeypatch.setattr(retrieval, '_split_adam', split_adam)
        for name in ENTRIES:
            def counted(*a, _fn=getattr(lib, name), _name=name):
                self.entries[_name] += 1
                return _fn(*a)
            monkeypatch.setattr(lib, name, counted)

    def reset(self):
        self.direct, self.split, self.opts = 0, [], []
        self.entries = dict.fromkeys(ENTRIES, 0)


def _run(op, case, gpu):
    """retrieval.gd on device copies of the case's inputs -> (Result, (y, mask, c0) as handed in,
    the loss terms (fid, neg, smooth))."""
    return gc.run_gd(op, case, gc.inputs(case), device=gpu)


def _no_plans(mp):
    from sph_raytracer_amd import retrieval
    mp.setattr(retrieval, '_direct_plan', lambda *a: None)
    mp.setattr(retrieval, '_fused_plan', lambda *a: None)


def _bits(res):
    return (res.c.view(np.int64).tolist(), res.y.view(np.int64).tolist(),
            [np.asarray(h).view(np.int64).tolist() for h in res.hist])


def _within(case, got, what):
    """`got` against the CPU reference: coefficients, stack and every loss history within the
    case's bound -> the largest distance as a fraction of its bound."""
    ref = gc.reference(case.name)
    b_c, b_y, b_h = gc.bounds(case.name)
    d_c, d_y, d_h = gc.distance(got, ref)
    assert got.c.shape == ref.c.shape and got.y.shape == ref.y.shape
    assert [len(h) for h in got.hist] == [N] * len(ref.hist)
    worst = max([d_c / b_c, d_y / b_y] + [d / b for d, b in zip(d_h, b_h)])
    print(f'{case.name} {what}: coefficients {d_c:.3g} (bound {b_c:.3g}), stack {d_y:.3g} '
          f'({b_y:.3g}), histories {["%.3g" % d for d in d_h]} ({["%.3g" % b for b in b_h]}); '
          f'worst {worst:.3g} of its bound')
    assert d_c <= b_c, (d_c, b_c)
    assert d_y <= b_y, (d_y, b_y)
    for d, b in zip(d_h, b_h):
        assert d <= b, (d_h, b_h)
    return worst


@pytest.mark.parametrize('name', gc.NAMES)
def test_case(name, gpu, monkeypatch):
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.model import FullyDenseModel
    case = gc.BY_NAME[name]
    op = _operator(case, gpu, monkeypatch)
    stored, det = case.O.startswith('stored'), case.O != 'mf_atomic'
    # the operator is the one the row names
    if stored:
        order = op._adjoint_trace_order()
        sd = op._stage_for_loop(F64)
        sd = sd[0] if sd is not None else op._loop_descriptor(F64)
        rows = op._trace_position_rows(sd) if sd is not None else None
        assert (order is not None) == (case.O == 'stored_reordered')
        assert (rows is not None) == (case.O == 'stored_reordered')
    else:
        assert op.deterministic == (case.O == 'mf_deterministic')
    inp = gc.inputs(case)
    spy = _Spy(monkeypatch)

    # ---- the direct loop and its route
    got, (y, mask, c0), (fid, neg, smooth) = _run(op, case, gpu)
    assert spy.direct == 1
    assert spy.split == [case.P != 'sgd']
    assert spy.entries == expected_entries(case), \
        {k: (v, expected_entries(case)[k]) for k, v in spy.entries.items()
         if v != expected_entries(case)[k]}
    model = FullyDenseModel(op.grid)
    plan = (retrieval._direct_plan if stored else retrieval._fused_plan)(
        op, y, model, c0, [fn for fn in (fid, neg, smooth) if fn is not None], [c0])
    assert plan == ((fid, neg, smooth) if smooth is not None else (fid, neg))

    # ---- side effects: y and the mask as handed in (y now requires grad, as in the reference);
    # the coefficients handed in are the ones optimised and returned; the optimiser's state
    assert y.requires_grad and y.dtype == inp.y.dtype and tr.equal(y.detach().cpu(), inp.y)
    if isinstance(mask, tr.Tensor):
        assert not mask.requires_grad and mask.dtype == inp.mask.dtype
        assert tr.equal(mask.cpu(), inp.mask)
    assert np.array_equal(c0.detach().cpu().numpy(), got.c) and not tr.equal(c0.cpu(), inp.c0)
    opt, = spy.opts
    if case.P == 'sgd':        # opt.step() ran: the momentum buffer of the one parameter
        assert len(opt.state) == 1 and next(iter(opt.state)) is c0
        assert opt.state[c0]['momentum_buffer'].shape == c0.shape
    else:                      # the loop owns the moments: the optimiser's state is untouched
        assert len(opt.state) == 0
    assert c0.grad is None or case.P == 'sgd'

    # ---- against the CPU reference (no HIP kernel on that side)
    worst = _within(case, got, 'direct loop')

    # ---- a second run: the same bits on the deterministic operators
    spy.reset()
    again, _, _ = _run(op, case, gpu)
    assert spy.direct == 1 and spy.entries == expected_entries(case)
    if det:
        assert _bits(again) == _bits(got)
    else:
        _within(case, again, 'direct loop again')

    # ---- against the autograd loop over the same operator
    spy.reset()
    with monkeypatch.context() as mp:
        _no_plans(mp)
        auto, _, _ = _run(op, case, gpu)
    assert spy.direct == 0 and spy.split == []
    _within(case, auto, 'autograd loop on the device')
    same = np.array_equal(auto.c.view(np.int64), got.c.view(np.int64)) \
        and np.array_equal(auto.y.view(np.int64), got.y.view(np.int64))
    print(f'{name}: direct and autograd iterates bitwise equal: {same}; worst {worst:.3g}')
    if stored or (case.O == 'mf_deterministic' and case.F == 'poisson'):
        # (`_gd_direct`: "the same iterates"; the deterministic operator's other terms quantise
        # the scaled residual on another fixed-point grid than op.T does: no such promise)
        assert same
        for ha, hb in zip(got.hist, auto.hist):
            assert np.allclose(ha, hb, rtol=1e-13, atol=0), (ha, hb)


@pytest.mark.parametrize('name', gc.DECLINED_NAMES)
def test_declined(name, gpu, monkeypatch):
    """`_loop_terms` refuses the row, `_gd_direct` is not entered, and the autograd loop over the
    stored operator meets the reference bound."""
    from sph_raytracer_amd import retrieval
    from sph_raytracer_amd.model import FullyDenseModel
    case = gc.BY_NAME[name]
    op = _operator(case, gpu, monkeypatch)
    spy = _Spy(monkeypatch)
    got, (y, mask, c0), parts = _run(op, case, gpu)
    assert spy.direct == 0 and spy.split == []
    fns, _ = gc.terms(case, mask, gpu)
    model = FullyDenseModel(op.grid)
    assert retrieval._loop_terms(op, y, model, c0, fns, [c0]) is None
    assert retrieval._direct_plan(op, y, model, c0, fns, [c0]) is None
    # (the same terms in the accepted order, without the refused attribute, are taken)
    base = gc.BY_NAME[gc.NAMES[0]]._replace(**{f: getattr(case, f) for f in gc.Case._fields
                                               if f != 'name'})
    ok, _ = gc.terms(base, mask, gpu)
    assert retrieval._loop_terms(op, y, model, c0, ok, [c0]) is not None
    _within(case, got, 'autograd loop (declined)')
