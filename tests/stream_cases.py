"""The table of launch paths test_gpu_stream_order.py runs behind the gate of stream_gate.py (no
tests; importing it needs no GPU), and the recipes that build each row's operator and inputs.
test_stream_cases_cpu.py holds the table to include/sphrt.h: every entry that takes a stream is
declared by a row or exempted with a reason.

A row names its path, the recipe and parameters that build it, the C entries (sphrt_*) its gated
run must reach, whether its result is bitwise reproducible (else which bound of the owning test
file holds), and whether it is documented as free of host synchronisation:

  nosync 'return'    nothing is read back: the gate is still closed when the call returns
         'readback'  the call ends in `readbacks` documented Tensor.cpu() calls and the gate is
                     closed at the first
         None        documented with a sync (table builds, the deterministic weighted gradient's
                     max|ray_scale|, construction, per-call uploads), or no claim
  native 'fast'      the launches go through the CPython entry (csrc/fastpath.cpp), which calls
                     the C entries by address: the row counts the entry's hits instead
         'construct' likewise csrc/construct.cpp's build_cone
  after              the row's lazily built piece is used a second time on the default stream,
                     after wait_stream, and compared too

Shapes are the smallest the suite already uses for each route: gd_cases' circ16 / rect7, the cg
problems tiny / two_workgroups, the 5-view orbit of test_first_float64_use_on_side_stream (rect:
geometry order; circ: wedge order, the perm / gather binding), SPHRT_BRICK='2,4,4' over grid
(30, 21, 26) for brick staging, and test_gpu_adjoint_paths' dynamic pairing (5 views <-> 5
slices)."""
import collections
import functools
import math
import os
import re

import gd_cases as gc

Row = collections.namedtuple(
    'Row', 'name recipe params entries bitwise bound nosync readbacks native after mutated')


def _row(name, recipe, params, entries, bitwise=True, bound=None, nosync=None, readbacks=None,
         native=None, after=False, mutated=()):
    return Row(name, recipe, params, tuple(entries), bitwise, bound, nosync, readbacks, native,
               after, tuple(mutated))


SOLVE_ITERATIONS = 20
VARIANTS = [(False, None), (True, None), (False, True), (True, False)]   # test_gpu_cg.VARIANTS
OPERATORS = ['stored', 'matrix_free', 'matrix_free_deterministic']      # test_gpu_cg.OPERATORS

_TRANSPOSE_BUILD = ['sphrt_csr_transpose', 'sphrt_csr_index', 'sphrt_csr_local_build',
                    'sphrt_csr_local_pack']
_CONSTRUCT_ONE_PASS = ['sphrt_trace_bound', 'sphrt_scan_counts', 'sphrt_trace_emit',
                       'sphrt_csr_index_staged', 'sphrt_csr_local_build_staged',
                       'sphrt_csr_local_pack']


def _stored_rows():
    rows = []
    for dt in ('f32', 'f64'):
        first = ['sphrt_forward_' + dt] + (['sphrt_trace_compact'] if dt == 'f64' else [])
        rows.append(_row(f'stored-forward-{dt}-first', 'stored',
                         dict(geom='rect5', op='forward', dtype=dt, warm=0), first,
                         nosync='return'))
        rows.append(_row(f'stored-forward-{dt}-bound', 'stored',
                         dict(geom='rect5', op='forward', dtype=dt, warm=2),
                         ['sphrt_forward_' + dt], nosync='return', native='fast'))
        rows.append(_row(f'stored-T-transpose-{dt}-bound', 'stored',
                         dict(geom='rect5', op='T', dtype=dt, warm=2),
                         ['sphrt_forward_' + dt], nosync='return', native='fast'))
        rows.append(_row(f'stored-reordered-T-{dt}-bound', 'stored',
                         dict(geom='circ5', op='T', dtype=dt, warm=2),
                         ['sphrt_gather_' + dt, 'sphrt_forward_' + dt], nosync='return',
                         native='fast'))
        rows.append(_row(f'stored-T-atomic-{dt}', 'stored',
                         dict(geom='rect5', op='T', dtype=dt, warm=0, mode='atomic'),
                         ['sphrt_adjoint_accumulate', 'sphrt_trace_compact']
                         + (['sphrt_f64_to_f32'] if dt == 'f32' else []),
                         bitwise=False, bound='atomic_adjoint', nosync='return'))
    # lazily built: the transposed CSR, first on the side stream, then on the default stream
    rows.append(_row('stored-T-transpose-f64-first', 'stored',
                     dict(geom='rect5', op='T', dtype='f64', warm=0),
                     _TRANSPOSE_BUILD + ['sphrt_forward_f64', 'sphrt_trace_compact'], after=True))
    rows.append(_row('stored-reordered-T-f64-first', 'stored',
                     dict(geom='circ5', op='T', dtype='f64', warm=0),
                     _TRANSPOSE_BUILD + ['sphrt_gather_f64', 'sphrt_forward_f64'], after=True))
    rows.append(_row('stored-reordered-forward-f64-first', 'stored',
                     dict(geom='circ5', op='forward', dtype='f64', warm=0),
                     ['sphrt_forward_f64', 'sphrt_trace_compact'], nosync='return'))
    rows.append(_row('stored-backward-f64', 'stored',
                     dict(geom='rect5', op='backward', dtype='f64', warm=1),
                     ['sphrt_forward_f64']))
    rows.append(_row('stored-first-f64-after-f32', 'stored',
                     dict(geom='circ5', op='first64', dtype='f64', warm=0),
                     ['sphrt_trace_compact', 'sphrt_forward_f64', 'sphrt_gather_f64']
                     + _TRANSPOSE_BUILD, after=True))
    # brick staging: the per-call stage of the forward and of the bound call
    for warm in (0, 2):
        rows.append(_row(f'stored-brick-forward-f32-{"bound" if warm else "first"}', 'stored',
                         dict(geom='brick6', op='forward', dtype='f32', warm=warm,
                              env={'SPHRT_BRICK': '2,4,4'}),
                         ['sphrt_forward_f32'], nosync='return', native='fast' if warm else None))
    return rows


def _dynamic_rows():
    rows = [
        # lazily built: the time-paired copy (and its dense transpose), then the default stream
        _row('dynamic-forward-first', 'dynamic', dict(op='forward', warm=0),
             ['sphrt_csr_time_columns', 'sphrt_csr_local_build', 'sphrt_csr_local_pack',
              'sphrt_forward_f64', 'sphrt_trace_compact'], after=True),
        _row('dynamic-forward-bound', 'dynamic', dict(op='forward', warm=2),
             ['sphrt_forward_f64'], nosync='return', native='fast'),
        _row('dynamic-gradient-first', 'dynamic', dict(op='grad', warm=0),
             ['sphrt_csr_time_columns', 'sphrt_csr_transpose', 'sphrt_csr_index_dense',
              'sphrt_csr_local_build', 'sphrt_csr_local_pack', 'sphrt_forward_f64'], after=True),
        _row('dynamic-gradient-bound', 'dynamic', dict(op='grad', warm=2),
             ['sphrt_forward_f64'], native='fast'),
        _row('dynamic-T-time-slices-first', 'dynamic', dict(op='T', warm=0),
             ['sphrt_csr_time_columns', 'sphrt_csr_transpose', 'sphrt_csr_index_dense',
              'sphrt_forward_f64'], after=True),
        _row('dynamic-T-time-slices-bound', 'dynamic', dict(op='T', warm=2),
             ['sphrt_forward_f64'], nosync='return', native='fast'),
    ]
    return rows


def _construct_rows():
    circ16 = dict(geom='circ16')
    return [
        _row('construct-native-tiled', 'construct', dict(circ16, kind='stored'),
             ['sphrt_rays_cone_tiled'] + _CONSTRUCT_ONE_PASS, native='construct', after=True),
        _row('construct-native-wedges', 'construct', dict(geom='circ5', kind='stored'),
             ['sphrt_rays_cone_ordered'] + _CONSTRUCT_ONE_PASS, native='construct', after=True),
        _row('construct-python-tiled', 'construct',
             dict(circ16, kind='stored', env={'SPHRT_CONSTRUCT': 'python'}),
             ['sphrt_rays_cone_tiled'] + _CONSTRUCT_ONE_PASS, after=True),
        _row('construct-python-wedges', 'construct',
             dict(geom='circ5', kind='stored', env={'SPHRT_CONSTRUCT': 'python'}),
             ['sphrt_rays_cone_ordered'] + _CONSTRUCT_ONE_PASS, after=True),
        _row('construct-python-rect', 'construct',
             dict(geom='rect7', kind='stored', env={'SPHRT_CONSTRUCT': 'python'}),
             ['sphrt_rays_cone'] + _CONSTRUCT_ONE_PASS, after=True),
        _row('construct-two-pass-trace', 'construct',
             dict(geom='rect7', kind='stored', env={'SPHRT_TRACE': 'twopass'}),
             ['sphrt_trace_count', 'sphrt_scan_counts', 'sphrt_trace_fill', 'sphrt_csr_index',
              'sphrt_csr_local_build', 'sphrt_csr_local_pack'], after=True),
        _row('construct-two-pass-tables', 'construct',
             dict(geom='rect7', kind='stored', env={'SPHRT_TABLES': 'twopass'}),
             ['sphrt_trace_compact', 'sphrt_csr_index', 'sphrt_csr_local_count',
              'sphrt_csr_local_fill'], after=True),
        _row('construct-run-records', 'construct',
             dict(geom='rect7', kind='stored', env={'SPHRT_RUNS': 'on'}),
             ['sphrt_csr_runs'], after=True),
        _row('construct-float32-trace', 'construct', dict(geom='rect7', kind='stored_f32'),
             ['sphrt_rays_cone', 'sphrt_trace_reference_emit', 'sphrt_scan_counts',
              'sphrt_trace_compact', 'sphrt_csr_index', 'sphrt_csr_local_build'], after=True),
        _row('construct-matrix-free', 'construct', dict(geom='rect7', kind='mf'),
             ['sphrt_rays_cone'], after=True),
    ]


_NORMAL = {'square': 'sphrt_trace_normal', 'weights': 'sphrt_trace_normal_weighted',
           'abs': 'sphrt_trace_normal_robust', 'huber': 'sphrt_trace_normal_robust'}


def _mf_rows():
    rows = [
        # (the functions build their plan, rays and start bins per call: host uploads, a sync)
        _row('mf-line-integrals', 'mf', dict(op='line_integrals'),
             ['sphrt_rays_cone', 'sphrt_trace_integrate_f64']),
        _row('mf-back-project-atomic', 'mf', dict(op='back_project', det=False),
             ['sphrt_rays_cone', 'sphrt_trace_backproject_f64'], bitwise=False,
             bound='atomic_adjoint'),
        _row('mf-back-project-deterministic', 'mf', dict(op='back_project', det=True),
             ['sphrt_fixed_scale_f64', 'sphrt_trace_backproject_fixed_f64',
              'sphrt_fixed_finalize_f64']),
        _row('mf-call-f64', 'mf', dict(op='call'), ['sphrt_trace_integrate_f64'],
             nosync='return'),
        _row('mf-call-f32', 'mf', dict(op='call', dtype='f32'), ['sphrt_trace_integrate_f32'],
             nosync='return'),
        _row('mf-T-atomic', 'mf', dict(op='T', det=False), ['sphrt_trace_backproject_f64'],
             bitwise=False, bound='atomic_adjoint', nosync='return'),
        _row('mf-T-atomic-f32', 'mf', dict(op='T', det=False, dtype='f32'),
             ['sphrt_trace_backproject_f64', 'sphrt_f64_to_f32'], bitwise=False,
             bound='atomic_adjoint_f32', nosync='return'),
        _row('mf-T-deterministic', 'mf', dict(op='T', det=True),
             ['sphrt_fixed_scale_f64', 'sphrt_trace_backproject_fixed_f64',
              'sphrt_fixed_finalize_f64'], nosync='return'),
        _row('mf-backward-atomic', 'mf', dict(op='backward', det=False),
             ['sphrt_trace_integrate_f64', 'sphrt_trace_backproject_f64'], bitwise=False,
             bound='atomic_adjoint'),
        _row('mf-backward-deterministic', 'mf', dict(op='backward', det=True),
             ['sphrt_trace_integrate_f64', 'sphrt_trace_backproject_fixed_f64']),
    ]
    for loss in ('square', 'weights', 'abs', 'huber', 'poisson'):
        for det in (False, True):
            if loss == 'poisson':
                entries = ['sphrt_trace_integrate_f64', 'sphrt_poisson_residual_f64',
                           'sphrt_fixed_scale_f64', 'sphrt_trace_backproject_fixed_f64',
                           'sphrt_fixed_finalize_f64'] if det else \
                    ['sphrt_trace_normal_poisson_f64']
            else:
                entries = [_NORMAL[loss] + ('_fixed_f64' if det else '_f64')]
                if det:
                    entries += ['sphrt_fixed_scale_f64', 'sphrt_fixed_finalize_f64']
            # the deterministic weighted form reads max|ray_scale| back: documented with a sync
            nosync = None if (det and loss == 'weights') else 'return'
            rows.append(_row(f'mf-residual-gradient-{loss}-{"deterministic" if det else "atomic"}',
                             'mf', dict(op='resgrad', det=det, loss=loss), entries,
                             bitwise=det, bound=None if det else 'atomic_adjoint',
                             nosync=nosync))
    return rows


def _smooth_rows():
    return [_row('smooth-regularizer-value-and-backward', 'smooth', dict(),
                 ['sphrt_smooth_reg_f64'])]


def gd_entries(case):
    """The C entries a direct run of the case reaches (test_gpu_gd_matrix.expected_entries'
    rule, the entries with a count > 0), and the ctypes forward of the stored loops' adjoint."""
    kind = {'square': 'sq' if case.M == 'unit' else 'wsq', 'abs': 'robust', 'huber': 'robust',
            'poisson': 'poisson'}[case.F]
    want = [f'sphrt_{kind}_residual_f64']
    if case.R in ('smooth', 'both'):
        want.append('sphrt_smooth_reg_f64')
    elif case.R == 'neg' and case.P == 'sgd':
        want.append('sphrt_neg_reg_f64')
    if case.P == 'adam_fused':
        want.append('sphrt_adam_neg_f64')
    elif case.P != 'sgd':
        want.append('sphrt_adam_foreach_neg_f64')
    if case.O.startswith('mf'):
        want.append('sphrt_trace_integrate_f64')
        det = case.O == 'mf_deterministic'
        if case.F == 'poisson' and det:
            want += ['sphrt_trace_backproject_fixed_f64', 'sphrt_fixed_scale_f64',
                     'sphrt_fixed_finalize_f64']
        else:
            trace = {'sq': 'normal', 'wsq': 'normal_weighted'}.get(kind, 'normal_' + kind)
            want.append(f'sphrt_trace_{trace}{"_fixed" if det else ""}_f64')
            if det:
                want += ['sphrt_fixed_scale_f64', 'sphrt_fixed_finalize_f64']
    else:
        want.append('sphrt_forward_f64')
    return want


def _gd_synced(case):
    """The deterministic weighted gradient's max|ray_scale|: one readback before the loop."""
    return case.F == 'square' and case.M != 'unit' and case.O == 'mf_deterministic'


def _gd_rows():
    rows = []
    for case in gc.CASES:
        atomic = case.O == 'mf_atomic'
        rows.append(_row('gd-' + case.name, 'gd', dict(case=case.name), gd_entries(case),
                         bitwise=not atomic, bound='gd' if atomic else None,
                         nosync=None if _gd_synced(case) else 'readback', readbacks=1,
                         mutated=('c0',)))
    # lazily built: the loop's trace-position rows (a reordered trace), and the loop-staged
    # descriptor of a brick-staged forward; first use behind the gate, then the default stream
    rows.append(_row('gd-loop-rows-first', 'gd_lazy', dict(geom='circ16', optim='sgd'),
                     ['sphrt_forward_f64', 'sphrt_sq_residual_f64'] + _TRANSPOSE_BUILD,
                     after=True, mutated=('c0',)))
    rows.append(_row('gd-loop-staged-brick', 'gd_lazy',
                     dict(geom='brick6', optim='adam', env={'SPHRT_BRICK': '2,4,4'}),
                     ['sphrt_forward_f64', 'sphrt_sq_residual_f64',
                      'sphrt_adam_foreach_neg_f64'], after=True, mutated=('c0',)))
    return rows


def _solve_rows():
    rows = []
    cases = [('tiny', v, k) for v in VARIANTS for k in OPERATORS] + \
        [('two_workgroups', VARIANTS[3], 'stored')]
    for solver in ('cg', 'fista'):
        for problem, (masked, wrap), kind in cases:
            fused, det = kind != 'stored', kind == 'matrix_free_deterministic'
            if fused:
                entries = ['sphrt_trace_normal' + ('_weighted' if masked else '')
                           + ('_fixed_f64' if det else '_f64'), 'sphrt_trace_integrate_f64']
            else:
                entries = ['sphrt_wsq_residual_f64' if masked else 'sphrt_sq_residual_f64',
                           'sphrt_forward_f64']
            if wrap is not None:
                entries.append('sphrt_smooth_reg_f64')
            entries += ['sphrt_cg_curvature_f64', 'sphrt_cg_update_f64',
                        'sphrt_cg_direction_f64'] if solver == 'cg' else \
                ['sphrt_pg_step_f64', 'sphrt_pg_momentum_f64']
            atomic = kind == 'matrix_free'
            name = (f'{solver}-{problem}-{"masked" if masked else "unit"}-'
                    f'{"nosmooth" if wrap is None else "ring" if wrap else "open"}-{kind}')
            rows.append(_row(name, 'solve',
                             dict(solver=solver, problem=problem, masked=masked, wrap=wrap,
                                  kind=kind),
                             entries, bitwise=not atomic, bound='solve' if atomic else None,
                             # (masked and deterministic: max|ray_scale| is read back first)
                             nosync=None if (masked and det) else 'readback', readbacks=1))
    return rows


ROWS = (_stored_rows() + _dynamic_rows() + _construct_rows() + _mf_rows() + _smooth_rows()
        + _gd_rows() + _solve_rows())
BY_NAME = {r.name: r for r in ROWS}
NAMES = [r.name for r in ROWS]

# Stream-taking entries no row reaches, each with the reason.
EXEMPT = {
    'sphrt_exact_sort_lists':
        'test hook of the exact path\'s sorts (test_gpu_exact_sort.py): no package caller',
    'sphrt_fixed_accumulate_f64':
        'test hook of the trace\'s device add (test_gpu_fixed_kernels.py): no package caller',
    'sphrt_trace_reference':
        'count / fill fallback of the reference-mode trace, taken only when n * K staging slots '
        'exceed 40 % of free device memory: not reachable at a test\'s size',
    'sphrt_solve':
        'r_torch / e_torch / a_torch: host inputs copied up and the result copied down inside the '
        'call (synchronous by contract); no device input a gate could hold back',
    'sphrt_solve_f32': 'as sphrt_solve',
}


def stream_entries(header=None):
    """Every entry of include/sphrt.h whose parameter list ends in `void *stream`."""
    if header is None:
        header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                              'include', 'sphrt.h')
    with open(header) as fh:
        src = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    return [m.group(1) for m in
            re.finditer(r'\b(sphrt_\w+)\s*\(([^;{()]*?)void\s*\*\s*stream\s*\)\s*;', src)]


# ---- recipes: operators and inputs (everything below runs on the GPU machine only) ----------------
def _orbit(n_views, det, kind, grid_shape):
    import torch as tr
    from sph_raytracer_amd import ConeCircGeom, ConeRectGeom, SphericalGrid
    grid = SphericalGrid(shape=grid_shape)
    geoms = []
    for th in tr.linspace(0, 2 * tr.pi, n_views):
        pos = (5 * tr.cos(th), 5 * tr.sin(th), 1)
        geoms.append(ConeRectGeom(det, pos=pos, fov=(45, 45)) if kind == 'rect'
                     else ConeCircGeom(shape=det, pos=pos, fov=(0, 45)))
    return grid, sum(geoms)


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(grid, geom) on the CPU."""
    if name in ('circ16', 'rect7'):
        return gc.geometry(name)
    if name == 'rect5':
        return _orbit(5, (24, 30), 'rect', (20, 17, 22))
    if name == 'circ5':
        return _orbit(5, (24, 30), 'circ', (20, 17, 22))
    if name == 'brick6':
        return _orbit(6, (24, 30), 'rect', (30, 21, 26))
    if name == 'dynamic':      # test_gpu_adjoint_paths' D: 5 views <-> 5 time slices
        import torch as tr
        from sph_raytracer_amd import ConeCircGeom, SphericalGrid
        grid = SphericalGrid(shape=(5, 12, 10, 16))
        geom = sum(ConeCircGeom((24, 16), pos=(5 * tr.cos(th), 5 * tr.sin(th), 1), fov=(0, 12))
                   for th in tr.linspace(0, 2 * tr.pi, 5))
        return grid, geom
    raise KeyError(name)


def _rand(shape, dtype, seed, gpu, lo=0.0):
    import torch as tr
    g = tr.Generator().manual_seed(seed)
    return (lo + tr.rand(tuple(shape), dtype=tr.float64, generator=g)).to(dtype).to(gpu)


def _dtype(params):
    import torch as tr
    return tr.float32 if params.get('dtype') == 'f32' else tr.float64


class Recipe:
    """setup(row, gpu) -> ctx (operators built and warmed on the default stream);
    inputs(row, ctx, gpu) -> {name: true values}; call(row, ctx, **inputs) -> a list of
    tensors and lists of floats; after(row, ctx, **inputs) the second use (Row.after)."""


class Stored(Recipe):
    @staticmethod
    def setup(row, gpu):
        from sph_raytracer_amd import Operator
        p = row.params
        grid, geom = geometry(p['geom'])
        op = Operator(grid, geom, device=gpu)
        op.adjoint_mode = p.get('mode', 'transpose')
        ctx = dict(op=op, grid=grid, geom=geom, hits=[])
        dt = _dtype(p)
        if p['geom'] == 'brick6':
            assert op._csr['desc'].stage_shape[0] > 0
        if p['geom'] == 'circ5':
            assert op._csr['ray_id'] is not None and not op._tcols_geom()
        if p['op'] == 'first64':
            op(_rand(grid.shape, dt, 1, gpu).float())     # float32 first: the lengths stay staged
            assert dict.__getitem__(op._csr, 'len') is None
        for k in range(p['warm']):
            Stored.call(row, ctx, **{n: _rand(v.shape, v.dtype, 50 + k, gpu)
                                     for n, v in Stored.inputs(row, ctx, gpu).items()})
        ctx['hits'].clear()
        return ctx

    @staticmethod
    def inputs(row, ctx, gpu):
        p, dt = row.params, _dtype(row.params)
        x = _rand(ctx['grid'].shape, dt, 3, gpu)
        y = _rand(ctx['geom'].shape, dt, 4, gpu)
        return {'forward': dict(x=x), 'T': dict(y=y), 'backward': dict(x=x, w=y),
                'first64': dict(x=x, y=y)}[p['op']]

    @staticmethod
    def call(row, ctx, x=None, y=None, w=None):
        op, kind = ctx['op'], row.params['op']
        fast = getattr(op, '_fastfn', None)
        if fast is not None:           # count the CPython entry's hits

            def counted(*a):
                out = fast(*a)
                ctx['hits'].append(out is not None)
                return out
            op._fastfn = counted
        try:
            if kind == 'forward':
                return [op(x)]
            if kind == 'T':
                return [op.T(y)]
            if kind == 'first64':
                return [op(x), op.T(y)]
            leaf = x.detach().requires_grad_()
            out = op(leaf)
            out.backward(w)
            return [out.detach(), leaf.grad]
        finally:
            if fast is not None:
                op._fastfn = fast

    after = call


class Dynamic(Recipe):
    @staticmethod
    def setup(row, gpu):
        from sph_raytracer_amd import Operator
        grid, geom = geometry('dynamic')
        op = Operator(grid, geom, dynamic=True, device=gpu)
        ctx = dict(op=op, grid=grid, geom=geom, hits=[])
        for k in range(row.params['warm']):
            Dynamic.call(row, ctx, **{n: _rand(v.shape, v.dtype, 60 + k, gpu)
                                      for n, v in Dynamic.inputs(row, ctx, gpu).items()})
        ctx['hits'].clear()
        return ctx

    @staticmethod
    def inputs(row, ctx, gpu):
        import torch as tr
        x = _rand(ctx['grid'].shape, tr.float64, 5, gpu)
        y = _rand(ctx['geom'].shape, tr.float64, 6, gpu)
        return {'forward': dict(x=x), 'T': dict(y=y), 'grad': dict(x=x, w=y)}[row.params['op']]

    @staticmethod
    def call(row, ctx, x=None, y=None, w=None):
        op, kind = ctx['op'], row.params['op']
        fast = getattr(op, '_fastfn', None)
        if fast is not None:

            def counted(*a):
                out = fast(*a)
                ctx['hits'].append(out is not None)
                return out
            op._fastfn = counted
        try:
            if kind == 'forward':
                return [op(x)]
            if kind == 'T':
                return [op.T(y, time_slices=True)]
            leaf = x.detach().requires_grad_()
            out = op(leaf)
            out.backward(w)
            return [out.detach(), leaf.grad]
        finally:
            if fast is not None:
                op._fastfn = fast

    after = call


class Construct(Recipe):
    """call: the construction itself (nothing returned: there is no value input to hold back);
    after: the CSR arrays and a forward / adjoint on the default stream."""

    @staticmethod
    def setup(row, gpu):
        grid, geom = geometry(row.params['geom'])
        return dict(grid=grid, geom=geom, gpu=gpu, hits=[])

    @staticmethod
    def inputs(row, ctx, gpu):
        return {}

    @staticmethod
    def call(row, ctx):
        import torch as tr
        from sph_raytracer_amd import MatrixFreeOperator, Operator, _lib
        kind, gpu = row.params['kind'], ctx['gpu']
        fc = _lib.load_construct()
        real = fc.build_cone if fc is not None else None
        if real is not None:

            def build_cone(*a):
                res = real(*a)
                ctx['hits'].append(res is not None)
                return res
            fc.build_cone = build_cone
        try:
            if kind == 'mf':
                ctx['op'] = MatrixFreeOperator(ctx['grid'], ctx['geom'], device=gpu)
            else:
                ctx['op'] = Operator(ctx['grid'], ctx['geom'], device=gpu,
                                     ftype=tr.float32 if kind == 'stored_f32' else tr.float64)
        finally:
            if real is not None:
                fc.build_cone = real
        return []

    @staticmethod
    def after(row, ctx):
        import torch as tr
        op = ctx['op']
        x = _rand(ctx['grid'].shape, tr.float64, 7, ctx['gpu'])
        y = _rand(ctx['geom'].shape, tr.float64, 8, ctx['gpu'])
        out = [op(x)]
        if row.params['kind'] == 'mf':
            op.deterministic = True
            return out + [op.T(y)]
        csr = op._csr
        out += [op.T(y), op(x.float())]
        # (the arrays up to the segment total: what lies past it is never written or read)
        total = csr['total']
        out += [csr['row_ptr'], csr['vox'][:total], csr['len32'][:total], csr['loc'][:total]]
        return out + list(op.segments())


class MatrixFree(Recipe):
    @staticmethod
    def setup(row, gpu):
        from sph_raytracer_amd import MatrixFreeOperator
        grid, geom = geometry('rect7')
        op = MatrixFreeOperator(grid, geom, device=gpu,
                                deterministic=bool(row.params.get('det')))
        return dict(op=op, grid=grid, geom=geom, hits=[])

    @staticmethod
    def inputs(row, ctx, gpu):
        import torch as tr
        p, dt = row.params, _dtype(row.params)
        x = _rand(ctx['grid'].shape, dt, 9, gpu, lo=0.25)
        y = _rand(ctx['geom'].shape, dt, 10, gpu, lo=0.25)
        if p['op'] in ('line_integrals', 'call'):
            return dict(x=x)
        if p['op'] in ('back_project', 'T'):
            return dict(y=y)
        if p['op'] == 'backward':
            return dict(x=x, w=y)
        ins = dict(x=x, m=y)
        if p['loss'] == 'weights':
            ins['weights'] = _rand(ctx['geom'].shape, tr.float64, 11, gpu, lo=0.1)
        return ins

    @staticmethod
    def call(row, ctx, x=None, y=None, w=None, m=None, weights=None):
        from sph_raytracer_amd.raytracer import back_project, line_integrals
        p, op = row.params, ctx['op']
        if p['op'] == 'line_integrals':
            return [line_integrals(ctx['grid'], ctx['geom'], x)]
        if p['op'] == 'back_project':
            return [back_project(ctx['grid'], ctx['geom'], y, deterministic=p['det'])]
        if p['op'] == 'call':
            return [op(x)]
        if p['op'] == 'T':
            return [op.T(y)]
        if p['op'] == 'backward':
            leaf = x.detach().requires_grad_()
            out = op(leaf)
            out.backward(w)
            return [out.detach(), leaf.grad]
        kw = {'square': {}, 'weights': dict(weights=weights), 'abs': dict(loss='abs'),
              'huber': dict(loss='huber', delta=0.3),
              'poisson': dict(loss='poisson', eps=0.1)}[p['loss']]
        return list(op.residual_gradient(x, m, 0.7, **kw))


class Smooth(Recipe):
    @staticmethod
    def setup(row, gpu):
        from sph_raytracer_amd.loss import SmoothRegularizer
        grid, _ = geometry('rect7')
        return dict(grid=grid, reg=SmoothRegularizer(weights=(1, 0.5, 2), kind='huber', delta=0.25,
                                                     wrap_a=True), hits=[])

    @staticmethod
    def inputs(row, ctx, gpu):
        import torch as tr
        return dict(d=_rand(ctx['grid'].shape, tr.float64, 12, gpu))

    @staticmethod
    def call(row, ctx, d):
        leaf = d.detach().requires_grad_()
        val = ctx['reg'].compute(None, None, leaf, leaf)
        val.backward()
        return [val.detach().reshape(1), leaf.grad]


_GD_OPERATORS = {}


def _gd_operator(geom_name, fused, gpu, fresh=False):
    from sph_raytracer_amd import MatrixFreeOperator, Operator
    key = (geom_name, fused, str(gpu))
    if fresh or key not in _GD_OPERATORS:
        grid, geom = geometry(geom_name)
        op = (MatrixFreeOperator if fused else Operator)(grid, geom, device=gpu)
        if fresh:
            return op
        _GD_OPERATORS[key] = op
    return _GD_OPERATORS[key]


class Gd(Recipe):
    """retrieval.gd on the case's device tensors as the gate hands them in (gd_cases.run_gd
    copies from the host, which would wait out the spin)."""

    @staticmethod
    def setup(row, gpu):
        case = gc.BY_NAME[row.params['case']]
        for var in ('SPHRT_RAY_ORDER', 'SPHRT_TCOLS'):
            assert var not in os.environ
        fused = case.O.startswith('mf')
        op = _gd_operator(case.geometry, fused, gpu)
        if fused:
            op.deterministic = case.O == 'mf_deterministic'
        return dict(op=op, case=case, gpu=gpu, hits=[])

    @staticmethod
    def inputs(row, ctx, gpu):
        inp = gc.inputs(ctx['case'])
        ins = dict(y=inp.y.to(gpu), c0=inp.c0.to(gpu))
        if not isinstance(inp.mask, int):
            ins['mask'] = inp.mask.to(gpu)
        return ins

    @staticmethod
    def call(row, ctx, y, c0, mask=1):
        from sph_raytracer_amd import retrieval
        from sph_raytracer_amd.model import FullyDenseModel
        case, op = ctx['case'], ctx['op']
        fns, _ = gc.terms(case, mask, ctx['gpu'])
        optim, kw = gc.optimiser(case)
        try:
            c, yhat, hist = retrieval.gd(op, y, FullyDenseModel(op.grid), coeffs=c0,
                                         num_iterations=gc.N_IT, loss_fns=fns, optim=optim,
                                         progress_bar=False, **kw)
        except RuntimeError:
            # every total NaN: gd has no best iterate and evaluates f(None), as the reference
            # does.  Hand the NaN back, for the comparison to report it
            import torch as tr
            if not bool(tr.isnan(c0.detach()).any()):
                raise
            return [c0.detach(), tr.full_like(y.detach(), float('nan'))] + \
                [[float('nan')] * gc.N_IT for _ in fns]
        assert c is c0
        return [c.detach(), yhat.detach()] + [list(hist[fn]) for fn in fns]


class GdLazy(Recipe):
    """A fresh stored operator whose first gd loop (3 iterations, a plain SquareLoss) runs
    behind the gate and whose second runs on the default stream."""

    @staticmethod
    def setup(row, gpu):
        p = row.params
        op = _gd_operator(p['geom'], False, gpu, fresh=True)
        if p['geom'] == 'brick6':
            assert op._csr['desc'].stage_shape[0] > 0
        else:
            assert op._adjoint_trace_order() is not None
        return dict(op=op, gpu=gpu, hits=[])

    @staticmethod
    def inputs(row, ctx, gpu):
        import torch as tr
        op = ctx['op']
        return dict(y=_rand(op.geom.shape, tr.float64, 13, gpu),
                    c0=_rand(op.grid.shape, tr.float64, 14, gpu, lo=0.5))

    @staticmethod
    def call(row, ctx, y, c0):
        import torch as tr
        from sph_raytracer_amd import retrieval
        from sph_raytracer_amd.loss import SquareLoss
        from sph_raytracer_amd.model import FullyDenseModel
        op, fn = ctx['op'], SquareLoss()
        optim, kw = (tr.optim.SGD, dict(lr=1.0, momentum=0.9)) if row.params['optim'] == 'sgd' \
            else (tr.optim.Adam, dict(lr=0.03))
        c, yhat, hist = retrieval.gd(op, y, FullyDenseModel(op.grid), coeffs=c0, num_iterations=3,
                                     loss_fns=[fn], optim=optim, progress_bar=False, **kw)
        return [c.detach().clone(), yhat.detach(), list(hist[fn])]

    @staticmethod
    def after(row, ctx, y, c0):
        return GdLazy.call(row, ctx, y, c0.clone())


@functools.lru_cache(maxsize=None)
def _problem(name, gpu):
    """test_gpu_cg._problem: (grid, geom, the stored Operator, y, mask), and a damp that bounds
    the condition number without the dense system: N = A^T diag(s) A + G + (2 damp / V) I with
    |A^T diag(s) A| <= max(s) * max row sum * max column sum of A (norm interpolation), so
    2 damp / V of that product keeps the data term's share of the condition number under 2."""
    import torch as tr
    from sph_raytracer_amd import ConeRectGeom, Operator, SphericalGrid
    F64 = tr.float64
    if name == 'tiny':
        grid = SphericalGrid(shape=(4, 3, 6))
        geom = ConeRectGeom((6, 6), pos=(5, 0.3, 1), fov=(25, 25)) + \
            ConeRectGeom((6, 6), pos=(-1, 4.5, -2), fov=(25, 25))
    else:
        grid = SphericalGrid(shape=(5, 6, 10))
        geom = ConeRectGeom((257, 1), pos=(4, 1, 0.5), fov=(50, 1))
    op = Operator(grid, geom, device=gpu)
    g = tr.Generator().manual_seed(11)
    truth = tr.rand(tuple(grid.shape), dtype=F64, generator=g).to(gpu)
    y = op(truth).detach()
    y = y + 0.01 * tr.randn(y.shape, dtype=F64, generator=g).to(gpu)
    mask = (tr.rand(y.shape, dtype=F64, generator=g) + 0.25).to(gpu)
    mask.view(-1)[3] = 0.0
    rows = float(op(tr.ones(tuple(grid.shape), dtype=F64, device=gpu)).max())
    cols = float(op.T(tr.ones(y.shape, dtype=F64, device=gpu)).max())
    lmax = 2 * 1.5 / y.numel() * 1.25 * rows * cols
    damp = lmax * math.prod(grid.shape) / 2
    return grid, geom, op, y, mask, damp


@functools.lru_cache(maxsize=None)
def _solve_operator(name, kind, gpu):
    from sph_raytracer_amd import MatrixFreeOperator
    grid, geom, op, _, _, _ = _problem(name, gpu)
    if kind == 'stored':
        return op
    return MatrixFreeOperator(grid, geom, device=gpu,
                              deterministic=kind == 'matrix_free_deterministic')


class Solve(Recipe):
    @staticmethod
    def setup(row, gpu):
        p = row.params
        grid, _, _, y, mask, damp = _problem(p['problem'], gpu)
        return dict(op=_solve_operator(p['problem'], p['kind'], gpu), grid=grid, y=y, mask=mask,
                    damp=damp, gpu=gpu, hits=[])

    @staticmethod
    def inputs(row, ctx, gpu):
        import torch as tr
        ins = dict(y=ctx['y'], x0=tr.full(tuple(ctx['grid'].shape), 0.5, dtype=tr.float64,
                                          device=gpu))
        if row.params['masked']:
            ins['mask'] = ctx['mask']
        return ins

    @staticmethod
    def call(row, ctx, y, x0, mask=1):
        from sph_raytracer_amd import retrieval
        from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
        p = row.params
        fns = [1.5 * SquareLoss(projection_mask=mask)]
        if p['wrap'] is not None:
            fns.append(0.3 * SmoothRegularizer(weights=(1, 0.5, 2), wrap_a=p['wrap']))
        if p['solver'] == 'cg':
            x, yhat, info = retrieval.cg(ctx['op'], y, loss_fns=fns, x0=x0, damp=ctx['damp'],
                                         num_iterations=SOLVE_ITERATIONS)
            return [x, yhat, list(info['residual'])]
        x, yhat, info = retrieval.fista(ctx['op'], y, loss_fns=fns, x0=x0, damp=ctx['damp'],
                                        num_iterations=SOLVE_ITERATIONS, lower=0.0, upper=0.9)
        return [x, yhat, list(info['residual']), [float(v) for v in info['restarts']],
                [info['lipschitz']]]


RECIPES = {'stored': Stored, 'dynamic': Dynamic, 'construct': Construct, 'mf': MatrixFree,
           'smooth': Smooth, 'gd': Gd, 'gd_lazy': GdLazy, 'solve': Solve}
