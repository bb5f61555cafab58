"""Host side of chambolle_pock's diagonal preconditioning (retrieval.chambolle_pock(precondition=
'diagonal'); csrc/loss.hip's three entries declared in include/sphrt_dp.h): the header, the
bindings and the library's exports agree and none of it leaks into the other headers or their
tables; the stream-order rows of dp_stream_cases reach every entry; the keyword is validated by
name; on dense systems from the CPU oracle's matrix the steps satisfy Pock and Chambolle's lemma
(|S^1/2 K T^1/2| <= 1 by SVD) and Condat's condition with the damping term's share
(T^-1 - K^T S K - c I >= 0), a voxel no ray crosses and a ray that misses the grid get +0.0 steps
and stay where they start; the generic (plain torch) path closes cp_cases' duality gap on every
case of cp_cases.solver_cases() within cp_cases.GAP_LIMIT after dp_cases.ITERATIONS iterations;
and precondition=None still gives, bit for bit, what the commit before this keyword computed
(tests/golden/dp_none_bits.npz).  (No compute call of the library.)"""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch as tr

import cp_cases as cp
import dp_cases as dc
import pd_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = tr.float64
VP, INT, DBL, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64
OTHER_HEADERS = ('sphrt.h', 'sphrt_pd.h', 'sphrt_cp.h')


def _header(name):
    with open(os.path.join(ROOT, 'include', name)) as fh:
        return fh.read()


def _declared(name):
    hdr = re.sub(r'/\*.*?\*/', '', _header(name), flags=re.S)
    return sorted(set(re.findall(r'\b(sphrt_[a-z0-9_]+)\s*\(', hdr)))


def test_header_bindings_and_exports_agree():
    from sph_raytracer_amd import _lib, build
    build.build()
    declared = _declared('sphrt_dp.h')
    assert declared == ['sphrt_dp_primal_f64', 'sphrt_dp_ray_dual_f64', 'sphrt_dp_steps_f64']
    assert sorted(_lib.DP_EXPORTED) == declared, 'ctypes bindings out of sync with sphrt_dp.h'
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name in declared:
        assert hasattr(raw, name), f'{name} declared in include/sphrt_dp.h but not exported'
        for other in OTHER_HEADERS:
            assert name not in _header(other)
        assert name not in _lib.EXPORTED + _lib.PD_EXPORTED + _lib.CP_EXPORTED
        assert getattr(lib, name).restype is ctypes.c_int
    assert 'sphrt_dp' not in ''.join(_header(h) for h in OTHER_HEADERS)
    hdr = re.sub(r'/\*.*?\*/', '', _header('sphrt_dp.h'), flags=re.S)
    for name, _, argtypes in _lib._DP_SIGNATURES:
        m = re.search(r'int\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr)
        args = [' '.join(a.split()) for a in m.group(1).split(',')]
        assert len(args) == len(argtypes) and args[-1] == 'void *stream', name
        for a, ct in zip(args, argtypes):
            want = VP if '*' in a else INT if a.startswith('int ') else \
                I64 if a.startswith('int64_t ') else DBL
            assert ct is want, (name, a)
        assert list(getattr(lib, name).argtypes) == argtypes
    # the two entries that restate older ones take exactly their arguments
    sig = {s[0]: s[2] for s in _lib._PD_SIGNATURES + _lib._CP_SIGNATURES + _lib._DP_SIGNATURES}
    assert sig['sphrt_dp_primal_f64'] == sig['sphrt_pd_primal_f64']
    assert sig['sphrt_dp_ray_dual_f64'] == sig['sphrt_cp_ray_dual_f64']
    assert 'sphrt_dp.h' in open(build.__file__).read()


def test_every_stream_entry_of_the_header_has_a_row():
    import dp_stream_cases as dsc
    import stream_cases as sc
    entries = sc.stream_entries(os.path.join(ROOT, 'include', 'sphrt_dp.h'))
    assert sorted(entries) == _declared('sphrt_dp.h')
    assert all(set(entries) <= set(row.entries) for row in dsc.ROWS) and dsc.ROWS
    known = set(entries) | set(sc.stream_entries())
    for other in OTHER_HEADERS[1:]:
        known |= set(sc.stream_entries(os.path.join(ROOT, 'include', other)))
    assert all(e in known for row in dsc.ROWS for e in row.entries)
    assert len({row.name for row in dsc.ROWS}) == len(dsc.ROWS)
    assert {row.params['kind'] for row in dsc.ROWS} == set(sc.OPERATORS)


def test_refusals_on_the_host():
    """Every refusal of the three entries returns non-zero with its word in sphrt_last_error
    before any launch: the pointers (small fake addresses) are never dereferenced."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    nan, inf = float('nan'), float('inf')
    P = [VP(1 << 24 | 65536 * k) for k in range(1, 13)]
    shape, n = (5, 7, 9), 315

    def primal(shape=shape, lower=0.0, upper=1.0, **kw):
        a = dict(zip(('x', 'g', 'q', 'xn', 'tau', 'mm'), P))
        a.update(kw)
        return lib.sphrt_dp_primal_f64(a['x'], a['g'], a['q'], a['xn'], *shape, 1, 1, 1, 1, 0.5,
                                       a['tau'], lower, upper, a['mm'], None)

    names = ('z', 'o', 'y', 's', 'w', 'sg', 'order', 'p', 'padj', 'pp', 'fid')

    def ray(n=300, kind=2, par=0.5, **kw):
        a = dict(zip(names, P))
        a.update(kw)
        return lib.sphrt_dp_ray_dual_f64(a['z'], a['o'], a['y'], 1, n, kind, par, a['s'], a['w'],
                                         a['sg'], a['order'], a['p'], a['padj'], a['pp'], a['fid'],
                                         None)

    def steps(shape=shape, n_ray=300, rho=0.5, c=0.0, **kw):
        a = dict(zip(('col', 'row', 'order', 'tau', 'sigma'), P))
        a.update(kw)
        return lib.sphrt_dp_steps_f64(a['col'], a['row'], n_ray, *shape, 1, 1, 1, 1, rho, c,
                                      a['order'], a['tau'], a['sigma'], None)

    at = dict(zip(names, P))
    cases = []
    for fn in (primal, steps):
        cases += [(fn, dict(shape=s), b'axis') for s in ((0, 7, 9), (5, -1, 9), (5, 7, 0))]
        cases += [(fn, dict(shape=(2 ** 11, 2 ** 10, 2 ** 10)), b'2^31')]
    cases += [(primal, {k: None}, b'null') for k in ('x', 'g', 'q', 'xn', 'tau', 'mm')]
    cases += [(primal, dict(lower=nan), b'bound'), (primal, dict(lower=1.0), b'bound'),
              (primal, dict(xn=P[0]), b'alias'), (primal, dict(xn=P[1]), b'alias'),
              # tau is n long here: its last element against the output's first
              (primal, dict(xn=VP(P[4].value + 8 * (n - 1))), b'alias'),
              (primal, dict(mm=VP(P[4].value + 8 * (n - 1))), b'alias')]
    cases += [(ray, dict(n=0), b'empty'), (ray, dict(kind=4), b'kind'), (ray, dict(kind=-1), b'kind')]
    cases += [(ray, {k: None}, b'null') for k in names]
    cases += [(ray, dict(kind=k, par=v), word) for k, word in ((2, b'delta'), (3, b'eps'))
              for v in (nan, 0.0, -1.0, inf)]
    cases += [(ray, dict(padj=at['p']), b'alias'), (ray, dict(p=at['z']), b'alias'),
              # sigma is n long here: its last element against an output's first
              (ray, dict(p=VP(at['sg'].value + 8 * 299)), b'alias'),
              (ray, dict(pp=VP(at['sg'].value + 8 * 299)), b'alias')]
    cases += [(steps, {k: None}, b'null') for k in ('col', 'row', 'tau', 'sigma')]
    cases += [(steps, dict(n_ray=v), b'n_ray') for v in (0, -3, 2 ** 31)]
    cases += [(steps, dict(rho=v), b'rho') for v in (0.0, -0.0, -1.0, nan, inf, -inf)]
    cases += [(steps, dict(c=v), b'c must') for v in (-1.0, nan, inf)]
    cases += [(steps, dict(tau=P[0]), b'alias'), (steps, dict(sigma=P[1]), b'alias'),
              (steps, dict(sigma=P[3]), b'alias'), (steps, dict(tau=VP(P[2].value + 4 * 299)), b'alias'),
              (steps, dict(sigma=VP(P[0].value + 8 * (n - 1))), b'alias')]
    for i, (fn, kw, word) in enumerate(cases):
        assert fn(**kw) != 0, (i, fn.__name__, kw)
        assert word in lib.sphrt_last_error(), (i, fn.__name__, kw, lib.sphrt_last_error())


# ---- the keyword ---------------------------------------------------------------------------------------
def test_precondition_is_validated_by_name():
    from sph_raytracer_amd.loss import AbsLoss, PoissonLoss, SmoothRegularizer
    from sph_raytracer_amd.retrieval import chambolle_pock
    from test_cp_cpu import _Shape
    par = list(inspect.signature(chambolle_pock).parameters.values())
    assert par[-1].name == 'precondition' and par[-1].default is None
    y, f = tr.zeros(2, 6, 6, dtype=F64), _Shape((4, 3, 6))
    for bad in ('jacobi', 'Diagonal', '', True, 1, 0.0, ['diagonal'], tr.tensor(1.0)):
        for fns in ([AbsLoss()], [PoissonLoss(), cp.tv_term()]):
            with pytest.raises(ValueError, match='chambolle_pock needs precondition.*'
                                                 + re.escape(repr(bad))):
                chambolle_pock(f, y, fns, precondition=bad)      # (before the operator is used)
    with pytest.raises(ValueError, match="chambolle_pock.*'diagonal'.*norm=5.0"):
        chambolle_pock(f, y, [AbsLoss()], precondition='diagonal', norm=5.0)
    # the older refusals still come first or alongside, in their own words
    with pytest.raises(ValueError, match='chambolle_pock needs.*dual_ratio'):
        chambolle_pock(f, y, [AbsLoss()], precondition='diagonal', dual_ratio=0.0)
    with pytest.raises(ValueError, match='time_weight'):
        chambolle_pock(_Shape((2, 4, 3, 6)), y,
                       [AbsLoss(), 0.1 * SmoothRegularizer(kind='abs', time_weight=1.0)],
                       precondition='diagonal')


# ---- the lemma on dense systems ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lemma():
    return dc.lemma_problem()


def _shipped_steps(op, y, wrap, tv, rho, damp):
    """(tau per column, sigma per row of K = [A; D]) as chambolle_pock itself forms them: info of
    a solve of zero iterations through the generic path over the CpuOperator, rho set through
    dual_ratio (rho = dual_ratio lam / M), sigma_tv repeated over D's rows."""
    from sph_raytracer_amd.retrieval import chambolle_pock
    fns = [cp.fidelity('abs')] + ([cp.tv_term(wrap)] if tv else [])
    _, _, info = chambolle_pock(op, y, fns, num_iterations=0, damp=damp, lower=0.0, upper=None,
                                dual_ratio=rho * y.numel() / cp.LAM_F, precondition='diagonal')
    assert info['norm'] is None and info['tau'].shape == tuple(op.grid.shape)
    assert info['sigma'].shape == y.shape and isinstance(info['sigma_tv'], float)
    return (info['tau'].numpy().reshape(-1), info['sigma'].numpy().reshape(-1), info['sigma_tv'])


@pytest.mark.parametrize('tv', [False, True], ids=['notv', 'tv'])
@pytest.mark.parametrize('wrap', [False, True], ids=['open', 'ring'])
def test_the_steps_satisfy_the_lemma_and_condat_s_condition(lemma, wrap, tv):
    """tau, sigma and sigma_tv as chambolle_pock returns them in info (`_shipped_steps`), against
    the dense K = [A; D] of the oracle's matrix and pd_cases' difference matrix: the lemma's norm
    by SVD, Condat's condition by eigenvalues, and the values themselves against |K|'s sums."""
    op, A = lemma
    assert (A >= 0).all()
    K, n_ray = dc.dense_k(A, dc.LEMMA_SHAPE, wrap, tv)
    V, n_edge = K.shape[1], len(K) - n_ray
    y = tr.ones(tuple(op.geom.shape), dtype=F64)
    # the brute-force edge count is |D|'s column sum, and every edge row sums to 2
    if tv:
        has = [w > 0 for w in pc.TV_WEIGHTS]
        assert np.array_equal(np.abs(K[n_ray:]).sum(axis=0), dc.degree(dc.LEMMA_SHAPE, wrap, has))
        assert np.all(np.abs(K[n_ray:]).sum(axis=1) == 2.0)
        assert dc.degree(dc.LEMMA_SHAPE, wrap, has).max() == 6
        assert n_edge == (5 * 24 + 6 * 3 * 6 + (24 * 6 if wrap else 24 * 5))
    norms = []
    for rho in dc.LEMMA_RHO:
        for damp in dc.LEMMA_DAMP:
            c = 2 * damp / V
            tau, sigma_ray, sigma_tv = _shipped_steps(op, y, wrap, tv, rho, damp)
            assert tau.shape == (V,) and sigma_ray.shape == (n_ray,)
            sigma = np.concatenate([sigma_ray, np.full(n_edge, sigma_tv)])
            # the values: |K|'s row and column sums in numpy (dual_ratio carries rho with one
            # rounding each way: 4 ulp)
            want_tau, want_sigma = dc.dense_steps(K, n_ray, rho, c)
            assert np.allclose(tau, want_tau, rtol=1e-14, atol=0)
            assert np.allclose(sigma, want_sigma, rtol=1e-14, atol=0)
            assert np.array_equal(tau == 0, want_tau == 0)
            assert np.array_equal(sigma == 0, want_sigma == 0)
            assert not np.signbit(tau).any() and not np.signbit(sigma).any()
            M = np.sqrt(sigma)[:, None] * K * np.sqrt(tau)[None, :]
            norm = np.linalg.svd(M, compute_uv=False)[0]
            live = tau > 0
            t_inv = np.where(live, 1.0 / np.where(live, tau, 1.0), 0.0)
            # on the voxels something acts on (the others never move: their row and column of
            # K^T S K are zero as well, and c is 0 there by the guard's own condition)
            C = (np.diag(t_inv) - K.T @ (sigma[:, None] * K) - c * np.eye(V))[np.ix_(live, live)]
            low = np.linalg.eigvalsh((C + C.T) / 2)[0]
            print(f'wrap {wrap} tv {tv} rho {rho:.3g} damp {damp}: norm {norm:.16g}, smallest '
                  f'eigenvalue {low:.3g} of |T^-1| {t_inv.max():.3g}')
            assert norm <= 1 + 1e-12
            assert low >= -1e-12 * t_inv.max()
            if damp == 0:
                norms.append(norm)
                # (without TV and damping the dead voxels and rays of this problem are among
                # the steps checked)
                assert tv or ((tau == 0).any() and (sigma_ray == 0).any())
    # rho cancels from the norm when c = 0
    assert len(norms) == len(dc.LEMMA_RHO) and np.allclose(norms, norms[0], rtol=1e-12)


def test_a_voxel_without_rays_and_a_ray_without_voxels_stay_put(lemma):
    """The lemma problem has voxels no ray crosses and rays that miss the grid: without TV and
    damping tau is +0.0 there and x keeps its (clamped) start; sigma is +0.0 on the rays that
    miss, whose dual stays +0.0 — with a positive count under the abs kind, where a scalar sigma
    would drive it to the clamp."""
    from sph_raytracer_amd.retrieval import chambolle_pock
    op, A = lemma
    row, col = A.sum(axis=1), A.sum(axis=0)
    dead_v, dead_r = col == 0, row == 0
    assert 0 < dead_v.sum() < len(col) and 0 < dead_r.sum() < len(row)
    g = tr.Generator().manual_seed(5)
    x0 = tr.rand(dc.LEMMA_SHAPE, dtype=F64, generator=g)
    y = op(tr.rand(dc.LEMMA_SHAPE, dtype=F64, generator=g)).detach() + 0.5
    for kind in cp.KINDS:
        x, _, info = chambolle_pock(op, y, [cp.fidelity(kind)], x0=x0, num_iterations=50,
                                    lower=0.0, upper=None, precondition='diagonal')
        tau, sigma = info['tau'].numpy().reshape(-1), info['sigma'].numpy().reshape(-1)
        assert tau.shape == col.shape and sigma.shape == row.shape
        assert info['tau'].shape == x.shape and info['sigma'].shape == y.shape
        assert info['norm'] is None and info['sigma_tv'] == cp.LAM_F / y.numel() / 2
        for v, dead in ((tau, dead_v), (sigma, dead_r)):
            assert not v[dead].any() and not np.signbit(v[dead]).any() and np.all(v[~dead] > 0)
        rho = cp.LAM_F / y.numel()
        assert np.allclose(sigma[~dead_r], rho / row[~dead_r], rtol=1e-14)
        assert np.allclose(tau[~dead_v], 1 / (rho * col[~dead_v]), rtol=1e-14)
        xn, pn = x.numpy().reshape(-1), info['ray_dual'].numpy().reshape(-1)
        assert np.array_equal(xn[dead_v], x0.numpy().reshape(-1)[dead_v])
        assert not np.array_equal(xn[~dead_v], x0.numpy().reshape(-1)[~dead_v])
        assert not pn[dead_r].any() and not np.signbit(pn[dead_r]).any()
        assert pn[~dead_r].any()
    # with TV every voxel has an edge, with damping every voxel a curvature: tau > 0 throughout
    for kw, fns in ((dict(damp=0.05), [cp.fidelity('abs')]),
                    (dict(), [cp.fidelity('abs'), cp.tv_term()])):
        _, _, info = chambolle_pock(op, y, fns, num_iterations=1, precondition='diagonal', **kw)
        assert bool((info['tau'] > 0).all())


# ---- the generic solver --------------------------------------------------------------------------------
CASES = cp.solver_cases()


@pytest.mark.parametrize('case', CASES, ids=[cp.case_id(c) for c in CASES])
def test_generic_path_closes_the_duality_gap(case):
    name, kind, tv, masked, damp, lower, upper = case
    op, y, mask, A = cp.problem(name)
    x, y_hat, info = dc.solve_case(case)
    assert x.shape == tuple(op.grid.shape) and x.dtype == F64 and not x.requires_grad
    assert tr.equal(y_hat, op(x)) and y_hat.shape == y.shape
    J, D, gap = cp.gap_of(case, x, info)
    print(f'{cp.case_id(case)}: J {J:.6g}, D {D:.6g}, gap {gap:.3g} (scalar steps, recorded at '
          f'{cp.ITERATIONS}: {cp.MEASURED[cp.case_id(case)]:.3g})')
    assert D <= J + cp.WEAK_DUALITY_SLACK * abs(J)              # weak duality
    assert gap <= cp.GAP_LIMIT[kind]
    # the iterate properties
    xn = x.numpy().reshape(-1)
    assert np.all(xn >= lower) and (upper is None or np.all(xn <= upper))
    s, _ = cp.ray_factors(y, mask, masked)
    p = info['ray_dual'].numpy().reshape(-1)
    b = {'abs': s, 'huber': s * cp.HUBER_DELTA}.get(kind)
    assert b is None or np.all(np.abs(p) <= b)
    assert kind != 'poisson' or np.all(p <= s)
    assert not p[s == 0].any() and not np.signbit(p[s == 0]).any()
    if tv:
        q = info['dual'].numpy().reshape(3, -1)
        cax = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS) / xn.size
        assert all(np.abs(q[ax]).max() <= cax[ax] for ax in range(3))
    else:
        assert info['dual'] is None and info['dual_change'] == [0.0] * dc.ITERATIONS
    for key in ('primal_change', 'dual_change', 'ray_dual_change', 'fidelity'):
        assert len(info[key]) == dc.ITERATIONS and all(math.isfinite(v) for v in info[key])
    assert math.isclose(info['fidelity'][-1], cp.phi(kind, s, y.numpy().reshape(-1), A @ xn).sum(),
                        rel_tol=1e-10)
    # the steps: the issue's formulas on the dense matrix
    rho, c = cp.LAM_F / y.numel(), 2 * damp / xn.size
    has = [w > 0 for w in pc.TV_WEIGHTS]
    deg = dc.degree(tuple(op.grid.shape), True, has) if tv else 0.0
    assert info['norm'] is None and info['sigma_tv'] == rho / 2
    assert info['tau'].shape == x.shape and info['sigma'].shape == y.shape
    row, col = A.sum(axis=1), A.sum(axis=0)
    want_sigma = np.where(row > 0, rho / np.where(row > 0, row, 1.0), 0.0)
    assert np.allclose(info['sigma'].numpy().reshape(-1), want_sigma, rtol=1e-12, atol=0)
    d = rho * (col + deg) + c
    want_tau = np.where(d > 0, 1 / np.where(d > 0, d, 1.0), 0.0)
    assert np.allclose(info['tau'].numpy().reshape(-1), want_tau, rtol=1e-12, atol=0)


def test_precondition_none_gives_the_recorded_bits():
    """precondition=None (given or left out) is the code path as it was: x, p, q and the four
    histories of dp_cases.GOLDEN_CASES, bit for bit against the values recorded from the commit
    before the keyword (under dp_cases.ieee_sqrt, and without the Poisson kind's fidelity
    history: torch's CPU sqrt and log are not the same bits on every host, see dp_cases)."""
    want = np.load(os.path.join(ROOT, 'tests', 'golden', dc.GOLDEN_FILE))
    for kw in ({}, dict(precondition=None)):
        got = dc.golden_arrays(**kw)
        assert sorted(got) == sorted(want.files) and len(got) == 28
        for key, v in got.items():
            assert v.dtype == np.float64 and v.shape == want[key].shape, key
            assert np.array_equal(v.view(np.int64), want[key].view(np.int64)), key
    # and 'diagonal' is another iteration: the bits differ
    other = dc.golden_arrays(precondition='diagonal')
    assert not any(np.array_equal(other[k], want[k]) for k in want.files if k.endswith('/x'))


def test_the_tv_paths_give_the_recorded_bits():
    """`primal_dual` with the abs and the iso term, `chambolle_pock` with the iso term and with
    precondition='diagonal': x, the duals, the histories and the steps of
    dp_cases.tv_golden_arrays, bit for bit against the values recorded before the TV term's
    plumbing was folded (tests/golden/tv_paths_bits.npz; the same rules as the record above)."""
    want = np.load(os.path.join(ROOT, 'tests', 'golden', dc.TV_GOLDEN_FILE))
    got = dc.tv_golden_arrays()
    assert sorted(got) == sorted(want.files)
    paths = {k.split('-')[0] + '-' + k.split('-')[1] for k in got}
    assert paths == {'pd-abs', 'pd-iso', 'cp-iso', 'cp-diag'}
    for key, v in got.items():
        assert v.dtype == np.float64 and v.shape == want[key].shape, key
        assert np.array_equal(v.view(np.int64), want[key].view(np.int64)), key


def test_other_inputs_solve_on_the_generic_path():
    """A float32 start runs in its dtype, zero iterations return the clamped start with the
    steps, and a dynamic operator (TV over each slice's r, e, a) closes its own gap."""
    from cpu_operator import CpuOperator
    from sph_raytracer_amd import SphericalGrid
    from sph_raytracer_amd.retrieval import chambolle_pock
    case = ('tiny', 'huber', True, True, cp.DAMP, cp.LOWER, cp.UPPER)
    op, y, mask, A = cp.problem('tiny')
    want = dc.solve_case(case)[0]
    x32, _, i32 = dc.solve_case(case, x0=tr.zeros(4, 3, 6, dtype=tr.float32))
    assert x32.dtype == tr.float32 and i32['tau'].dtype == tr.float32
    assert i32['tau'].shape == x32.shape and i32['sigma'].shape == y.shape
    # (float32 rounding 6e-8 at a condition number under 1e3: test_cp_cpu's bound)
    assert float((x32.double() - want).abs().max()) <= 1e-4
    x0 = tr.linspace(-1, 2, 72, dtype=F64).reshape(4, 3, 6)
    xz, _, iz = chambolle_pock(op, y, cp.terms('huber', True, mask), x0=x0, num_iterations=0,
                               lower=cp.LOWER, upper=cp.UPPER, precondition='diagonal',
                               power_iterations=1)
    assert tr.equal(xz, x0.clamp(cp.LOWER, cp.UPPER)) and iz['norm'] is None
    assert iz['primal_change'] == [] and not iz['ray_dual'].any() and not iz['dual'].any()
    assert bool((iz['tau'] > 0).all())
    dgrid = SphericalGrid(shape=(2, 4, 3, 6))
    dop = CpuOperator(dgrid, op.geom)
    g = tr.Generator().manual_seed(3)
    yd = dop(tr.rand(tuple(dgrid.shape), dtype=F64, generator=g)).detach().clamp(min=0.0)
    xt, yh, info = chambolle_pock(dop, yd, cp.terms('abs', True), damp=cp.DAMP, lower=cp.LOWER,
                                  upper=cp.UPPER, num_iterations=dc.ITERATIONS,
                                  precondition='diagonal')
    assert xt.shape == tuple(dgrid.shape) and info['tau'].shape == xt.shape
    assert info['sigma'].shape == yd.shape and info['dual'].shape == (3,) + tuple(dgrid.shape)
    cols = []
    for i in range(144):
        e = tr.zeros(144, dtype=F64)
        e[i] = 1.0
        cols.append(dop(e.reshape(2, 4, 3, 6)).reshape(-1))
    Ad = tr.stack(cols, dim=1).numpy()
    D1, c1, up = cp.tv_edges((4, 3, 6), True)
    edges = (np.kron(np.eye(2), D1), np.tile(c1, 2) / 2, up)     # (V doubles: c halves)
    s = np.full(yd.numel(), cp.LAM_F / yd.numel())
    q = np.concatenate([cp.flat_dual(info['dual'][:, k], up) for k in range(2)])
    xn, yn = xt.numpy().reshape(-1), yd.numpy().reshape(-1)
    J = cp.primal_value('abs', Ad, s, yn, edges, cp.DAMP, xn)
    D = cp.dual_value('abs', Ad, s, yn, edges, cp.DAMP, cp.LOWER, cp.UPPER,
                      info['ray_dual'].numpy().reshape(-1), q)
    print(f'dynamic abs: J {J:.6g}, D {D:.6g}, gap {(J - D) / abs(J):.3g}')
    assert D <= J + cp.WEAK_DUALITY_SLACK * abs(J) and (J - D) / abs(J) <= cp.GAP_LIMIT['abs']
