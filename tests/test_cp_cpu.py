"""Host side of the Chambolle-Pock solver (retrieval.chambolle_pock; csrc/loss.hip's ray-dual
entry, declared in include/sphrt_cp.h): the header, the bindings and the library's exports agree
and none of it leaks into sphrt.h, sphrt_pd.h or their tables; the stream-order rows of
cp_stream_cases reach the entry; its refusals fire on the host; chambolle_pock refuses bad terms
and arguments by name before the operator is used; the proxes of the generic path satisfy
p in d phi(z) on cp_cases' draws within the recorded bound; the restatement's fma is an fma; and
the generic (plain torch) path over the oracle-backed CpuOperator closes the duality gap —
J(x_K) and D(p_K, q_K) recomputed from the dense matrix without the solver — within
cp_cases.GAP_LIMIT on every case, agrees with a projected-gradient minimiser in numpy for the
smooth kinds (through that run's own lower bound, not the solver's dual), brackets a linear
programme's optimum for the undamped abs cases, and solves over a dynamic operator and from a float32 start.  (No compute call of
the library.)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch as tr

import cp_cases as cp
import cp_stream_cases as csc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = tr.float64
VP, INT, DBL, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64


def _header(name):
    with open(os.path.join(ROOT, 'include', name)) as fh:
        return fh.read()


def _declared(name):
    return sorted(set(re.findall(r'\b(sphrt_[a-z0-9_]+)\s*\(', _header(name))))


def test_header_bindings_and_exports_agree():
    from sph_raytracer_amd import _lib, build
    build.build()
    declared = _declared('sphrt_cp.h')
    assert declared == ['sphrt_cp_ray_dual_f64']
    assert sorted(_lib.CP_EXPORTED) == declared, 'ctypes bindings out of sync with sphrt_cp.h'
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name in declared:
        assert hasattr(raw, name), f'{name} declared in include/sphrt_cp.h but not exported'
        for other in ('sphrt.h', 'sphrt_pd.h'):
            assert name not in _declared(other) and name not in _header(other)
        assert name not in _lib.EXPORTED and name not in _lib.PD_EXPORTED
        assert getattr(lib, name).restype is ctypes.c_int
    hdr = re.sub(r'/\*.*?\*/', '', _header('sphrt_cp.h'), flags=re.S)
    for name, _, argtypes in _lib._CP_SIGNATURES:
        m = re.search(r'int\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr)
        args = [' '.join(a.split()) for a in m.group(1).split(',')]
        assert len(args) == len(argtypes) and args[-1] == 'void *stream', name
        for a, ct in zip(args, argtypes):
            want = VP if '*' in a else INT if a.startswith('int ') else \
                I64 if a.startswith('int64_t ') else DBL
            assert ct is want, (name, a)
        assert list(getattr(lib, name).argtypes) == argtypes
    # the kinds' numbers: the header's, the bindings' and cp_cases'
    ids = dict(re.findall(r'#define SPHRT_CP_([A-Z]+) (\d)', _header('sphrt_cp.h')))
    assert {k.lower(): int(v) for k, v in ids.items()} == cp.KIND_ID
    assert (_lib.CP_SQUARE, _lib.CP_ABS, _lib.CP_HUBER, _lib.CP_POISSON) == (0, 1, 2, 3)
    from sph_raytracer_amd import build as b
    assert 'sphrt_cp.h' in open(b.__file__).read()


def test_every_stream_entry_of_the_header_has_a_row():
    import stream_cases as sc
    entries = sc.stream_entries(os.path.join(ROOT, 'include', 'sphrt_cp.h'))
    assert sorted(entries) == _declared('sphrt_cp.h')
    assert all(set(entries) <= set(row.entries) for row in csc.ROWS) and csc.ROWS
    known = set(entries) | set(sc.stream_entries()) | set(
        sc.stream_entries(os.path.join(ROOT, 'include', 'sphrt_pd.h')))
    assert all(e in known for row in csc.ROWS for e in row.entries)
    assert len({row.name for row in csc.ROWS}) == len(csc.ROWS)
    assert {row.params['fidelity'] for row in csc.ROWS} == set(cp.KINDS)
    assert {row.params['tv'] for row in csc.ROWS} == {False, True}
    assert {row.params['kind'] for row in csc.ROWS} == set(sc.OPERATORS)


def test_refusals_on_the_host():
    """Every refusal returns non-zero with its word in sphrt_last_error before any launch: the
    pointers (small fake addresses) are never dereferenced."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    ptrs = [VP(1 << 24 | 65536 * k) for k in range(1, 12)]
    names = ('z', 'o', 'y', 's', 'w', 'sg', 'order', 'p', 'padj', 'pp', 'fid')
    nan, inf = float('nan'), float('inf')

    def call(n=300, kind=2, par=0.5, y_f64=1, **kw):
        a = dict(zip(names, ptrs))
        a.update(kw)
        return lib.sphrt_cp_ray_dual_f64(a['z'], a['o'], a['y'], y_f64, n, kind, par, a['s'], a['w'],
                                         a['sg'], a['order'], a['p'], a['padj'], a['pp'], a['fid'],
                                         None)

    cases = [(dict(n=0), b'empty'), (dict(n=-1), b'empty'), (dict(kind=-1), b'kind'),
             (dict(kind=4), b'kind'), (dict(kind=17), b'kind')]
    cases += [({k: None}, b'null') for k in names]
    cases += [(dict(kind=k, par=v), word) for k, word in ((2, b'delta'), (3, b'eps'))
              for v in (nan, 0.0, -0.0, -1.0, inf, -inf)]
    p, padj, z, pp = (ptrs[names.index(k)] for k in ('p', 'padj', 'z', 'pp'))
    cases += [(dict(padj=p), b'alias'), (dict(padj=VP(p.value + 8 * 299)), b'alias'),
              (dict(p=VP(padj.value + 8 * 299)), b'alias'), (dict(p=z), b'alias'),
              (dict(fid=pp), b'alias'), (dict(fid=VP(pp.value + 8)), b'alias'),
              (dict(pp=VP(z.value + 8 * 299)), b'alias')]
    for i, (kw, word) in enumerate(cases):
        assert call(**kw) != 0, (i, kw)
        assert word in lib.sphrt_last_error(), (i, kw, lib.sphrt_last_error())


# ---- chambolle_pock's refusals ---------------------------------------------------------------------
class _Shape:
    """A shape-only stand-in: any use of the operator itself raises AttributeError."""

    def __init__(self, shape):
        self.grid = self
        self.shape = shape
        self.a_b = None


def test_chambolle_pock_refuses_bad_terms_and_arguments():
    import sph_raytracer_amd as pkg
    from sph_raytracer_amd.loss import (AbsLoss, HuberLoss, NegRegularizer, PoissonLoss,
                                        SmoothRegularizer, SquareLoss, SquareRelLoss)
    from sph_raytracer_amd.retrieval import chambolle_pock
    assert 'chambolle_pock' in pkg.__all__ and pkg.chambolle_pock is chambolle_pock
    y = tr.zeros(2, 6, 6, dtype=F64)
    f = _Shape((4, 3, 6))
    tv = lambda **kw: 0.1 * SmoothRegularizer(kind='abs', **kw)       # noqa: E731

    class MyLoss(AbsLoss):
        pass
    bad = [([tv()], 'needs one SquareLoss, AbsLoss, HuberLoss or PoissonLoss'), ([], 'needs one'),
           ([AbsLoss(), PoissonLoss()], 'one fidelity term, not two'),
           ([AbsLoss(), SquareLoss()], 'one fidelity term, not two'),
           ([AbsLoss(), SmoothRegularizer()], "kind='square'"),
           ([AbsLoss(), SmoothRegularizer(kind='huber', delta=1.0)], "'huber'"),
           ([AbsLoss(), tv(), tv()], 'at most one SmoothRegularizer'),
           ([AbsLoss(), NegRegularizer()], 'NegRegularizer'), ([MyLoss()], 'MyLoss'),
           ([SquareRelLoss()], 'SquareRelLoss'),
           ([0.0 * AbsLoss()], 'lam > 0'), ([-1.0 * HuberLoss()], 'lam > 0'),
           ([tr.tensor(2.0) * PoissonLoss()], 'lam > 0'), ([float('inf') * SquareLoss()], 'lam > 0'),
           ([AbsLoss(), 0.0 * SmoothRegularizer(kind='abs')], 'lam > 0'),
           ([AbsLoss(use_grad=False)], 'use_grad'), ([AbsLoss(), tv(use_grad=False)], 'use_grad'),
           ([AbsLoss(volume_mask=2)], 'volume_mask'), ([AbsLoss(), tv(volume_mask=2)], 'volume_mask'),
           ([AbsLoss(projection_mask=2)], 'projection_mask'),
           ([AbsLoss(projection_mask=tr.ones(5))], 'projection_mask'),
           ([AbsLoss(), tv(projection_mask=tr.ones(2, 6, 6, dtype=F64))], 'projection_mask'),
           ([AbsLoss(), tv(weights=(0, 0, 0))], 'no edges')]
    for fns, word in bad:
        with pytest.raises(ValueError, match='chambolle_pock.*' + word):
            chambolle_pock(f, y, fns)                 # (refused before the operator is used)
    with pytest.raises(ValueError, match='no edges'):
        chambolle_pock(_Shape((4, 1, 6)), y, [AbsLoss(), tv(weights=(0, 1, 0))])
    with pytest.raises(ValueError, match='time_weight'):
        chambolle_pock(_Shape((2, 4, 3, 6)), y, [AbsLoss(), tv(time_weight=1.0)])
    with pytest.raises(ValueError, match='r, e, a'):
        chambolle_pock(f, y, [AbsLoss(), tv()], x0=tr.zeros(3, 6, dtype=F64))
    nan, inf = float('nan'), float('inf')
    for kw, word in ((dict(damp=-1.0), 'damp'), (dict(damp=nan), 'damp'),
                     (dict(num_iterations=-1), 'num_iterations'),
                     (dict(num_iterations=2.5), 'num_iterations'),
                     (dict(lower=nan), 'lower'), (dict(upper=nan), 'upper'),
                     (dict(lower='0'), 'lower'), (dict(upper=tr.tensor(1.0)), 'upper'),
                     (dict(lower=1.0, upper=1.0), 'lower < upper'),
                     (dict(lower=inf, upper=None), 'lower < upper'),
                     (dict(norm=0.0), 'norm'), (dict(norm=-1.0), 'norm'), (dict(norm=inf), 'norm'),
                     (dict(norm=nan), 'norm'), (dict(norm=tr.tensor(1.0)), 'norm'),
                     (dict(power_iterations=0), 'power_iterations'),
                     (dict(power_iterations=1.5), 'power_iterations'),
                     (dict(dual_ratio=0.0), 'dual_ratio'), (dict(dual_ratio=inf), 'dual_ratio'),
                     (dict(dual_ratio=nan), 'dual_ratio'), (dict(dual_ratio=True), 'dual_ratio'),
                     (dict(dual_ratio=tr.tensor(1.0)), 'dual_ratio')):
        for fns in ([AbsLoss()], [PoissonLoss(), tv()]):
            with pytest.raises(ValueError, match='chambolle_pock needs.*' + word):
                chambolle_pock(f, y, fns, **kw)
    with pytest.raises(ValueError, match='chambolle_pock needs measurements'):
        chambolle_pock(f, None, [AbsLoss()])
    # the other solvers still refuse these terms in their own words
    from sph_raytracer_amd.retrieval import fista
    with pytest.raises(ValueError, match='fista needs a quadratic total.*AbsLoss'):
        fista(None, y, loss_fns=[AbsLoss()])


# ---- the proxes ------------------------------------------------------------------------------------
def _prox(kind, a, sigma, s, y):
    from sph_raytracer_amd import retrieval
    return retrieval._cp_prox(cp.KIND_ID[kind], cp.par_of(kind),
                              *(tr.from_numpy(v) for v in (a, sigma, s, y))).numpy()


@pytest.mark.parametrize('kind', cp.KINDS)
def test_the_proxes_satisfy_their_optimality_condition(kind):
    """p = prox_{sigma phi*}(a) iff p in d phi((a - p) / sigma): checked on a few hundred draws
    per kind, s = 0, y = 0 and both sides of every clamp among them; the bound is 16 x the largest
    violation measured here (cp_cases.PROX_MEASURED, reproduced to a factor of two)."""
    a, sigma, s, y = cp.prox_draws(kind)
    assert (s == 0).sum() >= 8 and (y == 0).sum() >= 16 and len(a) >= 300
    p = _prox(kind, a, sigma, s, y)
    zero = s == 0
    assert not p[zero].any() and not np.signbit(p[zero]).any()
    v = cp.prox_violation(kind, a, sigma, s, y, p)
    print(f'{kind}: largest violation {v.max():.3g} (recorded {cp.PROX_MEASURED[kind]:.3g})')
    assert v.max() <= cp.PROX_BOUND[kind] and cp.PROX_BOUND[kind] == 16 * cp.PROX_MEASURED[kind]
    assert cp.PROX_MEASURED[kind] / 2 <= v.max() <= 2 * cp.PROX_MEASURED[kind]
    live = ~zero
    if kind in ('abs', 'huber'):      # both clamps and the inside occur
        b = s * (1.0 if kind == 'abs' else cp.HUBER_DELTA)
        assert (p[live] == b[live]).sum() >= 10 and (p[live] == -b[live]).sum() >= 10
        assert (np.abs(p[live]) < b[live]).sum() >= 30
    if kind == 'poisson':
        assert np.all(p <= s) and (p[live] < -10 * s[live]).any() and (p[live] > 0.9 * s[live]).any()
    # a wrong prox is seen: every p moved by 5 % of its scale
    wrong = p - 0.05 * (np.abs(p) + s)
    assert cp.prox_violation(kind, a, sigma, s, y, np.where(zero, p, wrong))[live].max() > \
        100 * cp.PROX_BOUND[kind]


def test_the_restatement_s_fma_is_an_fma_and_restates_the_generic_prox():
    g = tr.Generator().manual_seed(0)
    a, b, c = (tr.randn(4000, dtype=F64, generator=g)
               * 10.0 ** tr.randint(-3, 4, (4000,), generator=g).double() for _ in range(3))
    c[:2000] = -a[:2000] * b[:2000] + 1e-13 * c[:2000]          # (cancellation: the low part decides)
    exact = cp.fma_exact(a, b, c)
    assert tr.equal(cp.fma_eft(a, b, c), exact) and int((a * b + c != exact).sum()) > 1000
    # the restatement and the generic prox differ by roundings only, and ray_dual_ref's indexing
    # through `order` gives p_adj[j] = p[order[j]]
    for kind in cp.KINDS:
        av, sg, s, y = (tr.from_numpy(v) for v in cp.prox_draws(kind))
        n = len(av)
        sigma = 0.37
        zn, zo, p0 = tr.rand(n, dtype=F64, generator=g) + 0.1, tr.rand(n, dtype=F64, generator=g), \
            0.1 * tr.randn(n, dtype=F64, generator=g)
        order = tr.randperm(n, generator=g)
        pn, padj, tpp, tfid = cp.ray_dual_ref(kind, zn, zo, y, s, tr.ones(n, dtype=F64), sigma, p0,
                                              order=order)
        want = _prox(kind, (p0 + sigma * (2 * zn - zo)).numpy(), np.full(n, sigma), s.numpy(),
                     y.numpy())
        assert np.allclose(pn.numpy(), want, rtol=1e-9, atol=1e-12)
        assert tr.equal(padj, pn[order]) and tr.equal(tpp, ((pn - p0) ** 2)[order])
        plain, _, _, _ = cp.ray_dual_ref(kind, zn, zo, y, s, tr.ones(n, dtype=F64), sigma, p0)
        assert tr.equal(plain, pn)


# ---- the generic solver ------------------------------------------------------------------------------
CASES = cp.solver_cases()


def test_the_recorded_table_is_complete_and_the_limit_is_its():
    assert sorted(cp.MEASURED) == sorted(cp.case_id(c) for c in CASES)
    for kind in cp.KINDS:
        worst = 100 * max(v for k, v in cp.MEASURED.items() if f'-{kind}-' in k)
        assert worst <= cp.GAP_LIMIT[kind] <= 1.01 * max(worst, cp.GAP_FLOOR)
    assert sorted(cp.SENSITIVITY) == sorted(cp.gpu_cases())
    from sph_raytracer_amd import retrieval
    assert retrieval._CP_DUAL_RATIO == 1.0


@pytest.mark.parametrize('case', CASES, ids=[cp.case_id(c) for c in CASES])
def test_generic_path_closes_the_duality_gap(case):
    name, kind, tv, masked, damp, lower, upper = case
    op, y, mask, A = cp.problem(name)
    x, y_hat, info = cp.solve_case(case)
    assert x.shape == tuple(op.grid.shape) and x.dtype == F64 and not x.requires_grad
    assert tr.equal(y_hat, op(x)) and y_hat.shape == y.shape
    J, D, gap = cp.gap_of(case, x, info)
    rec = cp.MEASURED[cp.case_id(case)]
    print(f'{cp.case_id(case)}: J {J:.6g}, D {D:.6g}, gap {gap:.3g} (recorded {rec:.3g})')
    assert D <= J + cp.WEAK_DUALITY_SLACK * abs(J)              # weak duality
    assert gap <= cp.GAP_LIMIT[kind]
    # the primal value is the loss classes' own total
    import cg_cases as cc
    fns = cp.terms(kind, tv, mask if masked else 1)
    assert math.isclose(float(cc.total(op, y, fns, damp, x)), J, rel_tol=1e-12)
    # every iterate property of the result
    xn = x.numpy().reshape(-1)
    assert np.all(xn >= lower) and (upper is None or np.all(xn <= upper))
    s, _ = cp.ray_factors(y, mask, masked)
    p = info['ray_dual'].numpy().reshape(-1)
    assert info['ray_dual'].shape == y.shape
    b = {'abs': s, 'huber': s * cp.HUBER_DELTA}.get(kind)
    assert b is None or np.all(np.abs(p) <= b)
    assert kind != 'poisson' or np.all(p <= s)
    assert not p[s == 0].any() and not np.signbit(p[s == 0]).any()
    if tv:
        import pd_cases as pc
        q = info['dual'].numpy().reshape(3, -1)
        cax = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS) / xn.size
        assert all(np.abs(q[ax]).max() <= cax[ax] for ax in range(3))
    else:
        assert info['dual'] is None and info['dual_change'] == [0.0] * cp.ITERATIONS
    for key in ('primal_change', 'dual_change', 'ray_dual_change', 'fidelity'):
        assert len(info[key]) == cp.ITERATIONS and all(math.isfinite(v) for v in info[key])
    assert math.isclose(info['fidelity'][-1], cp.phi(kind, s, y.numpy().reshape(-1), A @ xn).sum(),
                        rel_tol=1e-10)
    # the steps: Kn^2 = L_A + B, sigma = sbar / Kn, 1 / tau = sigma Kn^2 + c
    LA, B = info['norm'], 12.0 if tv else 0.0
    assert np.linalg.norm(A, 2) ** 2 <= LA <= 1.31 * np.linalg.norm(A, 2) ** 2
    kn = math.sqrt(LA + B)
    assert math.isclose(info['sigma'], cp.LAM_F / y.numel() / kn, rel_tol=1e-12)
    assert math.isclose(1 / info['tau'], info['sigma'] * kn * kn + 2 * damp / xn.size, rel_tol=1e-12)
    # the smooth kinds without TV, damped: x_K against a long projected-gradient run in numpy,
    # without the solver's dual.  J is differentiable and c-strongly convex (c = 2 damp / V), so
    # at the numpy minimiser xg, J* >= LB = J(xg) + min over the box of <grad J(xg), x - xg> +
    # c/2 |x - xg|^2 (closed form per voxel), and |x - x*| <= sqrt(2 (J(x) - LB) / c) for any x
    # in the box: both points lie in such balls around the minimiser
    if not tv and damp and upper is not None and kind != 'abs':
        yn = y.numpy().reshape(-1)
        xg, LB = _projected_gradient(kind, A, s, yn, damp, lower, upper)
        c = 2 * damp / xn.size
        Jg = cp.primal_value(kind, A, s, yn, None, damp, xg)
        res = cp.GAP_FLOOR * abs(J)              # (what the recomputed values resolve)
        radius = math.sqrt(2 * max(J - LB, res) / c) + math.sqrt(2 * max(Jg - LB, res) / c)
        print(f'  projected gradient: J {Jg:.6g}, lower bound {LB:.6g}, distance '
              f'{np.linalg.norm(xn - xg):.3g}, radius {radius:.3g}')
        assert LB <= Jg      # (Jg - LB is what the numpy run has left; the radius carries it)
        assert D <= Jg + cp.WEAK_DUALITY_SLACK * abs(J)       # weak duality, independent primal
        assert np.linalg.norm(xn - xg) <= radius
    # the abs kind, undamped: a linear programme (scipy's HiGHS) gives J* without the solver:
    # D <= J* <= J(x_K) must hold, and the share of the gap that is primal is printed
    if kind == 'abs' and not damp:
        Js = _abs_lp(A, s, y.numpy().reshape(-1), cp.tv_edges(tuple(op.grid.shape), tv), lower,
                     upper)
        print(f'  linear programme: J* {Js:.8g}, (J - J*) / J* {(J - Js) / Js:.3g}, '
              f'(J* - D) / J* {(Js - D) / Js:.3g}')
        slack = 1e-9 * abs(Js)                   # (HiGHS' default optimality tolerances, 1e-7, on
        assert D <= Js + slack and Js <= J + slack   # an objective whose terms are ~1e-2 J*)


def _projected_gradient(kind, A, s, y, damp, lower, upper, iterations=20000):
    """argmin of sum phi_i((A x)_i) + damp mean(x^2) over the box by projected gradient with the
    step 1 / L, L from the largest curvature of phi on the box (numpy alone)."""
    par = cp.par_of(kind)
    c = 2 * damp / A.shape[1]
    if kind == 'poisson':            # (s y / (z + eps)^2, largest at the box's lower corner)
        z_lo = A @ np.full(A.shape[1], lower)
        curv = (s * y / (z_lo + par) ** 2)[y > 0].max()
    else:
        curv = 2 * s.max() if kind == 'square' else s.max()
    step = 1.0 / (np.linalg.norm(A, 2) ** 2 * curv + c)
    x = np.full(A.shape[1], lower)
    for _ in range(iterations):
        r = A @ x - y
        if kind == 'square':
            d = 2 * s * r
        elif kind == 'huber':
            d = s * np.clip(r, -par, par)
        else:
            d = s * (1 - y / (A @ x + par))
        x = np.clip(x - step * (A.T @ d + c * x), lower, upper)
    # the lower bound of strong convexity at x, minimised over the box voxel by voxel
    z = A @ x
    d = 2 * s * (z - y) if kind == 'square' else s * np.clip(z - y, -par, par) \
        if kind == 'huber' else s * (1 - y / (z + par))
    g = A.T @ d + c * x
    t = np.clip(-g / c, lower - x, upper - x)
    return x, float(cp.phi(kind, s, y, z).sum() + damp * np.mean(x * x) + (g * t + c / 2 * t * t).sum())


def _abs_lp(A, s, y, edges, lower, upper):
    """min sum s |A x - y| + sum c |D x| over the box as a linear programme in (x, u, v) with
    u >= |A x - y| and v >= |D x| -> the optimal value."""
    from scipy.optimize import linprog
    M, V = A.shape
    D, cd = (edges[0], edges[1]) if edges is not None else (np.zeros((0, V)), np.zeros(0))
    E = len(D)
    cost = np.concatenate([np.zeros(V), s, cd])
    Z = np.zeros
    A_ub = np.block([[A, -np.eye(M), Z((M, E))], [-A, -np.eye(M), Z((M, E))],
                     [D, Z((E, M)), -np.eye(E)], [-D, Z((E, M)), -np.eye(E)]])
    b_ub = np.concatenate([y, -y, Z(2 * E)])
    res = linprog(cost, A_ub=A_ub, b_ub=b_ub,
                  bounds=[(lower, upper)] * V + [(0, None)] * (M + E), method='highs')
    assert res.status == 0, res.message
    return float(res.fun)


def test_other_inputs_take_the_generic_path_and_still_solve():
    """A float32 x0 runs in its dtype, a non-contiguous x0 solves, zero iterations return the
    clamped start, and a dynamic operator (view i <-> time slice i, the TV term over each
    slice's r, e, a) closes its own gap."""
    from cpu_operator import CpuOperator
    from sph_raytracer_amd import SphericalGrid
    from sph_raytracer_amd.retrieval import chambolle_pock
    case = ('tiny', 'huber', True, True, cp.DAMP, cp.LOWER, cp.UPPER)
    op, y, mask, A = cp.problem('tiny')
    want = cp.solve_case(case)[0]
    x32, _, i32 = cp.solve_case(case, x0=tr.zeros(4, 3, 6, dtype=tr.float32))
    assert x32.dtype == tr.float32 and i32['dual'].dtype == tr.float32
    # (float32 rounding 6e-8 at a condition number under 1e3)
    assert float((x32.double() - want).abs().max()) <= 1e-4
    xs, _, _ = cp.solve_case(case, x0=tr.zeros(6, 3, 4, dtype=F64).permute(2, 1, 0))
    assert float((xs - want).abs().max()) <= 1e-12
    x0 = tr.linspace(-1, 2, 72, dtype=F64).reshape(4, 3, 6)
    xz, yz, iz = chambolle_pock(op, y, cp.terms('huber', True, mask), x0=x0, num_iterations=0,
                                lower=cp.LOWER, upper=cp.UPPER, norm=5.0)
    assert tr.equal(xz, x0.clamp(cp.LOWER, cp.UPPER)) and iz['norm'] == 5.0
    assert iz['primal_change'] == [] and not iz['ray_dual'].any() and not iz['dual'].any()
    # a dynamic grid: two time slices, one per view
    dgrid = SphericalGrid(shape=(2, 4, 3, 6))
    dop = CpuOperator(dgrid, op.geom)
    g = tr.Generator().manual_seed(3)
    yd = dop(tr.rand(tuple(dgrid.shape), dtype=F64, generator=g)).detach().clamp(min=0.0)
    for kind in ('abs', 'poisson'):
        xt, yh, info = chambolle_pock(dop, yd, cp.terms(kind, True), damp=cp.DAMP, lower=cp.LOWER,
                                      upper=cp.UPPER, num_iterations=cp.ITERATIONS)
        assert xt.shape == tuple(dgrid.shape) and yh.shape == yd.shape
        assert info['dual'].shape == (3,) + tuple(dgrid.shape)
        assert bool(((xt >= cp.LOWER) & (xt <= cp.UPPER)).all())
        # the gap of the stacked problem: A block-diagonal over the slices' views
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
        J = cp.primal_value(kind, Ad, s, yn, edges, cp.DAMP, xn)
        D = cp.dual_value(kind, Ad, s, yn, edges, cp.DAMP, cp.LOWER, cp.UPPER,
                          info['ray_dual'].numpy().reshape(-1), q)
        print(f'dynamic {kind}: J {J:.6g}, D {D:.6g}, gap {(J - D) / abs(J):.3g}')
        assert D <= J + cp.WEAK_DUALITY_SLACK * abs(J) and (J - D) / abs(J) <= cp.GAP_LIMIT[kind]
