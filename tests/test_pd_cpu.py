"""Host side of the primal-dual solver (retrieval.primal_dual; csrc/loss.hip's two pd entries,
declared in include/sphrt_pd.h): the header, the bindings and the library's exports agree, and
none of it leaks into sphrt.h's table; the stream-order rows of pd_stream_cases cover every
stream-taking entry of the header; the entries' refusals fire on the host; pd_cases holds what
it claims, on the references alone (the exact cases are integers, every clamp branch occurs, the
certificate holds, the MEASURED table reproduces); primal_dual refuses bad terms and arguments by
name; and the generic (plain torch) path over the oracle-backed CpuOperator reaches the
certified minimiser of the tiny problem — grid 4 x 3 x 6, two views of 6 x 6 rays — within the
limit.  (No compute call of the library.)"""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import fista_cases as fc
import loop_cases as lc
import pd_cases as pc
import pd_stream_cases as psc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = tr.float64
VP, INT, DBL = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


# ---- the header, the bindings, the library ---------------------------------------------------------------
def _header(name):
    with open(os.path.join(ROOT, 'include', name)) as fh:
        return fh.read()


def _declared(name):
    """As test_cpu_api parses sphrt.h: every sphrt_* name followed by a parenthesis."""
    return sorted(set(re.findall(r'\b(sphrt_[a-z0-9_]+)\s*\(', _header(name))))


def test_header_bindings_and_exports_agree():
    from sph_raytracer_amd import _lib, build
    build.build()
    declared = _declared('sphrt_pd.h')
    assert declared == ['sphrt_pd_dual_f64', 'sphrt_pd_primal_f64']
    assert sorted(_lib.PD_EXPORTED) == declared, 'ctypes bindings out of sync with sphrt_pd.h'
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    old = _declared('sphrt.h')
    for name in declared:
        assert hasattr(raw, name), f'{name} declared in include/sphrt_pd.h but not exported'
        assert name not in old and name not in _lib.EXPORTED and name not in _header('sphrt.h')
        assert getattr(lib, name).restype is ctypes.c_int
    # the argument types, from the declarations
    hdr = re.sub(r'/\*.*?\*/', '', _header('sphrt_pd.h'), flags=re.S)
    for name, _, argtypes in _lib._PD_SIGNATURES:
        m = re.search(r'int\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr)
        args = [' '.join(a.split()) for a in m.group(1).split(',')]
        assert len(args) == len(argtypes) and args[-1] == 'void *stream', name
        for a, ct in zip(args, argtypes):
            want = VP if '*' in a else INT if a.startswith('int ') else DBL
            assert ct is want, (name, a)
        assert list(getattr(lib, name).argtypes) == argtypes


def test_every_stream_entry_of_the_header_has_a_row():
    """pd_stream_cases.ROWS, between them, reach every entry of sphrt_pd.h that takes a stream;
    there is no exempt list."""
    import stream_cases as sc
    entries = sc.stream_entries(os.path.join(ROOT, 'include', 'sphrt_pd.h'))
    assert sorted(entries) == _declared('sphrt_pd.h')
    reached = {e for row in psc.ROWS for e in row.entries}
    assert set(entries) <= reached, sorted(set(entries) - reached)
    assert all(set(entries) <= set(row.entries) for row in psc.ROWS)
    known = set(entries) | set(sc.stream_entries())
    assert all(e in known for row in psc.ROWS for e in row.entries)
    assert len({row.name for row in psc.ROWS}) == len(psc.ROWS)


def test_refusals_on_the_host():
    """Every refusal returns non-zero with its word in sphrt_last_error before any launch: the
    pointers (small fake addresses) are never dereferenced."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    a, b, c, d, e, f = (VP(1 << 24 | 65536 * k) for k in range(1, 7))
    nan, inf = float('nan'), float('inf')

    def primal(x=a, g=b, q=c, xn=d, shape=(5, 7, 9), tau=e, lower=0.0, upper=1.0, mm=f):
        return lib.sphrt_pd_primal_f64(x, g, q, xn, *shape, 1, 1, 1, 1, 0.5, tau, lower, upper,
                                       mm, None)

    def dual(xn=a, xo=b, q=c, shape=(5, 7, 9), cs=(1.0, 0.0, 2.0), sigma=e, qq=f):
        return lib.sphrt_pd_dual_f64(xn, xo, q, *shape, 1, 1, 1, 1, *cs, sigma, qq, None)

    cases = []
    for fn in (primal, dual):
        cases += [(fn, dict(shape=s), b'axis') for s in ((0, 7, 9), (5, -1, 9), (5, 7, 0))]
        cases += [(fn, dict(shape=s), b'2^31') for s in ((2 ** 11, 2 ** 10, 2 ** 10),
                                                        (2 ** 30, 2 ** 30, 2 ** 30),
                                                        (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))]
    cases += [(primal, {k: None}, b'null') for k in ('x', 'g', 'q', 'xn', 'tau', 'mm')]
    cases += [(dual, {k: None}, b'null') for k in ('xn', 'xo', 'q', 'sigma', 'qq')]
    nb = 8 * 315
    cases += [(primal, dict(xn=a), b'alias'), (primal, dict(xn=b), b'alias'),
              (primal, dict(xn=c), b'alias'), (primal, dict(g=a), b'alias'),
              (primal, dict(xn=VP(c.value + 3 * nb - 8)), b'alias'),      # (q's last element)
              (primal, dict(xn=VP(a.value + nb - 8)), b'alias'),
              (primal, dict(mm=VP(d.value + 8)), b'alias'), (primal, dict(tau=VP(c.value + nb)), b'alias'),
              (primal, dict(mm=e), b'alias'),
              (dual, dict(q=a), b'alias'), (dual, dict(q=b), b'alias'), (dual, dict(xo=a), b'alias'),
              (dual, dict(xn=VP(c.value + 2 * nb)), b'alias'), (dual, dict(qq=VP(c.value + 8)), b'alias'),
              (dual, dict(sigma=VP(f.value + 8)), b'alias')]
    cases += [(primal, dict(lower=nan), b'bound'), (primal, dict(upper=nan), b'bound'),
              (primal, dict(lower=1.0), b'bound'), (primal, dict(lower=3.0), b'bound'),
              (primal, dict(lower=inf, upper=inf), b'bound'),
              (primal, dict(lower=-inf, upper=-inf), b'bound'),
              (primal, dict(lower=0.0, upper=-0.0), b'bound')]
    cases += [(dual, dict(cs=cs), b'c_ax') for cs in ((nan, 1.0, 1.0), (1.0, -1.0, 1.0),
                                                     (1.0, 1.0, inf), (-inf, 1.0, 1.0),
                                                     (1.0, -5e-324, 1.0))]
    for i, (fn, kw, word) in enumerate(cases):
        assert fn(**kw) != 0, (i, fn.__name__, kw)
        assert word in lib.sphrt_last_error(), (i, fn.__name__, kw, lib.sphrt_last_error())


# ---- pd_cases on its own references ----------------------------------------------------------------------
def test_edge_rules():
    """neighbours against edges written out by hand."""
    lo, up = pc.neighbours((3, 1, 2), True, (1, 1, 1))
    # voxels (r, a): 0 (0,0), 1 (0,1), 2 (1,0), 3 (1,1), 4 (2,0), 5 (2,1); e has one element
    assert up[0].tolist() == [2, 3, 4, 5, -1, -1] and lo[0].tolist() == [-1, -1, 0, 1, 2, 3]
    assert up[1].tolist() == [-1] * 6 and lo[1].tolist() == [-1] * 6
    assert up[2].tolist() == [1, 0, 3, 2, 5, 4] and lo[2].tolist() == [1, 0, 3, 2, 5, 4]   # two edges
    lo, up = pc.neighbours((3, 1, 2), False, (1, 1, 1))
    assert up[2].tolist() == [1, -1, 3, -1, 5, -1] and lo[2].tolist() == [-1, 0, -1, 2, -1, 4]
    lo, up = pc.neighbours((1, 5, 1), True, (1, 1, 1))             # a ring of one has no edge
    assert (up[2] == -1).all() and (up[0] == -1).all() and up[1].tolist() == [1, 2, 3, 4, -1]
    lo, up = pc.neighbours((1, 1, 1), True, (1, 1, 1))
    assert (up == -1).all() and (lo == -1).all()
    lo, up = pc.neighbours((5, 7, 9), True, (1, 0, 1))
    assert (up[1] == -1).all() and (up[2] >= 0).all() and (up[0] >= 0).sum() == 4 * 63
    assert up[2][8] == 0 and lo[2][0] == 8 and up[2][9 + 8] == 9
    # D from tv_matrix is the same rule: D x = x[up] - x, and D^T q is adjoint_sum
    rng = np.random.default_rng(0)
    for shape, wrap in (((5, 7, 9), True), ((3, 1, 2), True), ((4, 3, 6), False)):
        D, axis, B = pc.tv_matrix(shape, wrap, (1.0, 0.5, 2.0))
        has = [n > 1 for n in shape]
        lo, up = pc.neighbours(shape, wrap, has)
        assert B == 4 * sum(has) and len(D) == int((up >= 0).sum())
        x, q = rng.standard_normal(math.prod(shape)), rng.standard_normal(len(D))
        qv = np.zeros((3, len(x)))
        for ax in range(3):
            qv[ax][up[ax] >= 0] = q[axis == ax]
            assert np.array_equal((D @ x)[axis == ax], (x[up[ax]] - x)[up[ax] >= 0])
        assert np.allclose(D.T @ q, pc.adjoint_sum(qv, lo, up), rtol=0, atol=1e-14)
        assert np.linalg.norm(D, 2) ** 2 <= B * (1 + 1e-12)
    D, _, B = pc.tv_matrix((1, 1, 8), True, (0.0, 0.0, 1.0))           # an even ring attains 4
    assert B == 4 and abs(np.linalg.norm(D, 2) ** 2 - 4) < 1e-12


def test_the_reference_total_variation_is_the_loss_class_s():
    """sum c |D x| of the dense reference — D from pd_cases' edge rules, c = lam w / V — is what
    lam * SmoothRegularizer(kind='abs') itself evaluates to (its torch formula, and the call
    gd makes), for the ring closed, open, and inferred from a grid that spans 2 pi or does not."""
    from sph_raytracer_amd import SphericalGrid
    from sph_raytracer_amd.loss import SmoothRegularizer
    rng = np.random.default_rng(4)
    for shape in ((4, 3, 6), (5, 6, 10), (3, 1, 2), (1, 5, 1)):
        x = rng.standard_normal(shape)
        xt = tr.from_numpy(x)
        for wrap in (False, True):
            for weights in (pc.TV_WEIGHTS, (0.0, 1.5, 1.0)):
                D, axis, _ = pc.tv_matrix(shape, wrap, weights)
                c = pc.LAM_TV * np.asarray(weights)[axis] / x.size
                want = float((c * np.abs(D @ x.reshape(-1))).sum()) if len(D) else 0.0
                reg = pc.LAM_TV * SmoothRegularizer(weights=weights, kind='abs', wrap_a=wrap)
                assert reg.wraps(None) is wrap
                got = pc.LAM_TV * float(reg.formula(xt, wrap))
                assert abs(got - want) <= 1e-14 * max(abs(want), 1e-300), (shape, wrap, weights)
                assert abs(float(reg(None, None, xt, xt)) - want) <= 1e-14 * max(abs(want), 1e-300)
    # wrap_a=None: the ring closes exactly when the grid spans 2 pi in azimuth
    grid = SphericalGrid(shape=(4, 3, 6))
    reg = pc.LAM_TV * SmoothRegularizer(weights=pc.TV_WEIGHTS, kind='abs')
    f = _Shape((4, 3, 6))
    f.a_b = grid.a_b
    span = abs(float(grid.a_b[-1]) - float(grid.a_b[0]))
    assert reg.wraps(f) is (abs(span - 2 * math.pi) <= 1e-9 * 2 * math.pi) and reg.wraps(None) is False
    x = rng.standard_normal((4, 3, 6))
    D, axis, _ = pc.tv_matrix((4, 3, 6), reg.wraps(f), pc.TV_WEIGHTS)
    c = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS)[axis] / 72
    want = float((c * np.abs(D @ x.reshape(-1))).sum())
    assert abs(float(reg(f, None, tr.from_numpy(x), None)) - want) <= 1e-14 * want


def test_exact_cases_are_exact():
    """The integer references equal the float64 expressions (every operation is exact on this
    value set, fused or not); each clamp branch of either kernel takes a share of every case
    with at least 63 voxels; the partial sums are integers in their unit."""
    for shape, wrap, has in pc.kernel_cases():
        n = math.prod(shape)
        lo, up = pc.neighbours(shape, wrap, has)
        x, g, q, xn, xo = pc.exact_vectors(shape, seed=7 * n)
        s = pc.adjoint_sum(q, lo, up)
        for case in pc.EXACT_PRIMAL:
            c, tau, lower, upper = (a / b for a, b in case)
            want, mm, branch = pc.exact_primal(x, g, q, lo, up, *case)
            u = x - tau * ((c * x + g) + s)
            assert np.array_equal(want, np.where(u < lower, lower, np.where(u > upper, upper, u)))
            assert np.array_equal(mm, cc.block_partials((want - x) ** 2))
            assert len(mm) == lc.grid_of(n)
            unit = 8 * case[0][1] * case[1][1]
            assert np.array_equal(mm * unit ** 2, np.round(mm * unit ** 2))
            if n >= 63:
                for br in (-1, 0, 1):
                    assert (branch == br).sum() >= n / 20, (shape, case, br)
        for case in pc.EXACT_DUAL:
            sigma = case[0][0] / case[0][1]
            cax = [a / b for a, b in case[1:]]
            want, qq, branch = pc.exact_dual(xn, xo, q, up, case[0], case[1:])
            xb = 2 * xn - xo
            for ax in range(3):
                m = up[ax] >= 0
                v = q[ax][m] + sigma * (xb[up[ax][m]] - xb[m])
                assert np.array_equal(want[ax][m], np.clip(v, -cax[ax], cax[ax]))
                assert np.array_equal(want[ax][~m], q[ax][~m]) and (branch[ax][~m] == 2).all()
                if n >= 63 and m.any() and cax[ax] > 0:
                    for br in (-1, 0, 1):
                        assert (branch[ax][m] == br).sum() >= m.sum() / 20, (shape, case, ax, br)
            assert np.array_equal(qq, cc.block_partials(pc.dual_terms(want, q, up)))
            assert np.array_equal(qq * (8 * case[0][1]) ** 2, np.round(qq * (8 * case[0][1]) ** 2))
        # a sample through the rational sequences too
        case, dcase = pc.EXACT_PRIMAL[2], pc.EXACT_DUAL[1]
        want, _, _ = pc.exact_primal(x, g, q, lo, up, *case)
        dwant, _, _ = pc.exact_dual(xn, xo, q, up, dcase[0], dcase[1:])
        for i in cc.sample(n, 0, cap=16):
            assert pc.primal_ref(i, x, g, q, lo, up, *(a / b for a, b in case))[0] == want[i]
            got, _ = pc.dual_ref(i, xn, xo, q, up, dcase[0][0] / dcase[0][1],
                                 [a / b for a, b in dcase[1:]])
            assert all(v is None and up[ax, i] < 0 or v == dwant[ax][i] for ax, v in enumerate(got))
    assert {math.prod(s) for s, _, _ in pc.kernel_cases()} >= {1, 5, 6, 512, 315, 274365}
    assert lc.grid_of(315) == 2 and 274365 > lc.STRIDE


def test_random_cases_tell_fma_from_multiply_add():
    shape = (5, 7, 9)
    n = 315
    lo, up = pc.neighbours(shape, True, (1, 1, 1))
    x, g, q, xn, xo = pc.random_vectors(shape, seed=n)
    tau, lower, upper, sigma, cax = pc.random_scalars(n)
    differs, inside, dual_inside, dual_all = 0, 0, 0, 0
    for i in range(n):
        fused = pc.primal_ref(i, x, g, q, lo, up, 0.3, tau, lower, upper)[0]
        plain = pc.primal_unfused(i, x, g, q, lo, up, 0.3, tau, lower, upper)
        differs += fused != plain
        inside += lower < fused < upper
        assert abs(fused - plain) <= 1e-14
        got, _ = pc.dual_ref(i, xn, xo, q, up, sigma, cax)
        dual_all += sum(v is not None for v in got)
        dual_inside += sum(v is not None and abs(v) < c for v, c in zip(got, cax))
    assert differs > 30 and n / 10 < inside < 9 * n / 10
    assert dual_all / 10 < dual_inside < 9 * dual_all / 10


def test_special_cases_hold_what_they_claim():
    (x, g, q, xn, xo), where = pc.special_vectors(seed=9)
    lo, up = pc.neighbours(pc.SPECIAL_SHAPE, True, (1, 1, 1))
    for v in (x, g, q[0], q[1], q[2], xn, xo):
        assert np.isnan(v).any() and np.isinf(v).any() and (np.abs(v[v != 0]) < 1e-300).any()
        assert any(e == 0 and math.copysign(1, e) < 0 for e in v)
    assert len(where) > 60 and where.min() < 256 <= where.max()
    assert any(math.isinf(a) and math.isinf(b) for a, b in pc.SPECIAL_BOUNDS)
    out = [pc.primal_ref(i, x, g, q, lo, up, 0.375, 0.3, 0.0, math.inf)[0] for i in range(315)]
    assert any(math.isnan(v) for v in out) and math.inf in out and 0.0 in out
    assert all(c >= 0 and math.isfinite(c) for cs in pc.SPECIAL_C for c in cs)
    dual = [pc.dual_ref(i, xn, xo, q, up, 0.3, pc.SPECIAL_C[0])[0] for i in range(315)]
    assert any(math.isnan(v) for d in dual for v in d if v is not None)
    assert all(v is None or math.isnan(v) or abs(v) <= c
               for d in dual for v, c in zip(d, pc.SPECIAL_C[0]))
    # (fma(2, x, -x_old) does not overflow where 2 x alone would)
    assert pc.dual_ref(0, [1e308, 1e308], [1e308, 1e308], np.zeros((3, 2)),
                       np.array([[-1, -1], [-1, -1], [1, -1]]), 0.0, (1.0, 1.0, 1.0))[0][2] == 0.0


def test_pd_dense_and_the_certificate_on_a_known_problem():
    """One dimension, N = I: the minimiser of 1/2 |x - b|^2 + c |x_1 - x_0| is known in closed
    form (the two values move towards each other by c each, or meet at their mean); pd_dense
    reaches it, the certificate's radius covers the distance, and a q that is not optimal gives a
    larger gap, never a negative one."""
    N, D, B = np.eye(2), np.array([[-1.0, 1.0]]), 4.0
    for b, c, want, flat in ((np.array([0.0, 1.0]), 0.25, [0.25, 0.75], 0.0),
                             (np.array([0.0, 1.0]), 0.75, [0.5, 0.5], 1.0)):
        cv = np.array([c])
        x, q, radius = pc.certify(N, b, D, cv, -math.inf, math.inf, 1.0, B)
        assert np.allclose(x, want, rtol=0, atol=1e-12) and radius <= 1e-7
        assert np.linalg.norm(x - want) <= radius + 1e-15
        assert pc.edge_shares(q, cv)[0] == flat
        xs, qk, mm, qq = pc.pd_dense(N, b, D, cv, -math.inf, math.inf, 1.0, 1.0, 50, B)
        assert len(xs) == 51 and len(mm) == len(qq) == 50 and abs(qk[0]) <= c
        off = pc.dual_lower_bound(N, b - D.T @ (0.5 * q), b - D.T @ (0.5 * q), -math.inf, math.inf, 1.0)
        assert pc.primal_value(N, b, D, cv, x) - off > 1e-3
    # with bounds: the box cuts the upper value
    x, q, radius = pc.certify(N, np.array([0.0, 1.0]), D, np.array([0.25]), 0.1, 0.6, 1.0, B)
    assert np.allclose(x, [0.25, 0.6], atol=1e-12) and radius <= 1e-7
    assert pc.pd_steps(2.0, 3.0, 8.0) == (1 / 8, 0.75)


# ---- primal_dual's refusals ------------------------------------------------------------------------------
class _Shape:
    def __init__(self, shape):
        self.grid = self
        self.shape = shape
        self.a_b = None


def test_primal_dual_refuses_bad_terms_and_arguments():
    import sph_raytracer_amd as pkg
    from sph_raytracer_amd.loss import (AbsLoss, HuberLoss, NegRegularizer, PoissonLoss,
                                        SmoothRegularizer, SquareLoss)
    from sph_raytracer_amd.retrieval import primal_dual
    assert 'primal_dual' in pkg.__all__ and pkg.primal_dual is primal_dual
    y = tr.zeros(2, 6, 6, dtype=F64)
    f = _Shape((4, 3, 6))
    ok, tv = SquareLoss, lambda **kw: 0.1 * SmoothRegularizer(kind='abs', **kw)
    bad = [([tv()], 'primal_dual needs one SquareLoss'), ([ok(), ok(), tv()], 'two'),
           ([ok()], r"needs one SmoothRegularizer\(kind='abs'\).*fista"),
           ([ok(), SmoothRegularizer()], r"needs one SmoothRegularizer\(kind='abs'\).*fista"),
           ([ok(), tv(), tv()], "kind='abs'.*not 2"),
           ([ok(), tv(), NegRegularizer()], 'NegRegularizer'), ([AbsLoss(), tv()], 'AbsLoss'),
           ([HuberLoss(delta=0.5), tv()], 'HuberLoss'), ([PoissonLoss(), tv()], 'PoissonLoss'),
           ([ok(), tv(), SmoothRegularizer(kind='huber', delta=1.0)], "'huber'"),
           ([ok(), tv(), SmoothRegularizer(), SmoothRegularizer()], 'at most one SmoothRegularizer'),
           ([ok(), 0.0 * SmoothRegularizer(kind='abs')], 'lam > 0'),
           ([ok(), -1.0 * SmoothRegularizer(kind='abs')], 'lam > 0'),
           ([ok(), tr.tensor(2.0) * SmoothRegularizer(kind='abs')], 'lam > 0'),
           ([ok(), float('inf') * SmoothRegularizer(kind='abs')], 'lam > 0'),
           ([ok(), tv(use_grad=False)], 'use_grad'), ([ok(), tv(volume_mask=2)], 'volume_mask'),
           ([ok(), tv(projection_mask=2)], 'projection_mask'),
           ([tr.tensor(2.0) * ok(), tv()], 'lam'), ([ok(use_grad=False), tv()], 'use_grad'),
           ([ok(volume_mask=2), tv()], 'volume_mask'), ([ok(projection_mask=2), tv()], 'projection_mask'),
           ([ok(), tv(weights=(0, 0, 0))], 'no edges')]
    for fns, word in bad:
        with pytest.raises(ValueError, match=word):
            primal_dual(f, y, fns)                 # (refused before the operator is used)
    # an axis with a weight but one element has no edge either; a time weight needs a 3-D volume
    with pytest.raises(ValueError, match='no edges'):
        primal_dual(_Shape((4, 1, 6)), y, [ok(), tv(weights=(0, 1, 0))])
    with pytest.raises(ValueError, match='time_weight'):
        primal_dual(_Shape((2, 4, 3, 6)), y, [ok(), tv(time_weight=1.0)])
    with pytest.raises(ValueError, match='r, e, a'):
        primal_dual(f, y, [ok(), tv()], x0=tr.zeros(3, 6, dtype=F64))
    nan, inf = float('nan'), float('inf')
    for kw, word in ((dict(damp=-1.0), 'damp'), (dict(damp=nan), 'damp'),
                     (dict(num_iterations=-1), 'num_iterations'),
                     (dict(num_iterations=2.5), 'num_iterations'),
                     (dict(lower=nan), 'lower'), (dict(upper=nan), 'upper'),
                     (dict(lower='0'), 'lower'), (dict(upper=tr.tensor(1.0)), 'upper'),
                     (dict(lower=True), 'lower'),
                     (dict(lower=1.0, upper=1.0), 'lower < upper'),
                     (dict(lower=2.0, upper=1.0), 'lower < upper'),
                     (dict(lower=None, upper=-inf), 'lower < upper'),
                     (dict(lower=inf, upper=None), 'lower < upper'),
                     (dict(lipschitz=0.0), 'lipschitz'), (dict(lipschitz=-1.0), 'lipschitz'),
                     (dict(lipschitz=inf), 'lipschitz'), (dict(lipschitz=nan), 'lipschitz'),
                     (dict(lipschitz=tr.tensor(1.0)), 'lipschitz'),
                     (dict(power_iterations=0), 'power_iterations'),
                     (dict(power_iterations=1.5), 'power_iterations'),
                     (dict(dual_ratio=0.0), 'dual_ratio'), (dict(dual_ratio=-1.0), 'dual_ratio'),
                     (dict(dual_ratio=inf), 'dual_ratio'), (dict(dual_ratio=nan), 'dual_ratio'),
                     (dict(dual_ratio=True), 'dual_ratio'), (dict(dual_ratio='1'), 'dual_ratio'),
                     (dict(dual_ratio=tr.tensor(1.0)), 'dual_ratio')):
        with pytest.raises(ValueError, match='primal_dual needs.*' + word):
            primal_dual(f, y, [ok(), tv()], **kw)
    with pytest.raises(ValueError, match='primal_dual needs measurements'):
        primal_dual(f, None, [ok(), tv()])


def test_cg_and_fista_still_refuse_the_tv_term_in_their_own_words():
    from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
    from sph_raytracer_amd.retrieval import cg, fista
    y = tr.zeros(2, 6, 6, dtype=F64)
    for solver, who in ((cg, 'cg'), (fista, 'fista')):
        with pytest.raises(ValueError, match=who + r" needs a quadratic total: SmoothRegularizer\(kind='abs'\)"):
            solver(None, y, loss_fns=[SquareLoss(), SmoothRegularizer(kind='abs')])
    with pytest.raises(ValueError, match='fista needs lower < upper, not lower = 2.0, upper = 1.0'):
        fista(None, y, lower=2.0, upper=1.0)


# ---- the generic path against the certified minimiser --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operator(name='tiny'):
    from cpu_operator import CpuOperator
    from sph_raytracer_amd import ConeRectGeom, SphericalGrid
    if name == 'tiny':
        grid = SphericalGrid(shape=(4, 3, 6))
        geom = ConeRectGeom((6, 6), pos=(5, 0.3, 1), fov=(25, 25)) + \
            ConeRectGeom((6, 6), pos=(-1, 4.5, -2), fov=(25, 25))
    else:                                   # the 257-ray problem of test_gpu_cg.py
        grid = SphericalGrid(shape=(5, 6, 10))
        geom = ConeRectGeom((257, 1), pos=(4, 1, 0.5), fov=(50, 1))
    op = CpuOperator(grid, geom)
    g = tr.Generator().manual_seed(11)
    truth = tr.rand(tuple(grid.shape), dtype=F64, generator=g)      # uniform in [0, 1]
    y = op(truth).detach()
    y = y + 0.01 * tr.randn(y.shape, dtype=F64, generator=g)
    mask = tr.rand(y.shape, dtype=F64, generator=g) + 0.25
    mask.view(-1)[3] = 0.0                   # (a masked pixel)
    return op, y, mask


def quadratic_terms(mask, masked, wrap):
    from sph_raytracer_amd.loss import SmoothRegularizer, SquareLoss
    fns = [1.5 * SquareLoss(projection_mask=mask if masked else 1)]
    if wrap is not None:
        fns.append(0.3 * SmoothRegularizer(weights=(1, 0.5, 2), wrap_a=wrap))
    return fns


def tv_term(masked):
    from sph_raytracer_amd.loss import SmoothRegularizer
    return pc.LAM_TV * SmoothRegularizer(weights=pc.TV_WEIGHTS, kind='abs',
                                         wrap_a=pc.tv_wrap(masked))


BOUNDS = [(pc.LOWER, pc.UPPER), (None, None)]


def _inf(lower, upper):
    return (-math.inf if lower is None else lower, math.inf if upper is None else upper)


def power_lipschitz(N):
    """L as `primal_dual` estimates it: `fista`'s power method and margin."""
    from sph_raytracer_amd import retrieval
    v = np.ones(len(N))
    for _ in range(retrieval._FISTA_POWER_ITERATIONS):
        w = N @ v
        rho = (v @ w) / (v @ v)
        v = w / np.linalg.norm(w)
    return rho * (1 + retrieval._FISTA_MARGIN)


def dense_problem(op, y, mask, masked, wrap):
    """(the quadratic terms, damp, N, b, D, c, B, L) of a variant over the operator `op`: N and b
    from the loss classes by autograd (the TV term is not among them), D and c from pd_cases."""
    fns, shape = quadratic_terms(mask, masked, wrap), tuple(op.grid.shape)
    N0, _, _ = cc.dense_system(op, y, fns, 0.0, shape)
    damp = cc.damp_for(N0, math.prod(shape))
    N, b, asym = cc.dense_system(op, y, fns, damp, shape)
    assert asym <= 1e-12 * np.abs(N).max()
    assert cc.condition(N) <= cc.KAPPA_MAX
    D, axis, B = pc.tv_matrix(shape, pc.tv_wrap(masked), pc.TV_WEIGHTS)
    c = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS)[axis] / math.prod(shape)
    return fns, damp, N, b, D, c, B, power_lipschitz(N)


@functools.lru_cache(maxsize=None)
def _system(name, masked, wrap):
    op, y, mask = _operator(name)
    return dense_problem(op, y, mask, masked, wrap)


@functools.lru_cache(maxsize=None)
def _certified(name, masked, wrap, lower, upper):
    _, _, N, b, D, c, B, L = _system(name, masked, wrap)
    return pc.certify(N, b, D, c, *_inf(lower, upper), L, B)


def measure(name, masked, wrap, lower, upper, horizon=None):
    """-> (K, the error at pd_cases.ITERATIONS or None, the relative radius, the edge shares) of a
    case: what pd_cases.MEASURED records and tools/pd_study.py prints."""
    _, _, N, b, D, c, B, L = _system(name, masked, wrap)
    want, q, radius = _certified(name, masked, wrap, lower, upper)
    horizon = horizon or min(pc.ITERATIONS + 2000, pc.K_CAP + 2000)
    xs, _, _, _ = pc.pd_dense(N, b, D, c, *_inf(lower, upper), L, pc.DUAL_RATIO, horizon, B)
    errs = [cc.rel_err(x, want) for x in xs]
    k = pc.first_stays_under(errs, pc.STAYS_UNDER)
    at = errs[pc.ITERATIONS] if pc.ITERATIONS < len(errs) else None
    return k, at, radius / np.linalg.norm(want), pc.edge_shares(q, c)


@pytest.mark.parametrize('name', ['tiny', 'two_workgroups'])
def test_certificate_and_recorded_iterations(name):
    """On every case the certificate holds with a radius of at most RADIUS_MAX |x*|, the TV term
    is exercised (some edges flat, some carrying a jump), and pd_cases.ITERATIONS and LIMIT are
    what pd_dense measures: every case stays under STAYS_UNDER from ITERATIONS on at the latest,
    and LIMIT is 100 times the largest error there (RADIUS_MAX at least)."""
    assert pc.RADIUS_MAX <= pc.STAYS_UNDER and pc.ITERATIONS <= pc.K_CAP
    for masked, wrap in pc.VARIANTS:
        for lower, upper in BOUNDS:
            key = (name, masked, wrap, lower is not None)
            k, at, radius, (flat, jump) = measure(name, masked, wrap, lower, upper)
            print(key, k, at, radius, flat, jump)
            assert radius <= pc.RADIUS_MAX, key
            assert flat > 0 and jump > 0, key
            assert k is not None and k <= pc.ITERATIONS, key
            assert 100 * at <= pc.LIMIT and pc.LIMIT >= pc.RADIUS_MAX, key
            # as recorded: K to one iteration, the error and the radius to a couple of digits
            # (an error under 1e-9 is a hundredth of the smallest radius: below what the
            # certificate resolves, and compared absolutely)
            rec_k, rec_at, rec_radius = pc.MEASURED[key]
            assert abs(rec_k - k) <= 1, (key, k)
            assert math.isclose(at, rec_at, rel_tol=0.05, abs_tol=1e-9), (key, at)
            assert math.isclose(radius, rec_radius, rel_tol=0.05), (key, radius)
            if lower is not None and wrap is None:
                # (both bounds bind; the square smooth term pulls the solution towards its mean,
                # and with it one of them may hold no voxel: test_fista_cpu.py's docstring)
                want = _certified(name, masked, wrap, lower, upper)[0]
                assert (want == lower).any() and (want == upper).any(), key
    assert max(v[0] for v in pc.MEASURED.values()) == pc.ITERATIONS
    # LIMIT is 100 times the largest recorded error, rounded up in its second digit: no looser
    worst = 100 * max(v[1] for v in pc.MEASURED.values())
    assert worst <= pc.LIMIT <= 1.01 * max(worst, pc.RADIUS_MAX)


@pytest.mark.parametrize('lower,upper', BOUNDS)
@pytest.mark.parametrize('masked,wrap', pc.VARIANTS)
def test_generic_path_reaches_the_certified_minimiser(masked, wrap, lower, upper):
    from sph_raytracer_amd.retrieval import primal_dual
    op, y, mask = _operator()
    fns, damp, N, b, D, c, B, L = _system('tiny', masked, wrap)
    want, q_want, _ = _certified('tiny', masked, wrap, lower, upper)
    fns = fns + [tv_term(masked)]
    x, y_hat, info = primal_dual(op, y, fns, damp=damp, lower=lower, upper=upper,
                                 num_iterations=pc.ITERATIONS)
    assert x.shape == tuple(op.grid.shape) and x.dtype == F64 and not x.requires_grad
    assert tr.equal(y_hat, op(x)) and y_hat.shape == y.shape
    err = cc.rel_err(x.numpy(), want)
    print(f'primal_dual tiny masked={masked} wrap={wrap} bounds={lower, upper}: {err:.3g}')
    assert err <= pc.LIMIT
    lo, hi = _inf(lower, upper)
    xn = x.numpy().reshape(-1)
    assert np.all((xn >= lo) & (xn <= hi))
    q = info['dual']
    assert q.shape == (3, 4, 3, 6) and q.dtype == F64
    cax = pc.LAM_TV * np.asarray(pc.TV_WEIGHTS) / 72
    assert all(float(q[ax].abs().max()) <= cax[ax] for ax in range(3))
    _, up = pc.neighbours((4, 3, 6), pc.tv_wrap(masked), (1, 1, 1))
    qn = q.numpy().reshape(3, -1)
    assert not qn[up < 0].any() and not np.signbit(qn[up < 0]).any()     # +0.0 where no edge
    assert abs(info['lipschitz'] - L) <= 1e-12 * L
    tau, sigma = pc.pd_steps(info['lipschitz'], 1.0, B)
    assert info['tau'] == tau and info['sigma'] == sigma
    pcg, dcg = info['primal_change'], info['dual_change']
    assert len(pcg) == len(dcg) == pc.ITERATIONS and pcg[0] == 1.0
    assert all(math.isfinite(v) and v >= 0 for v in pcg + dcg) and pcg[-1] < 1e-6
    # a given L and ratio are used as they are, and the iterates are the dense restatement's
    L2 = 1.25 * float(np.linalg.eigvalsh(N)[-1])
    x12, _, i12 = primal_dual(op, y, fns, damp=damp, lower=lower, upper=upper, num_iterations=12,
                              lipschitz=L2, dual_ratio=0.5)
    xs, qk, mm, qq = pc.pd_dense(N, b, D, c, lo, hi, L2, 0.5, 12, B)
    assert i12['lipschitz'] == L2 and (i12['tau'], i12['sigma']) == pc.pd_steps(L2, 0.5, B)
    assert cc.rel_err(x12.numpy(), xs[-1]) <= 1e-12
    q12 = i12['dual'].numpy().reshape(3, -1)
    assert np.allclose(np.concatenate([q12[ax][up[ax] >= 0] for ax in range(3)]), qk,
                       rtol=0, atol=1e-12 * c.max())
    assert np.allclose(i12['primal_change'], np.sqrt(np.array(mm) / mm[0]), rtol=1e-9)
    assert np.allclose(i12['dual_change'], np.sqrt(qq), rtol=1e-9, atol=1e-18)


def test_iterates_bounds_zero_measurements_and_other_starts():
    from sph_raytracer_amd.retrieval import primal_dual
    op, y, mask = _operator()
    fns, damp, N, b, D, c, B, L = _system('tiny', True, False)
    fns = fns + [tv_term(True)]
    lo_bits, hi_bits = (np.float64(v).view(np.int64) for v in (pc.LOWER, pc.UPPER))
    x0 = tr.linspace(-1, 2, 72, dtype=F64).reshape(4, 3, 6)
    hit = [0, 0]
    for k in range(0, 6):
        x, _, info = primal_dual(op, y, fns, damp=damp, lower=pc.LOWER, upper=pc.UPPER,
                                 num_iterations=k, x0=x0)
        xn = x.numpy().reshape(-1)
        assert np.all((xn >= pc.LOWER) & (xn <= pc.UPPER)), k
        bits = xn.view(np.int64)
        assert np.all(bits[xn == pc.LOWER] == lo_bits) and np.all(bits[xn == pc.UPPER] == hi_bits)
        hit[0] += int((xn == pc.LOWER).sum())
        hit[1] += int((xn == pc.UPPER).sum())
        assert len(info['primal_change']) == len(info['dual_change']) == k
    assert min(hit) > 0 and tr.equal(x0, tr.linspace(-1, 2, 72, dtype=F64).reshape(4, 3, 6))
    # the default is x >= 0
    x, _, _ = primal_dual(op, y - 1.0, fns, damp=damp, num_iterations=30)
    assert float(x.min()) == 0.0 and bool((x == 0).any())
    # b = 0 with 0 inside the bounds: nothing moves, both histories are zeros
    x, y_hat, info = primal_dual(op, tr.zeros_like(y), fns, damp=damp, lower=-1.0, upper=1.0,
                                 num_iterations=5)
    assert not x.any() and not y_hat.any() and not info['dual'].any()
    assert info['primal_change'] == [0.0] * 5 and info['dual_change'] == [0.0] * 5
    # a float32 start runs in its dtype; a non-contiguous start solves
    want = _certified('tiny', True, False, pc.LOWER, pc.UPPER)[0]
    x32, _, i32 = primal_dual(op, y, fns, damp=damp, lower=pc.LOWER, upper=pc.UPPER,
                              num_iterations=2000, x0=tr.zeros(4, 3, 6, dtype=tr.float32))
    # (float32 rounding 6e-8 at a condition number of at most 100: 6e-6, with a decade to spare)
    assert x32.dtype == tr.float32 and i32['dual'].dtype == tr.float32
    assert cc.rel_err(x32.double().numpy(), want) <= 1e-4
    xs, _, _ = primal_dual(op, y, fns, damp=damp, lower=pc.LOWER, upper=pc.UPPER,
                           num_iterations=pc.ITERATIONS, x0=tr.zeros(6, 3, 4, dtype=F64).permute(2, 1, 0))
    assert cc.rel_err(xs.numpy(), want) <= pc.LIMIT
