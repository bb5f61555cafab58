"""Host side of isotropic total variation (loss.IsoTVRegularizer; csrc/loss.hip's two entries
declared in include/sphrt_iso.h; the iso branch of retrieval.primal_dual and
retrieval.chambolle_pock): the header, the bindings and the library's exports agree and none of it
leaks into the other headers or their tables; the stream-order rows of iso_stream_cases reach
every entry; the entries' refusals fire on the host; the class against a loop-written restatement;
iso_cases holds what it claims on its own references (the exact cases in Fractions, the
certificate on a known problem, the MEASURED tables reproduce); both solvers refuse bad terms by
name, follow iso_dense's iterates over the oracle-backed CpuOperator, and chambolle_pock closes
its duality gap with every fidelity kind; gd declines the class from its direct loops.  (No
compute call of the library.)"""
import ctypes
import math
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import cp_cases as cp
import iso_cases as ic
import pd_cases as pc
import test_pd_cpu as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = tr.float64
VP, INT, DBL = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
OTHER_HEADERS = ('sphrt.h', 'sphrt_pd.h', 'sphrt_cp.h', 'sphrt_dp.h')
NAMES = ['sphrt_iso_dual_f64', 'sphrt_iso_primal_f64']


def _header(name):
    with open(os.path.join(ROOT, 'include', name)) as fh:
        return fh.read()


def _declared(name):
    hdr = re.sub(r'/\*.*?\*/', '', _header(name), flags=re.S)
    return sorted(set(re.findall(r'\b(sphrt_[a-z0-9_]+)\s*\(', hdr)))


# ---- the header, the bindings, the library ---------------------------------------------------------------
def test_header_bindings_and_exports_agree():
    from sph_raytracer_amd import _lib, build
    build.build()
    declared = _declared('sphrt_iso.h')
    assert declared == NAMES
    assert sorted(_lib.ISO_EXPORTED) == declared, 'ctypes bindings out of sync with sphrt_iso.h'
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name in declared:
        assert hasattr(raw, name), f'{name} declared in include/sphrt_iso.h but not exported'
        for other in OTHER_HEADERS:
            assert name not in _header(other)
        assert name not in _lib.EXPORTED + _lib.PD_EXPORTED + _lib.CP_EXPORTED + _lib.DP_EXPORTED
        assert getattr(lib, name).restype is ctypes.c_int
    assert 'sphrt_iso' not in ''.join(_header(h) for h in OTHER_HEADERS)
    hdr = re.sub(r'/\*.*?\*/', '', _header('sphrt_iso.h'), flags=re.S)
    for name, _, argtypes in _lib._ISO_SIGNATURES:
        m = re.search(r'int\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr)
        args = [' '.join(a.split()) for a in m.group(1).split(',')]
        assert len(args) == len(argtypes) and args[-1] == 'void *stream', name
        for a, ct in zip(args, argtypes):
            want = VP if '*' in a else INT if a.startswith('int ') else DBL
            assert ct is want, (name, a)
        assert list(getattr(lib, name).argtypes) == argtypes
    assert 'sphrt_iso.h' in open(build.__file__).read()


def test_every_stream_entry_of_the_header_has_a_row():
    import iso_stream_cases as isc
    import stream_cases as sc
    entries = sc.stream_entries(os.path.join(ROOT, 'include', 'sphrt_iso.h'))
    assert sorted(entries) == _declared('sphrt_iso.h') == sorted(isc.ISO_ENTRIES)
    assert all(set(entries) <= set(row.entries) for row in isc.ROWS) and isc.ROWS
    known = set(entries) | set(sc.stream_entries())
    for other in OTHER_HEADERS[1:]:
        known |= set(sc.stream_entries(os.path.join(ROOT, 'include', other)))
    assert all(e in known for row in isc.ROWS for e in row.entries)
    assert not any(e.startswith('sphrt_pd_') for row in isc.ROWS for e in row.entries)
    assert len({row.name for row in isc.ROWS}) == len(isc.ROWS)
    for solver in ('primal_dual', 'chambolle_pock'):
        kinds = [row.params['kind'] for row in isc.ROWS if row.params['solver'] == solver]
        assert sorted(kinds) == sorted(sc.OPERATORS)          # one row per operator kind
    assert set(isc.RECIPES) == {row.recipe for row in isc.ROWS}


def test_refusals_on_the_host():
    """Every refusal returns non-zero with its word in sphrt_last_error before any launch: the
    pointers (small fake addresses) are never dereferenced."""
    from sph_raytracer_amd import _lib
    lib = _lib.load()
    a, b, c, d, e, f = (VP(1 << 24 | 65536 * k) for k in range(1, 7))
    nan, inf = float('nan'), float('inf')

    def primal(x=a, g=b, q=c, xn=d, shape=(5, 7, 9), ws=(1.0, 0.5, 2.0), tau=e, lower=0.0,
               upper=1.0, mm=f):
        return lib.sphrt_iso_primal_f64(x, g, q, xn, *shape, 1, *ws, 0.5, tau, lower, upper, mm,
                                        None)

    def dual(xn=a, xo=b, q=c, shape=(5, 7, 9), ws=(1.0, 0.0, 2.0), radius=1.0, sigma=e, qq=f):
        return lib.sphrt_iso_dual_f64(xn, xo, q, *shape, 1, *ws, radius, sigma, qq, None)

    cases = []
    for fn in (primal, dual):
        cases += [(fn, dict(shape=s), b'axis') for s in ((0, 7, 9), (5, -1, 9), (5, 7, 0))]
        cases += [(fn, dict(shape=s), b'2^31') for s in ((2 ** 11, 2 ** 10, 2 ** 10),
                                                        (2 ** 30, 2 ** 30, 2 ** 30),
                                                        (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))]
        cases += [(fn, dict(ws=ws), b'weights') for ws in ((nan, 1.0, 1.0), (1.0, -1.0, 1.0),
                                                          (1.0, 1.0, inf), (-inf, 1.0, 1.0),
                                                          (1.0, -5e-324, 1.0))]
    cases += [(primal, {k: None}, b'null') for k in ('x', 'g', 'q', 'xn', 'tau', 'mm')]
    cases += [(dual, {k: None}, b'null') for k in ('xn', 'xo', 'q', 'sigma', 'qq')]
    nb = 8 * 315
    cases += [(primal, dict(xn=a), b'alias'), (primal, dict(xn=b), b'alias'),
              (primal, dict(xn=c), b'alias'), (primal, dict(g=a), b'alias'),
              (primal, dict(xn=VP(c.value + 3 * nb - 8)), b'alias'),      # (q's last element)
              (primal, dict(xn=VP(a.value + nb - 8)), b'alias'),
              (primal, dict(mm=VP(d.value + 8)), b'alias'),
              (primal, dict(tau=VP(c.value + nb)), b'alias'), (primal, dict(mm=e), b'alias'),
              (dual, dict(q=a), b'alias'), (dual, dict(q=b), b'alias'), (dual, dict(xo=a), b'alias'),
              (dual, dict(xn=VP(c.value + 2 * nb)), b'alias'),
              (dual, dict(qq=VP(c.value + 8)), b'alias'), (dual, dict(sigma=VP(f.value + 8)), b'alias')]
    cases += [(primal, dict(lower=nan), b'bound'), (primal, dict(upper=nan), b'bound'),
              (primal, dict(lower=1.0), b'bound'), (primal, dict(lower=3.0), b'bound'),
              (primal, dict(lower=inf, upper=inf), b'bound'),
              (primal, dict(lower=-inf, upper=-inf), b'bound'),
              (primal, dict(lower=0.0, upper=-0.0), b'bound')]
    cases += [(dual, dict(radius=v), b'radius') for v in (nan, -1.0, inf, -inf, -5e-324)]
    for i, (fn, kw, word) in enumerate(cases):
        assert fn(**kw) != 0, (i, fn.__name__, kw)
        assert word in lib.sphrt_last_error(), (i, fn.__name__, kw, lib.sphrt_last_error())


# ---- the class -------------------------------------------------------------------------------------------
SHAPES = [(4, 3, 6), (3, 1, 2), (1, 5, 1), (1, 1, 1), (2, 2, 2), (2, 4, 3, 6), (2, 1, 3, 1, 2)]


def test_the_class_against_the_loops():
    from sph_raytracer_amd.loss import IsoTVRegularizer
    rng = np.random.default_rng(2)
    for shape in SHAPES:
        d = rng.standard_normal(shape)
        dt = tr.from_numpy(d)
        for wrap in (False, True):
            for weights in ic.WEIGHTS + [(1.0, 1.0, 1.0), (0.0, 0.0, 0.0)]:
                reg = IsoTVRegularizer(weights=weights, wrap_a=wrap)
                assert reg.wraps(None) is wrap
                want = ic.iso_value(d, weights, wrap)
                got = float(reg(None, None, dt, None))
                assert abs(got - want) <= 1e-14 * max(abs(want), 1e-300), (shape, wrap, weights)
                assert abs(float(3.0 * reg.formula(dt, wrap)) - 3.0 * want) <= 1e-13 * max(want, 1e-300)
                # float32 runs in its dtype
                assert reg(None, None, dt.float(), None).dtype == tr.float32
    # lam scales, the volume mask multiplies, use_grad=False detaches
    d = tr.from_numpy(rng.standard_normal((4, 3, 6))).requires_grad_()
    reg = 0.5 * IsoTVRegularizer(volume_mask=2.0)
    assert math.isclose(float(reg(None, None, d, None).detach()),
                        0.5 * ic.iso_value(2.0 * d.detach().numpy(), (1, 1, 1), False), rel_tol=1e-14)
    assert not IsoTVRegularizer(use_grad=False)(None, None, d, None).requires_grad
    # wrap_a=None: inferred from the grid as SmoothRegularizer infers it
    from sph_raytracer_amd import SphericalGrid
    from sph_raytracer_amd.loss import SmoothRegularizer
    f = tp._Shape((4, 3, 6))
    f.a_b = SphericalGrid(shape=(4, 3, 6)).a_b
    assert IsoTVRegularizer().wraps(f) is SmoothRegularizer().wraps(f)
    assert IsoTVRegularizer().wraps(None) is False


def test_one_axis_with_edges_is_the_abs_kind():
    from sph_raytracer_amd.loss import IsoTVRegularizer, SmoothRegularizer
    rng = np.random.default_rng(3)
    for shape, weights in (((4, 3, 6), (1.5, 0, 0)), ((4, 3, 6), (0, 0.5, 0)), ((4, 3, 6), (0, 0, 2.0)),
                           ((1, 5, 1), (1, 1, 1)), ((3, 1, 2), (0, 1, 2.0)), ((2, 1, 1, 7), (3, 2, 0.25))):
        d = tr.from_numpy(rng.standard_normal(shape))
        for wrap in (False, True):
            a = IsoTVRegularizer(weights=weights, wrap_a=wrap)(None, None, d, None)
            b = SmoothRegularizer(weights=weights, kind='abs', wrap_a=wrap)(None, None, d, None)
            assert abs(float(a) - float(b)) <= 1e-14 * abs(float(b)), (shape, weights, wrap)


def test_the_gradient_is_finite_and_zero_on_flat_voxels():
    from sph_raytracer_amd.loss import IsoTVRegularizer
    for wrap in (False, True):
        d = tr.full((4, 3, 6), 0.7, dtype=F64, requires_grad=True)
        val = IsoTVRegularizer(weights=(1, 0.5, 2), wrap_a=wrap)(None, None, d, None)
        val.backward()
        assert float(val.detach()) == 0.0 and not d.grad.any() and bool(tr.isfinite(d.grad).all())
    # one jump: the gradient is finite everywhere and agrees with a central difference
    rng = np.random.default_rng(5)
    base = np.full((4, 3, 6), 0.3)
    base[2:] = 0.9
    base[1, 1, 2] += 0.05
    d = tr.from_numpy(base).requires_grad_()
    reg = IsoTVRegularizer(weights=(1, 0.5, 2), wrap_a=True)
    reg(None, None, d, None).backward()
    assert bool(tr.isfinite(d.grad).all()) and d.grad.any()
    for idx in ((1, 1, 2), (2, 0, 0), (1, 1, 3)):
        h = 1e-6
        up_, dn = base.copy(), base.copy()
        up_[idx] += h
        dn[idx] -= h
        fd = (ic.iso_value(up_, (1, 0.5, 2), True) - ic.iso_value(dn, (1, 0.5, 2), True)) / (2 * h)
        assert abs(float(d.grad[idx]) - fd) <= 1e-6 * max(abs(fd), 1e-3), idx
    del rng


def test_the_class_validates_its_arguments():
    from sph_raytracer_amd.loss import IsoTVRegularizer
    for bad in ((1, 1), (1, 1, 1, 1), 3, (1, -1, 1), (1, float('nan'), 1), (1, float('inf'), 1),
                (True, 1, 1), ('1', 1, 1), None):
        with pytest.raises(ValueError, match='IsoTVRegularizer needs three weights'):
            IsoTVRegularizer(weights=bad)
    for bad in (1, 0, 'yes', 1.0):
        with pytest.raises(ValueError, match='wrap_a must be True, False or None'):
            IsoTVRegularizer(wrap_a=bad)
    with pytest.raises(ValueError, match=r'IsoTVRegularizer needs a density.*\(3, 6\)'):
        IsoTVRegularizer()(None, None, tr.zeros(3, 6, dtype=F64), None)
    reg = IsoTVRegularizer(weights=[2, 0, 1], wrap_a=True, lam=3)
    assert reg.weights == (2.0, 0.0, 1.0) and reg.wrap_a is True and reg.lam == 3


# ---- iso_cases on its own references ---------------------------------------------------------------------
def test_exact_dual_cases_are_exact():
    """In Fractions: every voxel's n2 is a perfect square, the norm R 2^-j and the scale 2^j
    exact, the expected store v 2^j outside and v inside and on the tie; the float64 sequence
    `dual_ref` gives the same bits; all three sides occur."""
    for shape, wrap, weights in ic.kernel_cases():
        n = math.prod(shape)
        if n > 600:
            continue
        _, up = pc.neighbours(shape, wrap, ic.has_of(weights, shape))
        seen = set()
        for seed in range(4):
            xn, xo, q, sigma, radius, want, side = ic.exact_dual_case(shape, wrap, weights, seed)
            for i in range(n):
                axes = [ax for ax in range(3) if up[ax, i] >= 0]
                assert all(q[ax, i] == 0 for ax in range(3) if ax not in axes)
                if not axes:
                    continue
                n2 = sum(Fraction(q[ax, i]) ** 2 for ax in axes)
                root = Fraction(math.isqrt(n2.numerator), math.isqrt(n2.denominator))
                assert root * root == n2 and n2 < 2 ** 53
                cmp_ = (root > radius) - (root < radius)
                assert cmp_ == side[i]
                scale = Fraction(radius) / root if cmp_ > 0 else Fraction(1)
                assert scale in (Fraction(1, 2), Fraction(1))
                for ax in axes:
                    assert Fraction(want[ax, i]) == Fraction(q[ax, i]) * scale
                got, _ = ic.dual_ref(i, xn, xo, q, up, weights, radius, sigma)
                assert all(got[ax] is None or got[ax] == want[ax, i] for ax in range(3))
                seen.add(int(side[i]))
        assert n < 63 or not any(ic.has_of(weights, shape)) or seen == {-1, 0, 1}
    assert ic.BALL == 1 + Fraction(12, 2 ** 53)


def test_the_feasibility_bound_on_the_reference_sequence():
    """`dual_ref` itself (the header's sequence in float64) stays inside radius^2 (1 + 12 u),
    in Fractions, on random data over several decades of the radius."""
    shape, weights = (5, 7, 9), (1.0, 0.5, 2.0)
    _, up = pc.neighbours(shape, True, (1, 1, 1))
    _, _, q, xn, xo = pc.random_vectors(shape, seed=77)
    worst = Fraction(0)
    for radius in (1.3, 0.37, 1e-3, 7.7e-7):
        out = np.zeros((3, 315))
        for i in range(315):
            got, _ = ic.dual_ref(i, xn, xo, q, up, weights, radius, 0.23)
            out[:, i] = got
        worst = max(worst, ic.ball_excess(out, up, radius))
    print(f'largest sum q^2 / r^2 - 1: {float((worst - 1) * 2 ** 53):.3g} u')
    assert 1 < worst <= ic.BALL


def test_iso_dense_and_the_certificate_on_a_known_problem():
    """Two voxels, N = I, one edge: with one axis the iso term is the abs term, whose minimiser
    is known in closed form (test_pd_cpu.py); iso_dense reaches it and the certificate's radius
    covers the distance.  And on the 4 x 3 x 6 grid with weights (1, 0.5, 2) |Dw|^2 is the
    issue's 20.16 (ring) and 19.09 (open) against B = 21."""
    N, D, B = np.eye(2), np.array([[-1.0, 1.0]]), 4.0
    voxel = np.array([0])
    for b, r, want in ((np.array([0.0, 1.0]), 0.25, [0.25, 0.75]),
                       (np.array([0.0, 1.0]), 0.75, [0.5, 0.5])):
        x, q, radius = ic.certify(N, b, D, voxel, r, -math.inf, math.inf, 1.0, B)
        assert np.allclose(x, want, rtol=0, atol=1e-12) and radius <= 1e-7
        assert np.linalg.norm(x - want) <= radius + 1e-15
        xs, qk, mm, qq = ic.iso_dense(N, b, D, voxel, r, -math.inf, math.inf, 1.0, 1.0, 50, B)
        xp, qp, _, _ = pc.pd_dense(N, b, D, np.array([r]), -math.inf, math.inf, 1.0, 1.0, 50, B)
        assert len(xs) == 51 and np.allclose(xs[-1], xp[-1], rtol=0, atol=1e-15)
        assert abs(qk[0]) <= r * (1 + 12 * ic.U)
    for wrap, norm2 in ((True, 20.16), (False, 19.09)):
        Dw, voxel, Bw = ic.iso_matrix((4, 3, 6), wrap, (1.0, 0.5, 2.0))
        assert Bw == 21.0 and abs(np.linalg.norm(Dw, 2) ** 2 - norm2) < 0.005
        assert len(voxel) == len(Dw) and voxel.max() < 72
    # the value through the matrix is the loops' value
    rng = np.random.default_rng(8)
    x = rng.standard_normal((4, 3, 6))
    for wrap in (False, True):
        Dw, voxel, _ = ic.iso_matrix((4, 3, 6), wrap, ic.TV_WEIGHTS)
        got = ic.norms(Dw @ x.reshape(-1), voxel, 72).sum() / 72
        assert abs(got - ic.iso_value(x, ic.TV_WEIGHTS, wrap)) <= 1e-14


# ---- the solvers' refusals -------------------------------------------------------------------------------
def test_the_solvers_refuse_bad_iso_terms_by_name():
    from sph_raytracer_amd.loss import AbsLoss, IsoTVRegularizer, SmoothRegularizer, SquareLoss
    from sph_raytracer_amd.retrieval import chambolle_pock, primal_dual
    y, f = tr.zeros(2, 6, 6, dtype=F64), tp._Shape((4, 3, 6))
    iso = lambda **kw: 0.1 * IsoTVRegularizer(**kw)                       # noqa: E731
    tv = lambda: 0.1 * SmoothRegularizer(kind='abs')                      # noqa: E731
    bad = [([iso(), tv()], 'IsoTVRegularizer.*beside|beside.*IsoTVRegularizer'),
           ([tv(), iso()], 'beside'), ([iso(), iso()], 'one IsoTVRegularizer, not'),
           ([0.0 * IsoTVRegularizer()], 'lam > 0.*IsoTVRegularizer|IsoTVRegularizer.*lam'),
           ([-1.0 * IsoTVRegularizer()], 'lam'), ([tr.tensor(2.0) * IsoTVRegularizer()], 'lam'),
           ([float('inf') * IsoTVRegularizer()], 'lam'),
           ([iso(volume_mask=2)], 'volume_mask.*IsoTVRegularizer'),
           ([iso(projection_mask=2)], 'projection_mask.*IsoTVRegularizer'),
           ([iso(use_grad=False)], r'IsoTVRegularizer\(use_grad=False\)'),
           ([iso(weights=(0, 0, 0))], r'IsoTVRegularizer\(weights=.*no edges')]
    for solver, fid in ((primal_dual, SquareLoss), (chambolle_pock, AbsLoss)):
        for fns, word in bad:
            with pytest.raises(ValueError, match=solver.__name__ + '.*(' + word + ')'):
                solver(f, y, [fid()] + fns)                 # (refused before the operator is used)
        with pytest.raises(ValueError, match='no edges'):
            solver(tp._Shape((4, 1, 6)), y, [fid(), iso(weights=(0, 1, 0))])
        with pytest.raises(ValueError, match='r, e, a'):
            solver(f, y, [fid(), iso()], x0=tr.zeros(3, 6, dtype=F64))
    with pytest.raises(ValueError, match="chambolle_pock: precondition='diagonal' with an "
                                         'IsoTVRegularizer is not built'):
        chambolle_pock(f, y, [AbsLoss(), iso()], precondition='diagonal')
    # the abs term's refusals keep their words
    with pytest.raises(ValueError, match="kind='abs'.*not 2"):
        primal_dual(f, y, [SquareLoss(), tv(), tv()])
    with pytest.raises(ValueError, match=r"at most one SmoothRegularizer\(kind='abs'\), not two"):
        chambolle_pock(f, y, [AbsLoss(), tv(), tv()])
    with pytest.raises(ValueError, match=r"needs one SmoothRegularizer\(kind='abs'\).*fista"):
        primal_dual(f, y, [SquareLoss()])


def test_gd_declines_the_class_from_its_direct_loops():
    """`_loop_terms` with everything else as the direct loops want it (stand-ins for the GPU
    tensors: it reads attributes only) accepts the fidelity term alone and declines the list once
    an IsoTVRegularizer is in it, wherever it stands."""
    from sph_raytracer_amd.loss import IsoTVRegularizer, NegRegularizer, SquareLoss
    from sph_raytracer_amd.model import FullyDenseModel
    from sph_raytracer_amd.retrieval import _loop_terms
    y = tr.zeros(2, 6, 6, dtype=F64)
    coeffs = types.SimpleNamespace(dtype=F64, is_cuda=True, device=y.device, shape=(4, 3, 6),
                                   is_contiguous=lambda: True)
    f = types.SimpleNamespace(_cdev=y.device, grid=types.SimpleNamespace(shape=(4, 3, 6)),
                              _ray_shape=(2, 6, 6))
    model = object.__new__(FullyDenseModel)
    sq, neg = SquareLoss(), NegRegularizer()
    assert _loop_terms(f, y, model, coeffs, [sq, neg], [coeffs]) == (sq, neg)
    for fns in ([sq, IsoTVRegularizer()], [IsoTVRegularizer(), sq], [sq, neg, 0.1 * IsoTVRegularizer()]):
        assert _loop_terms(f, y, model, coeffs, fns, [coeffs]) is None


# ---- the recorded measurements ---------------------------------------------------------------------------
def _system(name, masked, wrap):
    """(quadratic terms, damp, N, b, Dw, voxel, B, L, r) of a variant: test_pd_cpu's system with
    the iso term's weighted difference matrix."""
    fns, damp, N, b, _, _, _, L = tp._system(name, masked, wrap)
    shape = tuple(tp._operator(name)[0].grid.shape)
    Dw, voxel, B = ic.iso_matrix(shape, pc.tv_wrap(masked), ic.TV_WEIGHTS)
    return fns, damp, N, b, Dw, voxel, B, L, ic.LAM_TV / len(b)


_CERTIFIED = {}


def _certified(name, masked, wrap, lower, upper):
    key = (name, masked, wrap, lower, upper)
    if key not in _CERTIFIED:
        _, _, N, b, Dw, voxel, B, L, r = _system(name, masked, wrap)
        _CERTIFIED[key] = ic.certify(N, b, Dw, voxel, r, *tp._inf(lower, upper), L, B)
    return _CERTIFIED[key]


@pytest.mark.parametrize('name', ['tiny', 'two_workgroups'])
def test_certificate_and_recorded_iterations(name):
    assert ic.RADIUS_MAX <= ic.STAYS_UNDER and ic.ITERATIONS <= pc.K_CAP
    for masked, wrap in pc.VARIANTS:
        for lower, upper in tp.BOUNDS:
            key = (name, masked, wrap, lower is not None)
            _, _, N, b, Dw, voxel, B, L, r = _system(name, masked, wrap)
            want, q, radius = _certified(name, masked, wrap, lower, upper)
            xs, _, _, _ = ic.iso_dense(N, b, Dw, voxel, r, *tp._inf(lower, upper), L,
                                       pc.DUAL_RATIO, ic.ITERATIONS + 2000, B)
            errs = [cc.rel_err(x, want) for x in xs]
            k, at = pc.first_stays_under(errs, ic.STAYS_UNDER), errs[ic.ITERATIONS]
            radius = radius / np.linalg.norm(want)
            flat, jump = ic.ball_shares(q, voxel, len(b), r)
            print(key, k, at, radius, flat, jump)
            assert radius <= ic.RADIUS_MAX, key
            assert flat > 0 and jump > 0, key
            assert k is not None and k <= ic.ITERATIONS, key
            assert 100 * at <= ic.LIMIT and ic.LIMIT >= ic.RADIUS_MAX, key
            rec_k, rec_at, rec_radius = ic.MEASURED[key]
            assert abs(rec_k - k) <= 1, (key, k)
            assert math.isclose(at, rec_at, rel_tol=0.05, abs_tol=1e-9), (key, at)
            assert math.isclose(radius, rec_radius, rel_tol=0.05), (key, radius)
    assert max(v[0] for v in ic.MEASURED.values()) == ic.ITERATIONS
    worst = 100 * max(v[1] for v in ic.MEASURED.values())
    assert worst <= ic.LIMIT <= 1.01 * max(worst, ic.RADIUS_MAX)


# ---- the solvers against iso_dense -----------------------------------------------------------------------
@pytest.mark.parametrize('lower,upper', tp.BOUNDS)
@pytest.mark.parametrize('masked,wrap', pc.VARIANTS)
def test_primal_dual_follows_iso_dense(masked, wrap, lower, upper):
    from sph_raytracer_amd.retrieval import primal_dual
    op, y, mask = tp._operator()
    fns, damp, N, b, Dw, voxel, B, _, r = _system('tiny', masked, wrap)
    fns = list(fns) + [ic.tv_term(pc.tv_wrap(masked))]
    lo, hi = tp._inf(lower, upper)
    L2 = 1.25 * float(np.linalg.eigvalsh(N)[-1])
    x, y_hat, info = primal_dual(op, y, fns, damp=damp, lower=lower, upper=upper, num_iterations=40,
                                 lipschitz=L2, dual_ratio=0.5)
    xs, qk, mm, qq = ic.iso_dense(N, b, Dw, voxel, r, lo, hi, L2, 0.5, 40, B)
    assert info['lipschitz'] == L2 and (info['tau'], info['sigma']) == pc.pd_steps(L2, 0.5, B)
    assert tr.equal(y_hat, op(x)) and cc.rel_err(x.numpy(), xs[-1]) <= 1e-12
    q = info['dual']
    assert q.shape == (3, 4, 3, 6) and q.dtype == F64
    _, up = pc.neighbours((4, 3, 6), pc.tv_wrap(masked), (1, 1, 1))
    qn = q.numpy().reshape(3, -1)
    assert not qn[up < 0].any() and not np.signbit(qn[up < 0]).any()     # +0.0 where no edge
    assert np.allclose(ic.flat_dual(q, up), qk, rtol=0, atol=1e-12 * r)
    assert ic.ball_excess(qn, up, r) <= ic.BALL
    assert (ic.norms(qk, voxel, 72) >= r * (1 - 1e-9)).any()            # the projection acted
    assert np.allclose(info['primal_change'], np.sqrt(np.array(mm) / mm[0]), rtol=1e-9)
    assert np.allclose(info['dual_change'], np.sqrt(qq), rtol=1e-9, atol=1e-18)
    xn = x.numpy().reshape(-1)
    assert np.all((xn >= lo) & (xn <= hi))


def test_primal_dual_reaches_the_certified_minimiser():
    from sph_raytracer_amd.retrieval import primal_dual
    op, y, mask = tp._operator()
    fns, damp, N, b, Dw, voxel, B, L, r = _system('tiny', True, False)
    want, _, _ = _certified('tiny', True, False, pc.LOWER, pc.UPPER)
    x, _, info = primal_dual(op, y, list(fns) + [ic.tv_term(pc.tv_wrap(True))], damp=damp,
                             lower=pc.LOWER, upper=pc.UPPER, num_iterations=ic.ITERATIONS)
    assert cc.rel_err(x.numpy(), want) <= ic.LIMIT
    assert abs(info['lipschitz'] - L) <= 1e-12 * L
    assert (info['tau'], info['sigma']) == pc.pd_steps(info['lipschitz'], 1.0, B)


def _cp_dense(A, s2, yv, Dw, voxel, r, c, lower, upper, LA, B, s_bar, K):
    """chambolle_pock with a SquareLoss restated on the dense matrix: the ray dual's prox is
    t / (1 + sigma / (2 s)), t = a - sigma y (retrieval.chambolle_pock's docstring)."""
    kn2 = LA + B
    kn = math.sqrt(kn2)
    sigma = s_bar / kn
    tau = 1.0 / (sigma * kn2 + c)
    n = A.shape[1]
    x, p, q = np.clip(np.zeros(n), lower, upper), np.zeros(len(yv)), np.zeros(len(Dw))
    z = A @ x
    for _ in range(K):
        u = x - tau * ((A.T @ p + c * x) + Dw.T @ q)
        x_new = np.where(u < lower, lower, np.where(u > upper, upper, u))
        q = ic.project(q + sigma * (Dw @ (2 * x_new - x)), voxel, n, r)
        z_new = A @ x_new
        a = p + sigma * (2 * z_new - z)
        with np.errstate(all='ignore'):
            p = np.where(s2 == 0, 0.0, (a - sigma * yv) / (1.0 + sigma / (2.0 * s2)))
        x, z = x_new, z_new
    return x, p, q, tau, sigma


@pytest.mark.parametrize('masked', [False, True])
def test_chambolle_pock_follows_its_dense_restatement(masked):
    from sph_raytracer_amd.retrieval import chambolle_pock
    op, y, mask, A = cp.problem('tiny')
    s, _ = cp.ray_factors(y, mask, masked)
    Dw, voxel, B = ic.iso_matrix((4, 3, 6), True, ic.TV_WEIGHTS)
    norm = 1.1 * float(np.linalg.norm(A, 2) ** 2)
    x, _, info = chambolle_pock(op, y, [cp.fidelity('square', mask if masked else 1), ic.tv_term(True)],
                                damp=cp.DAMP, lower=cp.LOWER, upper=cp.UPPER, num_iterations=40,
                                norm=norm)
    xd, pd_, qd, tau, sigma = _cp_dense(A, s, y.numpy().reshape(-1), Dw, voxel, ic.LAM_TV / 72,
                                        2 * cp.DAMP / 72, cp.LOWER, cp.UPPER, norm, B,
                                        cp.LAM_F / y.numel(), 40)
    assert math.isclose(info['tau'], tau, rel_tol=1e-14) and math.isclose(info['sigma'], sigma, rel_tol=1e-14)
    assert cc.rel_err(x.numpy(), xd) <= 1e-12
    _, up = pc.neighbours((4, 3, 6), True, (1, 1, 1))
    assert np.allclose(ic.flat_dual(info['dual'], up), qd, rtol=0, atol=1e-12 * ic.LAM_TV / 72)
    assert np.allclose(info['ray_dual'].numpy().reshape(-1), pd_, rtol=0, atol=1e-12 * np.abs(pd_).max())
    assert info['dual'].shape == (3, 4, 3, 6)
    assert ic.ball_excess(info['dual'].numpy().reshape(3, -1), up, ic.LAM_TV / 72) <= ic.BALL


CP_CASES = ic.cp_cases()


@pytest.mark.parametrize('case', CP_CASES, ids=[cp.case_id(c) for c in CP_CASES])
def test_chambolle_pock_closes_the_duality_gap(case):
    name, kind, tv, masked, damp, lower, upper = case
    x, y_hat, info = ic.cp_solve(case)
    J, D, gap = ic.cp_gap(case, x, info)
    rec = ic.CP_MEASURED[cp.case_id(case)]
    print(f'{cp.case_id(case)}: J {J:.6g}, D {D:.6g}, gap {gap:.3g} (recorded {rec:.3g})')
    assert D <= J + cp.WEAK_DUALITY_SLACK * abs(J)              # weak duality
    assert gap <= ic.CP_GAP_LIMIT[kind]
    # as recorded, to a couple of digits (below the floor: compared absolutely)
    assert math.isclose(gap, rec, rel_tol=0.05, abs_tol=cp.GAP_FLOOR)
    xn = x.numpy().reshape(-1)
    assert np.all(xn >= lower) and (upper is None or np.all(xn <= upper))
    shape = tuple(x.shape)
    _, up = pc.neighbours(shape, True, (1, 1, 1))
    assert ic.ball_excess(info['dual'].numpy().reshape(3, -1), up, ic.LAM_TV / xn.size) <= ic.BALL


def test_the_gap_limits_are_the_rule_s():
    for kind in cp.KINDS:
        worst = 100 * max(v for k, v in ic.CP_MEASURED.items() if f'-{kind}-' in k)
        assert max(worst, cp.GAP_FLOOR) <= ic.CP_GAP_LIMIT[kind] <= 1.01 * max(worst, cp.GAP_FLOOR)
    assert sorted(ic.CP_MEASURED) == sorted(cp.case_id(c) for c in CP_CASES)


def test_other_inputs_solve_on_the_generic_path():
    """A float32 start runs in its dtype; a dynamic operator runs the iso term over each slice's
    r, e, a: held to iso_dense on the block system."""
    from cpu_operator import CpuOperator
    from sph_raytracer_amd import SphericalGrid
    from sph_raytracer_amd.loss import SquareLoss
    from sph_raytracer_amd.retrieval import primal_dual
    op, y, mask = tp._operator()
    fns, damp, N, b, Dw, voxel, B, L, r = _system('tiny', True, False)
    want = _certified('tiny', True, False, pc.LOWER, pc.UPPER)[0]
    fns = list(fns) + [ic.tv_term(pc.tv_wrap(True))]
    x32, _, i32 = primal_dual(op, y, fns, damp=damp, lower=pc.LOWER, upper=pc.UPPER,
                              num_iterations=2000, x0=tr.zeros(4, 3, 6, dtype=tr.float32))
    assert x32.dtype == tr.float32 and i32['dual'].dtype == tr.float32
    # (float32 rounding 6e-8 at a condition number of at most 100: test_pd_cpu's bound)
    assert cc.rel_err(x32.double().numpy(), want) <= 1e-4
    dgrid = SphericalGrid(shape=(2, 4, 3, 6))
    dop = CpuOperator(dgrid, op.geom)
    g = tr.Generator().manual_seed(3)
    yd = dop(tr.rand(tuple(dgrid.shape), dtype=F64, generator=g)).detach()
    quad = [2.0 * SquareLoss()]
    N0, _, _ = cc.dense_system(dop, yd, quad, 0.0, tuple(dgrid.shape))
    ddamp = cc.damp_for(N0, 144)
    Nd, bd, _ = cc.dense_system(dop, yd, quad, ddamp, tuple(dgrid.shape))
    D1, v1, B1 = ic.iso_matrix((4, 3, 6), True, ic.TV_WEIGHTS)
    Dd, vd = np.kron(np.eye(2), D1), np.concatenate([v1, v1 + 72])
    Ld = 1.05 * float(np.linalg.eigvalsh(Nd)[-1])
    xs, qk, mm, _ = ic.iso_dense(Nd, bd, Dd, vd, ic.LAM_TV / 144, pc.LOWER, pc.UPPER, Ld, 1.0, 40, B1)
    xt, yh, info = primal_dual(dop, yd, quad + [ic.tv_term(True)], damp=ddamp, lower=pc.LOWER,
                               upper=pc.UPPER, num_iterations=40, lipschitz=Ld)
    assert xt.shape == tuple(dgrid.shape) and info['dual'].shape == (3,) + tuple(dgrid.shape)
    assert cc.rel_err(xt.numpy(), xs[-1]) <= 1e-12
    _, up = pc.neighbours((4, 3, 6), True, (1, 1, 1))
    qt = info['dual'].numpy().reshape(3, 2, -1)
    flat = np.concatenate([qt[ax, s][up[ax] >= 0] for s in range(2) for ax in range(3)])
    assert np.allclose(flat, qk, rtol=0, atol=1e-12 * ic.LAM_TV / 144)
    assert np.allclose(info['primal_change'], np.sqrt(np.array(mm) / mm[0]), rtol=1e-9)
