"""Stream order of every launch path, behind the gate of stream_gate.py: one test per row of
stream_cases.ROWS.

Per row: (1) the reference, the same call on the default stream (a fresh operator where the row
is about a first use); (2) the gated run on a side stream whose inputs hold NaN until a spin of D
ms has passed, compared bitwise where the row is reproducible and within the owning test file's
bound where float64 atomics sum (test_gpu_matrix_free's rtol 1e-12 / atol 1e-12 max|ref| for the
atomic adjoint — float32 results one float32 rounding of that —, gd_cases.bounds for gd,
cg_cases.SOLVE_TOL relative to the default-stream solve for cg / fista), no NaN anywhere; (3) the
C entries the row declares were all called (counted at the ctypes binding; rows that run through
the CPython entries count those entries' hits); (4) where the path is documented free of host
synchronisation the gate is still closed when the call returns, or — gd, cg, fista — at the one
Tensor.cpu() readback they end in; (5) the caller's inputs are unchanged.  Rows with a lazily
built piece use it again on the default stream afterwards.  Two further tests show that the gate
bites: a residual launch moved to another stream, and a synchronise hidden in a cg launch, both
fail the row's check.

Measured on one MI355X (wall time of the ungated call on a side stream with its synchronise ->
D = max(50 ms, 20 x that), spun by torch.cuda._sleep at 2.4e6 cycles per ms): MEASURED below,
from a run of this file; every row prints its own figures.  The whole file ran in 11 s.

Found by these rows and fixed with them: `_cg_direct` set `one[0] = 1.0`, a host scalar copied
into a 0-dim view — a pageable copy that waits for the stream (every cg-* row with a 'readback'
claim fails without the fill launch that replaced it); `_fista_direct` built its momentum table
with torch.tensor(list, device=...), the same kind of copy (every such fista-* row; the table
now goes up from pinned memory, not waited for)."""
import numpy as np
import pytest
import torch as tr

import cg_cases as cc
import gd_cases as gc
import stream_cases as sc
import stream_gate as sg

pytestmark = pytest.mark.gpu

# group of rows (the name's first word) -> (ungated call with its synchronise, ms: smallest and
# largest over the group's rows; D used, ms: smallest and largest)
MEASURED = {
    'stored': (0.08, 5.79, 50, 116),     # (the largest: the first float32 forward of the session)
    'dynamic': (0.05, 1.37, 50, 50),
    'construct': (0.48, 1.18, 50, 50),
    'mf': (0.08, 0.45, 50, 50),
    'smooth': (0.45, 0.45, 50, 50),
    'gd': (0.67, 1.83, 50, 50),
    'cg': (1.16, 1.74, 50, 50),
    'fista': (1.59, 2.48, 50, 50),
}


class _Counted:
    """A ctypes entry that counts its calls (and still casts to its address: raytracer binds
    the forward entries into the CPython entry by address)."""

    def __init__(self, fn, name, counts, before=None):
        self.fn, self.name, self.counts, self.before = fn, name, counts, before
        self._as_parameter_ = getattr(fn, '_as_parameter_', fn)

    def __call__(self, *a):
        self.counts[self.name] = self.counts.get(self.name, 0) + 1
        if self.before is not None:
            a = self.before(a)
        return self.fn(*a)


def _spy(mp, lib):
    counts = {}
    for name in sc.stream_entries():
        mp.setattr(lib, name, _Counted(getattr(lib, name), name, counts))
    return counts


def _clone(ins):
    return {k: v.clone() if isinstance(v, tr.Tensor) else v for k, v in ins.items()}


def _host(out):
    return [v.detach().cpu().clone() if isinstance(v, tr.Tensor) else list(v) for v in out]


def _bits(a):
    return a.contiguous().view(tr.uint8).reshape(-1)


def _compare(row, got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for k, (a, b) in enumerate(zip(got, ref)):
        where = f'{row.name} {what} output {k}'
        if isinstance(b, list):
            a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        else:
            assert a.shape == b.shape and a.dtype == b.dtype, where
            a, b = a.numpy(), b.numpy()
        assert a.shape == b.shape, where
        assert not np.isnan(a).any(), f'{where}: NaN'
        if row.bitwise:
            assert a.tobytes() == b.tobytes(), f'{where}: differs from the default stream'
    if row.bitwise:
        return
    if row.bound.startswith('atomic_adjoint'):
        for k, (a, b) in enumerate(zip(got, ref)):
            # float32 results: the float64 sums, within 1e-12, rounded once to float32
            tol = 1e-12 if b.dtype == tr.float64 else 2.0 ** -23
            assert tr.allclose(a, b, rtol=tol, atol=tol * float(b.abs().max())), \
                f'{row.name} {what} output {k}: differs from the default stream'
    elif row.bound == 'gd':
        name = row.params['case']
        b_c, b_y, b_h = gc.bounds(name)
        d_c, d_y = (float(np.abs(a.numpy() - b.numpy()).max()) for a, b in zip(got[:2], ref[:2]))
        d_h = [float(np.abs(np.subtract(p, q)).max()) for p, q in zip(got[2:], ref[2:])]
        print(f'{row.name} {what}: coefficients {d_c:.3g} ({b_c:.3g}), stack {d_y:.3g} '
              f'({b_y:.3g}), histories {d_h} ({b_h})')
        assert d_c <= b_c and d_y <= b_y, f'{row.name} {what}: differs from the default stream'
        assert all(d <= b for d, b in zip(d_h, b_h)), \
            f'{row.name} {what}: differs from the default stream'
    else:
        assert row.bound == 'solve'
        for k, (a, b) in enumerate(zip(got, ref)):
            a, b = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, b))
            if a.size:
                err = cc.rel_err(a, b)
                print(f'{row.name} {what} output {k}: relative error {err:.3g}')
                assert err <= cc.SOLVE_TOL, \
                    f'{row.name} {what} output {k}: differs from the default stream'


def check_row(row, gpu, monkeypatch, mutate=None):
    """Steps (1)-(5) of the module docstring for one row.  mutate(mp, lib): patches installed for
    the gated run alone (the tests that show the gate bites)."""
    from sph_raytracer_amd import _lib
    lib, recipe = _lib.load(), sc.RECIPES[row.recipe]
    for k, v in row.params.get('env', {}).items():
        monkeypatch.setenv(k, v)
    # (1) the reference on the default stream
    ctx = recipe.setup(row, gpu)
    ins = recipe.inputs(row, ctx, gpu)
    saved = _clone(ins)
    ref = _host(recipe.call(row, ctx, **_clone(ins)))
    ref_after = _host(recipe.after(row, ctx, **_clone(ins))) if row.after else None
    # the enqueue time's upper bound -> D
    ctx = recipe.setup(row, gpu)
    t_call = sg.measure(gpu, lambda: recipe.call(row, ctx, **_clone(ins)))
    # (2) the gated run
    ctx = recipe.setup(row, gpu)
    with monkeypatch.context() as mp:
        counts = _spy(mp, lib)
        if mutate is not None:
            mutate(mp, lib)
        with sg.gated(gpu, ins, t_call) as g:
            with sg.readbacks(g) as seen:
                out = recipe.call(row, ctx, **g.inputs)
            closed = g.closed()
        print(f'{row.name}: ungated call {t_call * 1e3:.2f} ms, D {g.d_ms:.0f} ms, gate closed at '
              f'return {closed}, at the readbacks {seen}')
        got = _host(out)
    _compare(row, got, ref, 'gated')
    # (3) the entries the row declares
    if row.native is None:
        missed = [e for e in row.entries if not counts.get(e)]
        assert not missed, f'{row.name}: entries not reached: {missed}'
    else:
        assert any(ctx['hits']), f'{row.name}: the {row.native} entry was not taken'
    # (4) no host synchronisation, where documented
    if row.nosync == 'return':
        assert closed, f'{row.name}: gate open at return: the call synchronised the host'
    elif row.nosync == 'readback':
        assert len(seen) == row.readbacks, f'{row.name}: {len(seen)} readbacks, gate open?'
        assert seen[0], f'{row.name}: gate open at the first readback: a hidden host sync'
    # (5) the caller's inputs
    assert g.unchanged(skip=row.mutated) == [], f'{row.name}: inputs changed'
    for k, v in ins.items():
        if isinstance(v, tr.Tensor) and not sg.is_value(v):
            assert g.inputs[k] is v and tr.equal(v, saved[k]), f'{row.name}: inputs changed'
    if row.after:      # the lazily built piece again, on the default stream
        _compare(row, _host(recipe.after(row, ctx, **_clone(ins))), ref_after, 'second use')


@pytest.mark.parametrize('name', sc.NAMES)
def test_row(name, gpu, monkeypatch):
    check_row(sc.BY_NAME[name], gpu, monkeypatch)


def test_gate_catches_a_misplaced_launch(gpu, monkeypatch):
    """The residual launch of a gd row sent to a second side stream: it runs while the gated
    stream still spins, reads the measurements before they exist (NaN), and the comparison fails.
    Floats only, read in bounds."""
    import ctypes
    other = tr.cuda.Stream(device=gpu)

    def mutate(mp, lib):
        def elsewhere(args):
            return args[:-1] + (ctypes.c_void_p(other.cuda_stream),)
        mp.setattr(lib, 'sphrt_sq_residual_f64',
                   _Counted(lib.sphrt_sq_residual_f64, 'moved', {}, before=elsewhere))
    row = sc.BY_NAME['gd-00-square-unit-f64-smooth-stored_in_order-adam_wd']
    assert 'sphrt_sq_residual_f64' in row.entries
    with pytest.raises(AssertionError, match='NaN|differs from the default stream'):
        check_row(row, gpu, monkeypatch, mutate)


def test_gate_catches_a_hidden_sync(gpu, monkeypatch):
    """torch.cuda.synchronize() before every sphrt_cg_update_f64 launch: the host waits out the
    spin, the gate is open at cg's readback, and the row's no-sync assertion fails."""
    def mutate(mp, lib):
        def synced(args):
            tr.cuda.synchronize()
            return args
        mp.setattr(lib, 'sphrt_cg_update_f64',
                   _Counted(lib.sphrt_cg_update_f64, 'synced', {}, before=synced))
    row = sc.BY_NAME['cg-tiny-unit-nosmooth-stored']
    assert row.nosync == 'readback' and 'sphrt_cg_update_f64' in row.entries
    with pytest.raises(AssertionError, match='gate open at the first readback'):
        check_row(row, gpu, monkeypatch, mutate)
