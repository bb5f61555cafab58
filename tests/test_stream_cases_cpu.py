"""The table of stream_cases.py against include/sphrt.h, without a GPU: every C entry that takes
a stream is declared by a row of the table or stands in EXEMPT with a written reason, and EXEMPT
holds at most a tenth of them."""
import gd_cases as gc
import stream_cases as sc
from sph_raytracer_amd import _lib


def test_header_parse_finds_the_stream_entries():
    entries = sc.stream_entries()
    assert len(entries) == len(set(entries)) and len(entries) >= 50
    # the ctypes signatures say the same: the last argument of each is the void* stream
    sigs = {name: args for name, _, args in _lib._SIGNATURES}
    for name in entries:
        assert name in sigs and sigs[name][-1] is _lib.c_vp, name
    # entries the header declares without a stream are not in the list
    for name in ('sphrt_time_next_forward', 'sphrt_forward_plan', 'sphrt_loss_partials',
                 'sphrt_plan_create'):
        assert name in sigs and name not in entries


def test_every_stream_entry_is_declared_or_exempt():
    entries = set(sc.stream_entries())
    declared = {e for row in sc.ROWS for e in row.entries}
    assert declared <= entries, sorted(declared - entries)          # (no misspelt entry)
    assert set(sc.EXEMPT) <= entries, sorted(set(sc.EXEMPT) - entries)
    assert not declared & set(sc.EXEMPT), sorted(declared & set(sc.EXEMPT))
    missing = entries - declared - set(sc.EXEMPT)
    assert not missing, sorted(missing)
    assert all(isinstance(why, str) and len(why) > 10 for why in sc.EXEMPT.values())
    assert 10 * len(sc.EXEMPT) <= len(entries), (len(sc.EXEMPT), len(entries))


def test_rows_are_well_formed():
    assert len(sc.NAMES) == len(set(sc.NAMES))
    names = set(sc.NAMES)
    for case in gc.NAMES:
        assert 'gd-' + case in names, case
    for row in sc.ROWS:
        assert row.recipe in sc.RECIPES and row.entries, row.name
        assert row.nosync in (None, 'return', 'readback')
        assert (row.nosync == 'readback') <= (row.readbacks is not None)
        assert row.bitwise == (row.bound is None), row.name
        assert row.native in (None, 'fast', 'construct')
        if row.after:
            assert hasattr(sc.RECIPES[row.recipe], 'after'), row.name
    # the solver rows the table promises: four variants x three operators on tiny and one on
    # two_workgroups, for cg and for fista
    for solver in ('cg', 'fista'):
        rows = [r for r in sc.ROWS if r.recipe == 'solve' and r.params['solver'] == solver]
        assert len(rows) == len(sc.VARIANTS) * len(sc.OPERATORS) + 1
        assert all(r.readbacks == 1 for r in rows)
    # every documented sync-free family has a row that asserts it
    for prefix in ('stored-forward', 'stored-T', 'mf-T', 'mf-call', 'mf-residual-gradient',
                   'gd-', 'cg-', 'fista-'):
        assert any(r.name.startswith(prefix) and r.nosync for r in sc.ROWS), prefix
