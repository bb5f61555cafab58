"""Stream order of the isotropic-TV branch of retrieval.primal_dual and retrieval.chambolle_pock
and of the two entries of include/sphrt_iso.h, behind the gate of stream_gate.py: one test per
row of iso_stream_cases.ROWS, run by test_gpu_stream_order.check_row itself as
test_gpu_dp_stream.py runs dp_stream_cases' rows — the reference on the default stream, the gated
run on a side stream whose inputs hold NaN until a spin has passed, the entries reached, the gate
still closed at the solve's single Tensor.cpu() readback, the caller's inputs unchanged.  The
entries outside include/sphrt.h are counted through check_row's `mutate` hook: the two new ones
once per iteration each, and the two of include/sphrt_pd.h never."""
import pytest

import iso_stream_cases as isc
import stream_cases as sc
from test_gpu_stream_order import _Counted, check_row

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', isc.NAMES)
def test_row(name, gpu, monkeypatch):
    row = isc.BY_NAME[name]
    assert set(isc.ISO_ENTRIES) <= set(row.entries) and row.readbacks == 1
    monkeypatch.setitem(sc.RECIPES, row.recipe, isc.RECIPES[row.recipe])
    counts = {}
    known = set(sc.stream_entries())
    own = [e for e in row.entries if e not in known]
    assert set(own) >= set(isc.ISO_ENTRIES)
    watched = own + ['sphrt_pd_primal_f64', 'sphrt_pd_dual_f64']

    def count_own(mp, lib):
        for entry in watched:
            mp.setattr(lib, entry, _Counted(getattr(lib, entry), entry, counts))

    check_row(row._replace(entries=tuple(e for e in row.entries if e in known)), gpu, monkeypatch,
              mutate=count_own)
    assert counts == {entry: sc.SOLVE_ITERATIONS for entry in own}, counts
