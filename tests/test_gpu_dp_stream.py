"""Stream order of retrieval.chambolle_pock(precondition='diagonal') and of the three entries of
include/sphrt_dp.h, behind the gate of stream_gate.py: one test per row of dp_stream_cases.ROWS,
run by test_gpu_stream_order.check_row itself as test_gpu_cp_stream.py runs cp_stream_cases' rows
— the reference on the default stream, the gated run on a side stream whose inputs hold NaN until
a spin has passed, the entries reached, the gate still closed at the solve's single Tensor.cpu()
readback, the caller's inputs unchanged.  The entries of include/sphrt_pd.h and include/sphrt_dp.h
are counted through check_row's `mutate` hook: the primal step, the TV dual and the ray dual once
per iteration, the steps launch once per solve."""
import pytest

import dp_stream_cases as dsc
import stream_cases as sc
from test_gpu_stream_order import _Counted, check_row

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', dsc.NAMES)
def test_row(name, gpu, monkeypatch):
    row = dsc.BY_NAME[name]
    assert set(dsc.DP_ENTRIES) <= set(row.entries) and row.readbacks == 1
    monkeypatch.setitem(sc.RECIPES, row.recipe, dsc.RECIPES[row.recipe])
    counts = {}
    known = set(sc.stream_entries())
    own = [e for e in row.entries if e not in known]
    assert set(own) >= set(dsc.DP_ENTRIES)

    def count_own(mp, lib):
        for entry in own:
            mp.setattr(lib, entry, _Counted(getattr(lib, entry), entry, counts))

    check_row(row._replace(entries=tuple(e for e in row.entries if e in known)), gpu, monkeypatch,
              mutate=count_own)
    assert counts == {entry: dsc.launches(entry) for entry in own}, counts
