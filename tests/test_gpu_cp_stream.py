"""Stream order of retrieval.chambolle_pock's launches, behind the gate of stream_gate.py: one
test per row of cp_stream_cases.ROWS, run by test_gpu_stream_order.check_row itself — its steps
(1) to (5): the reference on the default stream, the gated run on a side stream whose inputs hold
NaN until a spin has passed (compared bitwise where the row is reproducible, within
cg_cases.SOLVE_TOL of the default-stream solve where float64 atomics sum, no NaN anywhere), the
entries reached, the gate still closed at the solve's single Tensor.cpu() readback, the caller's
inputs unchanged; a fresh `setup` before every run, as for every other row.

check_row looks its recipe up in stream_cases.RECIPES and counts the entries of include/sphrt.h;
the recipe of these rows is entered there for the test's duration, and the entries of
include/sphrt_pd.h and include/sphrt_cp.h are counted through check_row's `mutate` hook, which
installs patches for the gated run alone."""
import pytest

import cp_stream_cases as csc
import stream_cases as sc
from test_gpu_stream_order import _Counted, check_row

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', csc.NAMES)
def test_row(name, gpu, monkeypatch):
    row = csc.BY_NAME[name]
    assert set(csc.CP_ENTRIES) <= set(row.entries) and row.readbacks == 1
    monkeypatch.setitem(sc.RECIPES, row.recipe, csc.RECIPES[row.recipe])
    counts = {}
    known = set(sc.stream_entries())
    own = [e for e in row.entries if e not in known]

    def count_own(mp, lib):
        for entry in own:
            mp.setattr(lib, entry, _Counted(getattr(lib, entry), entry, counts))

    check_row(row._replace(entries=tuple(e for e in row.entries if e in known)), gpu, monkeypatch,
              mutate=count_own)
    # the launches of the loop itself, once per iteration of the gated solve
    assert counts == {entry: sc.SOLVE_ITERATIONS for entry in own}, counts
