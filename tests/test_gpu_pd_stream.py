"""Stream order of retrieval.primal_dual's launches, behind the gate of stream_gate.py: one test
per row of pd_stream_cases.ROWS, run by test_gpu_stream_order.check_row itself — its steps (1) to
(5): the reference on the default stream, the gated run on a side stream whose inputs hold NaN
until a spin has passed (compared bitwise where the row is reproducible, within
cg_cases.SOLVE_TOL of the default-stream solve where float64 atomics sum, no NaN anywhere), the
entries reached, the gate still closed at the solve's single Tensor.cpu() readback (rows over a
masked deterministic operator read max|ray_scale| back first, as fista's do: no claim there),
the caller's inputs unchanged; a fresh `setup` before every run and the row's environment, as
for every other row.

check_row looks its recipe up in stream_cases.RECIPES and counts the entries of include/sphrt.h;
the recipe of these rows is entered there for the test's duration, and the two entries of
include/sphrt_pd.h are counted through check_row's `mutate` hook, which installs patches for the
gated run alone."""
import pytest

import pd_stream_cases as psc
import stream_cases as sc
from test_gpu_stream_order import _Counted, check_row

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', psc.NAMES)
def test_row(name, gpu, monkeypatch):
    row = psc.BY_NAME[name]
    assert set(psc.PD_ENTRIES) <= set(row.entries) and row.readbacks == 1
    monkeypatch.setitem(sc.RECIPES, row.recipe, psc.RECIPES[row.recipe])
    counts = {}

    def count_pd(mp, lib):
        for entry in psc.PD_ENTRIES:
            mp.setattr(lib, entry, _Counted(getattr(lib, entry), entry, counts))

    known = set(sc.stream_entries())
    check_row(row._replace(entries=tuple(e for e in row.entries if e in known)), gpu, monkeypatch,
              mutate=count_pd)
    # both new entries, once per iteration of the gated solve
    assert counts == {entry: sc.SOLVE_ITERATIONS for entry in psc.PD_ENTRIES}, counts
