"""Helpers shared by the GPU test modules (no tests here)."""
import torch as tr


def exact_stats(grid, geom, gpu):
    """(deferred rays, depth-limit ranges rank-sorted, ranges heap-sorted by one lane) of a count
    pass: the trace workspace's counters (trace.hip launch_trace, exact_heap_range)."""
    from sph_raytracer_amd import _lib, raytracer as rt
    lib = _lib.load()
    plan = rt._Plan(grid, gpu)
    batch = rt._RayBatch(grid, geom.ray_starts, rt._geom_rays(geom, gpu), gpu)
    counts = tr.empty(max(batch.n, 1), dtype=tr.int32, device=gpu)
    tws = rt._workspace(lib, plan, batch.n, gpu)
    _lib.check(lib.sphrt_trace_count(plan.handle, batch.desc, _lib.ptr(counts), _lib.ptr(tws),
                                     tws.numel(), _lib.stream_of(gpu)), 'sphrt_trace_count')
    head = tws[:256].cpu().view(tr.int64)
    return int(head[0]), int(head[16]), int(head[17])
