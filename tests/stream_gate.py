"""A gate that makes a launch on the wrong stream, a hidden host synchronisation and a buffer freed
across streams certain to show, instead of racing two streams and hoping (no tests; imported by
test_gpu_stream_order.py).

    with gated(gpu, inputs, enqueue_s) as g:    # inside: torch.cuda.stream(g.side) is current
        out = call(**g.inputs)
        # g.closed() may be asked here and right after the call returns
    # on exit: zero-filled junk on the default stream, then wait_stream, synchronize

`inputs` maps names to the true values.  Every floating tensor among them is a *value* input:
the call receives a device tensor of the same shape and dtype that holds NaN (written on the
default stream, synchronised), and the true values reach it through a copy enqueued on the side
stream behind a spin of D milliseconds and the event `gate`.  Everything the call enqueues is
therefore right only if it is ordered after those copies on the side stream:

  * a launch or memset on any other stream (the null stream, a stream remembered from
    construction, another device's) runs while the side stream still spins, reads NaN or stale
    state, and the result mismatches;
  * a hidden host synchronisation makes the host wait out the spin: `g.closed()`
    (`not gate.query()`) is then False when the call returns, or at its first readback;
  * a block the call handed back to the allocator while a gated kernel still needs it is
    overwritten on exit — on the default stream, which has not waited for the side stream — with
    all-zero bytes, before the gated kernels even start.  Zero bytes turn indices, row pointers
    and lengths into zeros: in bounds, a wrong result, never a wild address.

Integer, bool and index tensors are never poisoned (a NaN has no meaning there and a wild index
must not exist); anything that is not a tensor is handed through.

The spin D is no pass criterion; it only has to outlast the host's enqueue time of the gated
call.  `measure` takes the wall time of the same call on an ungated side stream with its closing
synchronise (an upper bound of the enqueue time) and `spin_ms` turns it into D = max(50 ms,
20 x that time) — the factor covers a descheduled host on a shared slot — capped at 500 ms: a
call whose 20 x exceeds the cap must be shrunk (fewer iterations), the cap is not raised.  The
spin is torch.cuda._sleep, calibrated once per process with two events; a torch without it spins
on a chain of matmuls of the same calibrated length."""
import contextlib
import time

import torch as tr

D_MIN_MS, D_FACTOR, D_CAP_MS = 50.0, 20.0, 500.0
# the junk ladder: bytes per tensor, several per size, up to a few MB
JUNK_SIZES = [512 << k for k in range(0, 14)]      # 512 B .. 4 MiB
JUNK_EACH = 4

_calibration = {}


def _spin_unit(gpu):
    """-> (enqueue(ms) on the current stream, what spins)."""
    key = str(gpu)
    if key in _calibration:
        return _calibration[key]
    a, b = tr.cuda.Event(enable_timing=True), tr.cuda.Event(enable_timing=True)
    sleep = getattr(tr.cuda, '_sleep', None)
    if sleep is not None:
        probe = 20_000_000
        sleep(1000)
        tr.cuda.synchronize(gpu)
        a.record()
        sleep(probe)
        b.record()
        tr.cuda.synchronize(gpu)
        per_ms = probe / max(a.elapsed_time(b), 1e-3)

        def enqueue(ms):
            sleep(int(per_ms * ms))
        what = f'torch.cuda._sleep, {per_ms:.4g} cycles per ms'
    else:
        m = tr.rand((2048, 2048), dtype=tr.float32, device=gpu)
        tr.matmul(m, m)
        tr.cuda.synchronize(gpu)
        a.record()
        for _ in range(16):
            tr.matmul(m, m)
        b.record()
        tr.cuda.synchronize(gpu)
        per_ms = 16 / max(a.elapsed_time(b), 1e-3)

        def enqueue(ms):
            for _ in range(max(int(per_ms * ms) + 1, 1)):
                tr.matmul(m, m)
        what = f'matmul chain, {per_ms:.4g} products per ms'
    _calibration[key] = (enqueue, what)
    return _calibration[key]


def spin_ms(enqueue_s):
    """D in milliseconds for a call whose enqueue time is at most `enqueue_s` seconds."""
    want = D_FACTOR * enqueue_s * 1e3
    assert want <= D_CAP_MS, (f'20 x the measured {enqueue_s * 1e3:.1f} ms exceeds the cap of '
                              f'{D_CAP_MS:.0f} ms: shrink the call, do not raise the cap')
    return max(D_MIN_MS, want)


def measure(gpu, call):
    """Wall seconds of `call()` on an ungated side stream, its closing synchronise included."""
    tr.cuda.synchronize(gpu)
    side = tr.cuda.Stream(device=gpu)
    t0 = time.perf_counter()
    with tr.cuda.stream(side):
        out = call()
        side.synchronize()
    dt = time.perf_counter() - t0
    tr.cuda.current_stream(gpu).wait_stream(side)
    tr.cuda.synchronize(gpu)
    del out
    return dt


def is_value(v):
    return isinstance(v, tr.Tensor) and v.is_floating_point()


class Gate:
    def __init__(self, gpu, side, event, inputs, truth, d_ms):
        self.gpu, self.side, self.gate = gpu, side, event
        self.inputs, self.truth, self.d_ms = inputs, truth, d_ms

    def closed(self):
        """True while the side stream has not passed the gate: the host has not waited."""
        return not self.gate.query()

    def unchanged(self, skip=()):
        """Names of value inputs that no longer hold their true bits (after the gate's exit)."""
        bad = []
        for k, v in self.truth.items():
            if k not in skip and not tr.equal(self.inputs[k].detach().view(tr.uint8).reshape(-1),
                                              v.view(tr.uint8).reshape(-1)):
                bad.append(k)
        return bad


@contextlib.contextmanager
def gated(gpu, inputs, enqueue_s=0.0, d_ms=None):
    """See the module docstring.  enqueue_s: `measure`'s time of the same call (-> D); d_ms
    overrides D."""
    d_ms = spin_ms(enqueue_s) if d_ms is None else d_ms
    spin, _ = _spin_unit(gpu)
    tr.cuda.synchronize(gpu)
    side = tr.cuda.Stream(device=gpu)
    handed, truth = {}, {}
    with tr.cuda.device(gpu):
        for k, v in inputs.items():
            if is_value(v):
                truth[k] = v.detach().to(gpu).clone().contiguous()
                handed[k] = tr.full_like(truth[k], float('nan'))
            else:
                handed[k] = v
        tr.cuda.synchronize(gpu)
        event = tr.cuda.Event()
        with tr.cuda.stream(side):
            spin(d_ms)
            event.record(side)
            for k, v in truth.items():
                handed[k].copy_(v, non_blocking=True)
        g = Gate(gpu, side, event, handed, truth, d_ms)
        try:
            with tr.cuda.stream(side):
                yield g
        finally:
            # the default stream has not waited for the side stream: what the call freed too
            # early is rewritten with zero bytes before the gated kernels start
            junk = [tr.zeros(size, dtype=tr.uint8, device=gpu)
                    for size in JUNK_SIZES for _ in range(JUNK_EACH)]
            tr.cuda.current_stream(gpu).wait_stream(side)
            tr.cuda.synchronize(gpu)
            del junk


@contextlib.contextmanager
def readbacks(g):
    """Wraps torch.Tensor.cpu for the duration: -> a list that gains g.closed() at every call."""
    seen, real = [], tr.Tensor.cpu

    def cpu(self, *a, **k):
        seen.append(g.closed())
        return real(self, *a, **k)
    tr.Tensor.cpu = cpu
    try:
        yield seen
    finally:
        tr.Tensor.cpu = real
