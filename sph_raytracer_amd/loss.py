"""Retrieval losses — thin counterparts of the reference's loss.py (loss.py:14-162).

A loss is built once, weighted by multiplying with a scalar (``5 * SquareLoss()``), and called
by ``gd()`` as ``loss(f, y, density, coeffs)``; the fidelity losses call the Operator ``f``.
"""
import math
import numbers

import torch as t


def _scaled(m, x):
    """m * x, skipping the multiply (one kernel, and one more in the backward) when m is the
    scalar 1: x * 1 == x exactly."""
    if isinstance(m, (int, float)) and not isinstance(m, bool) and m == 1:
        return x
    return m * x


class Loss:
    """Base loss: ``compute(f, y, d, c)`` times weight ``lam``.

    Args: projection_mask / volume_mask (multiplied into measurements / densities), lam (weight),
    use_grad (False -> evaluated under no_grad, e.g. for monitoring).
    """

    kind = 'regularizer'

    def __init__(self, *args, projection_mask=1, volume_mask=1, lam=1, use_grad=True, **kwargs):
        self.projection_mask = projection_mask
        self.volume_mask = volume_mask
        self.lam = lam
        self.use_grad = use_grad

    def compute(self, f, y, d, c):
        raise NotImplementedError

    def __call__(self, f, y, d, c):
        if self.use_grad:
            val = self.compute(f, y, d, c)
        else:
            with t.no_grad():
                val = self.compute(f, y, d, c)
        return None if val is None else _scaled(self.lam, val)

    def __mul__(self, other):
        self.lam = other
        return self

    __rmul__ = __mul__

    def __repr__(self):
        return f'{self.lam:.0e} * {type(self).__name__}'


class SquareLoss(Loss):
    """mean((y - f(d))^2) over unmasked pixels."""
    kind = 'fidelity'

    def compute(self, f, y, d, c):
        return t.mean(_scaled(self.projection_mask, (y - f(_scaled(self.volume_mask, d))) ** 2))


class SquareRelLoss(Loss):
    """mean(((y - f(d)) / y)^2), zero where y == 0."""
    kind = 'fidelity'

    def compute(self, f, y, d, c):
        pred = f(_scaled(self.volume_mask, d))
        nz = y != 0
        rel = t.zeros_like(y)
        rel[nz] = (y - pred)[nz] / y[nz]
        return t.mean(_scaled(self.projection_mask, rel) ** 2)


class AbsLoss(Loss):
    """mean(|y - f(d)|)."""
    kind = 'fidelity'

    def compute(self, f, y, d, c):
        return t.mean(_scaled(self.projection_mask, (y - f(_scaled(self.volume_mask, d))).abs()))


class HuberLoss(Loss):
    """mean(huber(f(d) - y)): 0.5 r^2 where |r| < delta, delta (|r| - 0.5 delta) beyond —
    quadratic near the solution (where AbsLoss's constant-magnitude gradient makes Adam
    oscillate), linear in the outliers.  Not in the reference.  A float32 y against a float64
    forward is promoted, as torch's arithmetic promotes it."""
    kind = 'fidelity'

    def __init__(self, delta=1.0, **kwargs):
        # (a real number — int, float, a numpy scalar; no bool, no tensor — finite and > 0)
        if isinstance(delta, bool) or not isinstance(delta, numbers.Real) or not delta > 0 \
                or delta == float('inf'):
            raise ValueError(f'HuberLoss needs a finite delta > 0, not {delta!r}')
        self.delta = float(delta)
        super().__init__(**kwargs)

    def compute(self, f, y, d, c):
        pred = f(_scaled(self.volume_mask, d))
        if y.dtype != pred.dtype:     # (huber_loss itself refuses mixed dtypes)
            dt = t.promote_types(y.dtype, pred.dtype)
            y, pred = y.to(dt), pred.to(dt)
        return t.mean(_scaled(self.projection_mask, t.nn.functional.huber_loss(
            pred, y, reduction='none', delta=self.delta)))


class PoissonLoss(Loss):
    """mean(p - y log(p + eps)), p = f(d): the Poisson negative log-likelihood of photon counts y
    (up to the term in y alone), the fidelity for low counts — torch's ``poisson_nll_loss(p, y,
    log_input=False, full=False, eps=eps)`` under the mask and the mean.  Not in the reference.
    No guards: where p + eps <= 0 the log and the quotient give what torch gives (NaN, +-inf),
    and they propagate.  A float32 y against a float64 forward is promoted, as HuberLoss does."""
    kind = 'fidelity'

    def __init__(self, eps=1e-8, **kwargs):
        # (a real number — int, float, a numpy scalar; no bool, no tensor — finite and > 0)
        if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or not eps > 0 \
                or eps == float('inf'):
            raise ValueError(f'PoissonLoss needs a finite eps > 0, not {eps!r}')
        self.eps = float(eps)
        super().__init__(**kwargs)

    def compute(self, f, y, d, c):
        pred = f(_scaled(self.volume_mask, d))
        if y.dtype != pred.dtype:
            dt = t.promote_types(y.dtype, pred.dtype)
            y, pred = y.to(dt), pred.to(dt)
        return t.mean(_scaled(self.projection_mask, t.nn.functional.poisson_nll_loss(
            pred, y, log_input=False, full=False, eps=self.eps, reduction='none')))


class CheaterLoss(Loss):
    """L2 distance to a known ground-truth density (monitoring only)."""
    kind = 'oracle'

    def __init__(self, density_truth, *args, **kwargs):
        self.density_truth = density_truth
        super().__init__(**kwargs)

    def compute(self, f, y, d, c):
        return t.mean(_scaled(self.volume_mask, (d - self.density_truth) ** 2))


class NegRegularizer(Loss):
    """Mean magnitude of negative voxels."""

    def compute(self, f, y, d, c):
        return t.mean(t.abs(_scaled(self.volume_mask, d.clip(max=0))))


SMOOTH_KINDS = {'square': 0, 'abs': 1, 'huber': 2}   # 0, SPHRT_RESID_ABS, SPHRT_RESID_HUBER


def _real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


class SmoothRegularizer(Loss):
    """Roughness of the density: a difference penalty over its trailing axes (r, e, a) and,
    with ``time_weight``, the axis before them (a dynamic grid's time axis, or a channel axis);
    any further leading axes are batch.  Not in the reference.

        P(d) = (1/N) * sum_ax w_ax * sum_{edges i -> i+1 along ax} rho(d[i+1] - d[i])

    with N = d.numel() and rho by ``kind``: ``'square'`` (r^2), ``'abs'`` (|r|: anisotropic total
    variation) or ``'huber'`` (torch's huber_loss with ``delta``).  ``weights`` are (w_r, w_e,
    w_a).  With ``wrap_a`` the azimuth ring closes — one more edge from the last azimuth bin to the
    first, ``roll(d, -1, -1) - d``; None: it closes when the grid of the operator `f` spans 2 pi
    in azimuth (to 1e-9 relative; no grid: open).  An axis of length 1 or of weight 0 contributes
    nothing.

    A contiguous float64 density on a GPU is evaluated by one HIP launch (csrc/loss.hip,
    sphrt_smooth_reg_f64: value and gradient in one pass); anything else — CPU tensors, float32,
    non-contiguous tensors, a differentiable backward — by the same formula in plain torch
    (`formula`)."""

    def __init__(self, weights=(1, 1, 1), time_weight=0, kind='square', delta=None, wrap_a=None,
                 **kwargs):
        try:
            weights = tuple(weights)
        except TypeError:
            weights = ()
        if len(weights) != 3 or not all(self._weight(w) for w in weights):
            raise ValueError('SmoothRegularizer needs three weights (w_r, w_e, w_a), real numbers '
                             f'that are finite and >= 0, not {weights!r}')
        if not self._weight(time_weight):
            raise ValueError('SmoothRegularizer needs a time_weight that is a real number, finite '
                             f'and >= 0, not {time_weight!r}')
        if not isinstance(kind, str) or kind not in SMOOTH_KINDS:
            raise ValueError(f"kind must be 'square', 'abs' or 'huber', not {kind!r}")
        if kind == 'huber':
            if not (_real(delta) and delta > 0 and delta != float('inf')):
                raise ValueError(f"kind='huber' needs a finite delta > 0, not {delta!r}")
        elif delta is not None:
            raise ValueError(f"delta belongs to kind='huber', not kind={kind!r}")
        if wrap_a is not None and not isinstance(wrap_a, bool):
            raise ValueError(f'wrap_a must be True, False or None, not {wrap_a!r}')
        self.weights = tuple(float(w) for w in weights)
        self.time_weight = float(time_weight)
        self.smooth_kind = kind
        self.delta = float(delta) if kind == 'huber' else None
        self.wrap_a = wrap_a
        super().__init__(**kwargs)

    @staticmethod
    def _weight(w):
        return _real(w) and 0 <= w < float('inf')

    def wraps(self, f):
        """Does the azimuth ring close: ``wrap_a``, or inferred from the grid of `f`."""
        if self.wrap_a is not None:
            return self.wrap_a
        grid = getattr(f, 'grid', None)
        a_b = getattr(grid, 'a_b', None)
        if a_b is None or len(a_b) < 2:
            return False
        span = abs(float(a_b[-1]) - float(a_b[0]))
        return abs(span - 2 * math.pi) <= 1e-9 * (2 * math.pi)

    def _rho(self, hi, lo):
        if self.smooth_kind == 'square':
            return (hi - lo) ** 2
        if self.smooth_kind == 'abs':
            return (hi - lo).abs()
        return t.nn.functional.huber_loss(hi, lo, reduction='none', delta=self.delta)

    def _axes(self, d):
        """[(dim, weight)] of the axes that have edges, in the order t, r, e, a."""
        if d.dim() < 3:
            raise ValueError(f'SmoothRegularizer needs a density with axes (..., r, e, a), not '
                             f'shape {tuple(d.shape)}')
        axes = [(-4, self.time_weight)] if d.dim() >= 4 else []
        axes += [(-3, self.weights[0]), (-2, self.weights[1]), (-1, self.weights[2])]
        return [(dim, w) for dim, w in axes if w > 0 and d.shape[dim] > 1]

    def formula(self, d, wrap):
        """The penalty in plain torch (differentiable): narrow, roll, abs, huber_loss."""
        total = d.new_zeros(())
        for dim, w in self._axes(d):
            n = d.shape[dim]
            if dim == -1 and wrap:
                hi, lo = t.roll(d, -1, -1), d
            else:
                hi, lo = d.narrow(dim, 1, n - 1), d.narrow(dim, 0, n - 1)
            total = total + w * self._rho(hi, lo).sum()
        return total / d.numel()

    def _launch(self, d, wrap, lam, c_neg, g_in, g_out, part_smooth, part_neg):
        """sphrt_smooth_reg_f64 over the contiguous float64 GPU density `d`."""
        from . import _lib
        lib = _lib.load()
        timed = d.dim() >= 4 and self.time_weight > 0
        nt = d.shape[-4] if timed else 1
        nr, ne, na = d.shape[-3:]
        _lib.check(lib.sphrt_smooth_reg_f64(
            _lib.ptr(d), d.numel() // (nt * nr * ne * na), nt, nr, ne, na, self.time_weight,
            *self.weights, SMOOTH_KINDS[self.smooth_kind], self.delta or 0.0, int(wrap),
            1.0 / d.numel(), lam, c_neg, _lib.ptr(g_in), _lib.ptr(g_out), _lib.ptr(part_smooth),
            _lib.ptr(part_neg), _lib.stream_of(d.device)), 'sphrt_smooth_reg_f64')

    def compute(self, f, y, d, c):
        d = _scaled(self.volume_mask, d)
        wrap = self.wraps(f)
        if isinstance(d, t.Tensor) and d.is_cuda and d.dtype == t.float64 and d.is_contiguous() \
                and d.dim() >= 3 and d.numel() > 0:
            return _SmoothFunction.apply(d, self, wrap)
        return self.formula(d, wrap)


class _SmoothFunction(t.autograd.Function):
    """SmoothRegularizer on a contiguous float64 GPU density: the forward is one launch that
    leaves the penalty's partial sums and its gradient G (lam = 1), the backward G * grad_out.
    A backward that is itself differentiated (create_graph) comes from the torch formula."""

    @staticmethod
    def forward(ctx, d, reg, wrap):
        from . import _lib
        src = d.detach()
        n_part = _lib.load().sphrt_loss_partials(src.numel())
        part = t.empty(n_part, dtype=t.float64, device=src.device)
        grad = t.empty_like(src)
        with t.cuda.device(src.device):
            reg._launch(src, wrap, 1.0, 0.0, None, grad, part, None)
        ctx.reg, ctx.wrap, ctx.grad = reg, wrap, grad
        ctx.save_for_backward(d)
        return part.sum() / src.numel()

    @staticmethod
    def backward(ctx, grad_out):
        if t.is_grad_enabled():
            d, = ctx.saved_tensors
            with t.enable_grad():
                src = d if d.requires_grad else d.detach().requires_grad_()
                g, = t.autograd.grad(ctx.reg.formula(src, ctx.wrap), src, grad_out,
                                     create_graph=True)
            return g, None, None
        return ctx.grad * grad_out, None, None


class IsoTVRegularizer(Loss):
    """Isotropic total variation of the density over its trailing axes (r, e, a); every leading
    axis is batch.  Not in the reference.

        P(d) = (1/N) * sum_i sqrt( sum_ax (w_ax * (D_ax d)[i])^2 )

    with N = d.numel() and D_ax the forward difference of include/sphrt_pd.h: an edge belongs to
    its lower voxel, (D_ax d)[i] = d[upper neighbour of i] - d[i]; with the azimuth ring closed
    (``wrap_a``, read as SmoothRegularizer reads it) the wrap edge belongs to the ring's last
    voxel; an axis of weight 0 or of length 1 has no edges, and a missing edge contributes 0 to
    its voxel's sum.  With one axis carrying edges P is SmoothRegularizer(kind='abs') of the same
    weights.

    `compute` is plain torch on every device and differentiable; where all of a voxel's
    differences vanish the gradient is 0 (the square root is masked before and after), not NaN.
    `gd` runs the class through autograd; `primal_dual` and `chambolle_pock` take it as their TV
    term and never differentiate it (include/sphrt_iso.h)."""

    def __init__(self, weights=(1, 1, 1), wrap_a=None, **kwargs):
        try:
            weights = tuple(weights)
        except TypeError:
            weights = ()
        if len(weights) != 3 or not all(SmoothRegularizer._weight(w) for w in weights):
            raise ValueError('IsoTVRegularizer needs three weights (w_r, w_e, w_a), real numbers '
                             f'that are finite and >= 0, not {weights!r}')
        if wrap_a is not None and not isinstance(wrap_a, bool):
            raise ValueError(f'wrap_a must be True, False or None, not {wrap_a!r}')
        self.weights = tuple(float(w) for w in weights)
        self.wrap_a = wrap_a
        super().__init__(**kwargs)

    wraps = SmoothRegularizer.wraps

    def formula(self, d, wrap):
        """The penalty in plain torch (differentiable): narrow, roll, a masked sqrt."""
        if d.dim() < 3:
            raise ValueError(f'IsoTVRegularizer needs a density with axes (..., r, e, a), not '
                             f'shape {tuple(d.shape)}')
        n2 = t.zeros_like(d)
        for dim, w in zip((-3, -2, -1), self.weights):
            n = d.shape[dim]
            if not (w > 0 and n > 1):
                continue
            if dim == -1 and wrap:
                n2 = n2 + (w * (t.roll(d, -1, -1) - d)) ** 2
            else:
                e = w * (d.narrow(dim, 1, n - 1) - d.narrow(dim, 0, n - 1))
                pad = [0, 0] * (-dim - 1) + [0, 1]       # (one zero after the axis' last voxel)
                n2 = n2 + t.nn.functional.pad(e ** 2, pad)
        live = n2 != 0                   # (a NaN stays live)
        root = t.sqrt(t.where(live, n2, t.ones_like(n2)))
        return t.where(live, root, t.zeros_like(root)).sum() / d.numel()

    def compute(self, f, y, d, c):
        return self.formula(_scaled(self.volume_mask, d), self.wraps(f))


class NegSumRegularizer(Loss):
    """Summed magnitude of negative voxels."""

    def compute(self, f, y, d, c):
        return t.sum(t.abs(_scaled(self.volume_mask, d.clip(max=0))))
