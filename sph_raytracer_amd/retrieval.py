"""Gradient-descent retrieval — thin counterpart of the reference's retrieval.py (:24-127).

Every iteration is one Operator forward per fidelity loss plus one backward, i.e. the forward
and adjoint HIP kernels on the cached trace; the optimiser step is plain PyTorch.  The
examples/static_retrieval.py loop (FullyDenseModel, SquareLoss + NegRegularizer) runs the same
arithmetic without autograd (_gd_direct): the same iterates, a quarter of the launches.

`cg` (not in the reference) solves the totals that are quadratic — a SquareLoss, a square
SmoothRegularizer, a damping term — as a linear system by conjugate gradients: the same operator
launches per iteration, three csrc/loss.hip launches for the vector side, no learning rate.
"""
import ctypes
import math
import types

import torch as t

from .loss import (AbsLoss, HuberLoss, IsoTVRegularizer, NegRegularizer, PoissonLoss,
                   SmoothRegularizer, SquareLoss)
from .model import FullyDenseModel

try:
    from tqdm import tqdm
except ImportError:    # progress bars are cosmetic
    def tqdm(it, disable=False):
        return it


def detach_loss(loss):
    """Loss value as a float, detached from autograd."""
    return float(loss.detach().cpu()) if isinstance(loss, t.Tensor) else loss


class _Bar:
    def __init__(self, it, enabled):
        self.it = tqdm(it, disable=not enabled)
        self.enabled = enabled

    def __iter__(self):
        return iter(self.it)

    def describe(self, text):
        if self.enabled and hasattr(self.it, 'set_description'):
            self.it.set_description(text)


def gd(f, y, model, coeffs=None, num_iterations=100, loss_fns=[SquareLoss()], optim=t.optim.Adam,
       optim_vars=None, progress_bar=True, device=None, **kwargs):
    """Minimise the weighted sum of ``loss_fns`` over the model coefficients.

    Same contract as the reference: returns (coeffs, f(model(coeffs)), {loss_fn: [values]});
    Ctrl-C stops early.  Like the reference, the coefficients returned are those of the last
    iteration (its best-loss bookkeeping never updates, retrieval.py:112-113).
    """
    if hasattr(f, 'grid') and f.grid != model.grid:
        raise ValueError("f and model must have same grid")
    if y is not None:
        y.requires_grad_()
    if coeffs is None:
        coeffs = t.ones(model.coeffs_shape, requires_grad=True, device=device or f.device,
                        dtype=t.float64)
    if optim_vars is None:
        optim_vars = [coeffs]
    for v in optim_vars:
        v.requires_grad_()
    best_loss, best_coeffs = float('inf'), None
    # the optimiser exactly as the reference builds it (retrieval.py:84): torch's own default
    # implementation choice (foreach on GPU tensors) unless the caller passes foreach=/fused=
    opt = optim(optim_vars, **kwargs)
    plan = _direct_plan(f, y, model, coeffs, loss_fns, optim_vars)
    if plan is None:
        plan = _fused_plan(f, y, model, coeffs, loss_fns, optim_vars)
    if plan is not None:
        return _gd_direct(f, y, coeffs, loss_fns, opt, plan, num_iterations, progress_bar)
    losses = {fn: [] for fn in loss_fns}
    o_stat = 0
    bar = _Bar(range(num_iterations), progress_bar)
    # Without a progress bar nothing needs the loss values during the loop: they stay on the
    # device and are read back once at the end (no host sync per iteration; same values, same
    # return contract).  With a bar, every iteration reads them back as the reference does.
    deferred = not progress_bar
    pending = {fn: [] for fn in loss_fns}
    improved = None                       # device flag: some iteration had total < best_loss
    try:
        for _ in bar:
            opt.zero_grad()
            density = model(coeffs)
            total = f_stat = r_stat = 0
            for fn in loss_fns:
                val = fn(f, y, density, coeffs)
                if fn.use_grad and fn.kind != 'oracle':
                    total += val
                if deferred:
                    pending[fn].append(val.detach() if isinstance(val, t.Tensor) else val)
                    continue
                if fn.kind == 'oracle' and not math.isnan(val):
                    o_stat = val
                elif fn.kind == 'fidelity':
                    f_stat += val
                elif fn.kind == 'regularizer':
                    r_stat += val
                losses[fn].append(detach_loss(val))
            if deferred:
                ok = total < best_loss
                improved = ok if improved is None else improved | ok
            else:
                bar.describe(f'F:{f_stat:.1e} R:{r_stat:.1e} O:{o_stat * 100:.0f}')
                if total < best_loss:
                    best_coeffs = coeffs
            total.backward(retain_graph=True)
            opt.step()
            if hasattr(model, 'proj'):
                coeffs.data = model.proj(coeffs)
    except KeyboardInterrupt:
        pass
    if deferred:
        for fn, vals in pending.items():
            tens = [v for v in vals if isinstance(v, t.Tensor)]
            host = iter(t.stack(tens).cpu().tolist()) if tens else iter(())
            losses[fn] = [next(host) if isinstance(v, t.Tensor) else v for v in vals]
        if improved is not None and bool(improved):
            best_coeffs = coeffs    # the same tensor object every iteration (updated in place)
    return best_coeffs, f(model(best_coeffs)), losses



def _unit(m):
    return isinstance(m, (int, float)) and not isinstance(m, bool) and m == 1


def _direct_plan(f, y, model, coeffs, loss_fns, optim_vars):
    """The loss terms of a loop `_gd_direct` runs without autograd, or None.  It covers the
    examples/static_retrieval.py loop: a FullyDenseModel (the coefficients are the density) on a
    static Operator, one fidelity term — a SquareLoss, an AbsLoss, a HuberLoss or a PoissonLoss,
    exactly those types — at most one NegRegularizer and at most one SmoothRegularizer, scalar weights, no
    masks but the fidelity term's projection_mask (`_ray_mask`: per-ray weights, a mask of bad
    pixels), the coefficients the only optimised variable.  With all three terms the fidelity
    term must come first in `loss_fns`: autograd accumulates the terms [t1, t2, t3] of the total
    at the shared leaf as (g3 + g2) + g1, and the smooth kernel forms g_fid + (g_smooth + g_neg);
    with the fidelity term second or third the sum would round otherwise, so that list is
    declined (two terms commute: any order).  Anything else takes the autograd loop."""
    from .raytracer import Operator
    if not isinstance(f, Operator) or f.dynamic or f._csr is None or y is None:
        return None
    return _loop_terms(f, y, model, coeffs, loss_fns, optim_vars)


def _fused_plan(f, y, model, coeffs, loss_fns, optim_vars):
    """`_direct_plan` for a MatrixFreeOperator on a static grid: the same loop and the same
    conditions, with the forward and the adjoint of an iteration in one trace
    (MatrixFreeOperator.residual_gradient's kernel; the operator's `deterministic` attribute
    picks the float64-atomic or the fixed-point scatter, and with the latter two runs of gd give
    the same bits).  Anything else takes the autograd loop."""
    from .raytracer import MatrixFreeOperator
    if not isinstance(f, MatrixFreeOperator) or f.dynamic or f.grid.dynamic or y is None:
        return None
    return _loop_terms(f, y, model, coeffs, loss_fns, optim_vars)


def _ray_mask(mask, y):
    """Is `mask` a fidelity term's projection_mask `_gd_direct` weighs the residual with: a constant
    tensor on y's device, bool, float32 or float64, broadcastable to y's shape."""
    if not (isinstance(mask, t.Tensor) and mask.device == y.device and not mask.requires_grad
            and mask.dtype in (t.bool, t.float32, t.float64)):
        return False
    try:
        return tuple(t.broadcast_shapes(mask.shape, y.shape)) == tuple(y.shape)
    except RuntimeError:
        return False


# the direct loops' fidelity terms, by exact type
_FIDELITY = (SquareLoss, AbsLoss, HuberLoss, PoissonLoss)


def _robust_of(fid):
    """(kind, delta) of a robust fidelity term as the C entries take them, None for SquareLoss."""
    from .raytracer import ROBUST_KINDS
    if type(fid) is AbsLoss:
        return ROBUST_KINDS['abs'], 0.0
    if type(fid) is HuberLoss:
        return ROBUST_KINDS['huber'], float(fid.delta)
    return None


def _poisson_of(fid):
    """The eps of a PoissonLoss as the C entries take it, None for any other fidelity term."""
    return float(fid.eps) if type(fid) is PoissonLoss else None


def _loop_terms(f, y, model, coeffs, loss_fns, optim_vars):
    """(fidelity term, NegRegularizer or None) when model, variables, measurements and loss terms
    are those `_gd_direct` runs over the operator `f`, else None; with a SmoothRegularizer among
    the terms, the 3-tuple (fidelity, NegRegularizer or None, SmoothRegularizer).  The fidelity
    term is exactly one SquareLoss, AbsLoss, HuberLoss or PoissonLoss (`_FIDELITY`; a subclass may compute
    anything: the autograd loop); with both regularisers it is the first term (`_direct_plan`)."""
    if type(model) is not FullyDenseModel or hasattr(model, 'proj'):
        return None
    if len(optim_vars) != 1 or optim_vars[0] is not coeffs or coeffs.dtype != t.float64:
        return None     # (float64, the reference's coefficients: every scalar below is exact)
    if not (isinstance(y, t.Tensor) and coeffs.is_cuda and coeffs.device == f._cdev
            and y.device == coeffs.device and y.dtype in (t.float32, t.float64)
            and coeffs.is_contiguous() and tuple(coeffs.shape) == tuple(f.grid.shape)
            and tuple(y.shape) == tuple(f._ray_shape)):
        # (other devices, or a y the reference's SquareLoss would broadcast: the autograd loop)
        return None
    sq = neg = smooth = None
    for fn in loss_fns:
        if not (fn.use_grad and isinstance(fn.lam, (int, float)) and not isinstance(fn.lam, bool)
                and _unit(fn.volume_mask)):
            return None
        if not (_unit(fn.projection_mask)
                or type(fn) in _FIDELITY and _ray_mask(fn.projection_mask, y)):
            return None
        if type(fn) in _FIDELITY and sq is None:
            sq = fn
        elif type(fn) is NegRegularizer and neg is None:
            neg = fn
        elif type(fn) is SmoothRegularizer and smooth is None:
            smooth = fn
        else:
            return None
    if sq is None:
        return None
    if smooth is None:
        return sq, neg
    if neg is not None and loss_fns[0] is not sq:
        return None     # ((g3 + g2) + g1: only a leading fidelity term gives g_fid + (the rest))
    return sq, neg, smooth


def _stored_loop_setup(f, yd, w_res, s_res, stage=True):
    """What a direct loop over a stored Operator arranges once: the loop's forward descriptor (or
    None: f(d) itself), the adjoint's input order, the measurements and the per-ray factors
    (None: unweighted) in the order the loop's forward writes — trace positions when the
    descriptor's rows can be pointed at them, else geometry rays, and then `res_order` gathers
    the adjoint's input (the same values in the same order either way: bitwise the same
    iterates).  `stage`: take the brick-staged descriptor where there is one (its forward packs d
    itself unless the caller keeps the stage current: `_gd_direct`'s Adam launch); without it
    only the plain copy of the trace's descriptor, which a reordered trace needs.
    -> (loop_desc, order, res_order, y_res, w_res, s_res, keep): keep = (the staged pair, the
    trace-position lists), either None when not in use, for the caller to hold."""
    f64, n_meas = t.float64, yd.numel()
    staged = f._stage_for_loop(f64) if stage else None
    if staged is not None and f._csr['n'] != n_meas:
        staged = None
    order = f._adjoint_trace_order()
    if order is not None and order.numel() != n_meas:
        order = None
    loop_desc = staged[0] if staged is not None else None
    y_res, res_order, keep_rows = yd.reshape(-1), order, None
    if order is not None:
        sd = loop_desc if loop_desc is not None else f._loop_descriptor(f64)
        keep_rows = f._trace_position_rows(sd) if sd is not None else None
        if keep_rows is not None:
            loop_desc = sd
            y_res, res_order = y_res.index_select(0, f._ray_id_long()), None
            if w_res is not None:
                w_res, s_res = (v.index_select(0, f._ray_id_long())
                                for v in (w_res, s_res))
    return loop_desc, order, res_order, y_res, w_res, s_res, (staged, keep_rows)


def _fidelity_stage(f, y, fid, gradient=True, n_total=None, stage=True, zero_m=False):
    """The fidelity side of a direct loop over `f`, arranged once per solve; `_gd_direct`,
    `_normal_direct` and `_chambolle_pock_direct` all read it.

        yd, n_meas, y_f64   the measurements as measured (detached, contiguous; a float32 y is
                            promoted inside the kernels, exactly), their count, the float64 flag
        n_norm, c           the mean's N (`n_total`: the whole stack's, distributed.gd) and lam / N
        robust, poisson     `_robust_of`, `_poisson_of` of the term
        w_res, s_res        the loss's weights w and the per-ray factors s, flat float64, in the
                            order y_res is in.  `gradient`: s is the factor of the gradient's
                            residual — for the square term (c * w) * 2, and None (as w) for a unit
                            mask, where the scalar `scale` = 2 c serves; for a robust or Poisson
                            term c * w, always arrays (a unit mask: ones, and a fill of c).
                            Without it (chambolle_pock's ray dual): c * w for every term, always
                            arrays.
        loop_desc, order, res_order, y_res, staged, positions
                            over a stored Operator, `_stored_loop_setup` (`stage` is its flag);
                            positions: the loop's forward writes trace positions
        m64, weighted, fixed   over a MatrixFreeOperator: float64 measurements and the masked
                            square term's (s, max|s| or None) for the fused trace (`gradient`
                            only), the deterministic operator's (`_fixed_buffers`,) or ()
        residual(yhat, r_scaled, part, stream, against_y=True)
                            the term's csrc/loss.hip launch, bound once (`gradient` only): the
                            adjoint's input of the forward `yhat` into r_scaled — through
                            res_order where the adjoint takes trace order: no permutation launch —
                            and the loss's partial sums into part; against_y=False: against
                            `zero_m`, float64 zeros held when the caller asks for them"""
    from . import _lib
    from .raytracer import MatrixFreeOperator, _scale_max
    lib = _lib.load()
    dev, f64 = f._cdev, t.float64
    st = types.SimpleNamespace(fused=isinstance(f, MatrixFreeOperator))
    st.yd = yd = y.detach().contiguous()
    st.n_meas = n_meas = yd.numel()
    st.y_f64 = int(yd.dtype == f64)
    st.n_norm = n_meas if n_total is None else n_total
    st.c = c = fid.lam / st.n_norm
    st.scale = 2 * c
    st.robust, st.poisson = _robust_of(fid), _poisson_of(fid)
    square = gradient and st.robust is None and st.poisson is None
    w = s = None
    if isinstance(fid.projection_mask, t.Tensor):
        w = fid.projection_mask.detach().to(f64).expand(yd.shape).contiguous().reshape(-1)
        s = (c * w) * 2 if square else c * w
    elif not square:
        w = t.ones(n_meas, dtype=f64, device=dev)
        s = t.full((n_meas,), c, dtype=f64, device=dev)
    st.loop_desc = st.order = st.res_order = st.staged = None
    st.y_res, st.positions = yd.reshape(-1), False
    st.m64 = st.weighted = None
    st.fixed = ()
    st.zero_m = t.zeros(n_meas, dtype=f64, device=dev) if zero_m else None
    if not st.fused:
        st.loop_desc, st.order, st.res_order, st.y_res, w, s, keep = _stored_loop_setup(
            f, yd, w, s, stage=stage)
        st.staged, st.positions, st._keep = keep[0], keep[1] is not None, keep
    elif gradient:
        # the fused trace subtracts float64 measurements; a deterministic operator's fixed-point
        # bound on the masked square term: max|s|, read back once for the loop
        st.m64 = yd.to(f64).reshape(-1)
        if square and s is not None:
            st.weighted = (s, _scale_max(s) if f.deterministic else None)
    if st.fused and f.deterministic:
        # (the integer accumulator and scale record, once for the whole loop)
        st.fixed = (f._fixed_buffers(),)
    st.w_res, st.s_res = w, s
    if not gradient:
        return st
    if st.poisson is not None:
        name, par = 'sphrt_poisson_residual_f64', (st.poisson,)
    elif st.robust is not None:
        name, par = 'sphrt_robust_residual_f64', st.robust
    else:
        name, par = 'sphrt_sq_residual_f64' if s is None else 'sphrt_wsq_residual_f64', ()
    entry = getattr(lib, name)
    factors = (*par, _lib.ptr(s), _lib.ptr(w)) if s is not None else (st.scale,)
    against = {True: (_lib.ptr(st.y_res), st.y_f64), False: (_lib.ptr(st.zero_m), 1)}
    order = _lib.ptr(st.res_order)

    def residual(yhat, r_scaled, part, stream, against_y=True):
        _lib.check(entry(_lib.ptr(yhat), *against[against_y], n_meas, *factors, order,
                         _lib.ptr(r_scaled), _lib.ptr(part), stream), name)
    st.residual = residual
    return st


def _gd_direct(f, y, coeffs, loss_fns, opt, plan, num_iterations, progress_bar, reduce=None,
               n_total=None):
    """`gd` for `_direct_plan` loops: the same arithmetic as autograd's, op by op, so the
    iterates are the same (the Operator forward, the adjoint of the SquareLoss residual, the
    NegRegularizer's -lam/N on negative voxels, the optimiser step), without building and walking
    a graph every iteration: one forward, one adjoint, the residual kernel of csrc/loss.hip
    (over a MatrixFreeOperator, `_fused_plan`: one trace that integrates, forms the scaled
    residual and scatters it — sphrt_trace_normal_f64 — and the residual kernel for the loss's
    partial sums only, on the forward that trace wrote) and the optimiser step (for Adam, one
    csrc/loss.hip launch that also applies the regulariser and keeps the forward's brick-staged
    density current; otherwise the regulariser's own kernel, then opt.step()).  The loss values are the fused kernels' partial
    sums, summed for all iterations after the loop: deterministic, within rounding of the
    autograd loop's torch.mean.

    Gradient of lam * mean((y - f(d))^2): autograd's chain gives (lam / N) * (2 * (y - f(d)))
    negated, i.e. (f(d) - y) * (2 * (lam / N)) exactly (scaling by 2 and negation are exact).
    With a projection_mask w (`_ray_mask`), lam * mean(w * (y - f(d))^2): autograd's mul backward
    weighs the mean's lam / N first, (lam / N) * w_i (one rounding), and the pow backward
    multiplies by 2 * (y - f(d)) (exact), so the adjoint's input is (f(d) - y) * s with
    s = ((lam / N) * w) * 2, formed once before the loop; the loss sums w * (r * r)
    (sphrt_wsq_residual_f64; fused: sphrt_trace_normal_weighted_f64 with ray_scale = s).
    AbsLoss, lam * mean(w * |y - f(d)|), and HuberLoss, lam * mean(w * huber(f(d), y)): the mean
    and the mask give s = (lam / N) * w_i as above (one rounding, none for a unit mask); abs's
    backward multiplies by sign(y - f(d)) and the subtraction negates — s * sign(f(d) - y), exact —
    and huber_loss's backward gives -(s * delta), s * delta or (f(d) - y) * s by the residual's
    side of +-delta, which is s * clamp(f(d) - y, -delta, delta) (one rounding either way).  So
    the adjoint's input is s * psi(f(d) - y) (sphrt_robust_residual_f64, which also sums
    w * |r| or w * huber(r); fused: sphrt_trace_normal_robust_f64 with ray_scale = s).  A NaN
    residual has a zero gradient under AbsLoss and a NaN one under HuberLoss, as in torch.
    PoissonLoss, lam * mean(w * (p - y * log(p + eps))) with p = f(d): s = (lam / N) * w_i as
    above, and the composite's sub, mul and log backward leave s + ((-s) * y) / (p + eps) at p —
    not a function of the residual (sphrt_poisson_residual_f64, which also sums
    w * (p - y * log(p + eps)); fused: sphrt_trace_normal_poisson_f64 with ray_scale = s).  That
    weight has no bound before the forward has run, so a deterministic MatrixFreeOperator runs
    two traces per iteration — the forward, the residual kernel, then op.T's own fixed-point
    back-projection — where the other terms run one; the iterates are then bitwise the autograd
    loop's over the same operator.
    Gradient of lam * mean(|clip(d, max=0)|): -(lam / N) where d < 0, else 0 (sign(0) = 0).
    The two are summed (IEEE addition commutes, so the order autograd accumulates them in does
    not matter) and handed to the optimiser as coeffs.grad.
    With a SmoothRegularizer (a 3-tuple plan): its Function's backward is G * lam with
    G = (S * (1 / N)) * 1, i.e. (S * inv_n) * lam, and autograd sums three terms as
    (g_smooth + g_neg) + g_fid (`_direct_plan`).  One sphrt_smooth_reg_f64 launch after the
    adjoint forms g = g + (G + neg) in place — the NegRegularizer's term as above, folded in —
    and leaves both regularisers' partial sums; the Adam launch then runs without a regulariser
    (c_neg = 0), and for another optimiser the launch stands in for sphrt_neg_reg_f64.

    Data-parallel use (distributed.gd): `f` is this rank's operator over its share of the views,
    `y` its share of the measurements, `n_total` the size of the whole stack (the SquareLoss
    mean's N) and `reduce` an in-place sum over the ranks, applied to the adjoint's gradient
    before the regulariser and the optimiser step (which are then identical on every rank) and
    to the SquareLoss sums after the loop."""
    from . import _lib
    sq, neg = plan[:2]
    smooth = plan[2] if len(plan) > 2 else None
    losses = {fn: [] for fn in loss_fns}
    y.requires_grad_()                 # (the reference's own side effect on y)
    step = _split_adam(opt, coeffs)
    # the fidelity side; over a stored Operator the brick-staged forward only with the Adam
    # launch, which keeps the stage current (no pack launch per iteration)
    fs = _fidelity_stage(f, y, sq, n_total=n_total, stage=step is not None)
    fused, yd, n_norm, staged, loop_desc = fs.fused, fs.yd, fs.n_norm, fs.staged, fs.loop_desc
    m64, s_res, fixed, robust, poisson = fs.m64, fs.s_res, fs.fixed, fs.robust, fs.poisson
    # (a deterministic Poisson loop: two traces, the stored loop's order of launches)
    two_trace = poisson is not None and fused and bool(f.deterministic)
    c_neg = neg.lam / coeffs.numel() if neg is not None else 0.0
    bar = _Bar(range(num_iterations), progress_bar)
    lib = _lib.load()
    n_meas, n_vox = fs.n_meas, coeffs.numel()
    yhat_buf = t.empty(n_meas, dtype=coeffs.dtype, device=coeffs.device) \
        if loop_desc is not None or fused else None
    # every iteration's loss as the workgroup partial sums of its fused kernel, one row per
    # iteration, summed once after the loop (no reduction launch, no host sync per iteration)
    ps, pn = lib.sphrt_loss_partials(n_meas), lib.sphrt_loss_partials(n_vox)
    rows = max(num_iterations, 1)
    part_sq = t.empty((rows, ps), dtype=t.float64, device=coeffs.device)
    part_neg = t.empty((rows, pn), dtype=t.float64, device=coeffs.device) if neg is not None else None
    part_smooth = smooth_wrap = None
    if smooth is not None:
        part_smooth = t.empty((rows, pn), dtype=t.float64, device=coeffs.device)
        smooth_wrap = smooth.wraps(f)
    done = 0

    def scaled(sums, n, lam):
        val = sums / n
        return val if _unit(lam) else lam * val

    try:
        # every launch below on the coefficients' GPU, whatever device is current (the C entry
        # points launch on the stream's device; torch's default stream handle is the current
        # device's)
        with t.no_grad(), t.cuda.device(coeffs.device):
            for it in bar:
                opt.zero_grad()
                d = coeffs.detach()
                stream = _lib.stream_of(d.device)
                if fused:
                    # f(d) into yhat_buf and A^T((f(d) - y) * (2 lam / N)) into a zeroed g from
                    # one trace; the residual launch below then only sums the loss
                    g = None if two_trace else t.zeros_like(d)
                    if two_trace:
                        f._forward_into(d, yhat_buf)
                    elif poisson is not None:
                        # (A^T(s + ((-s) y) / (f(d) + eps)) from the one trace)
                        f._poisson_into(d, m64, s_res, poisson, yhat_buf, g)
                    elif robust is not None:
                        # (a robust term: A^T(s psi(f(d) - y)), the fixed-point bound formed on
                        # the device from s)
                        # (s does not change: the record is written by the first iteration)
                        f._robust_into(d, m64, s_res, robust, yhat_buf, g, *fixed,
                                       scaled=bool(fixed) and it > 0)
                    elif fs.weighted is None:
                        f._normal_into(d, m64, fs.scale, yhat_buf, g, *fixed)
                    else:
                        f._normal_into(d, m64, fs.scale, yhat_buf, g, *fixed,
                                       weighted=fs.weighted)
                    yhat = yhat_buf.view(yd.shape)
                elif loop_desc is not None:
                    # (staged: the forward reads the brick copy the previous Adam launch wrote;
                    # the first one packs it)
                    f._forward_staged(d, yhat_buf, loop_desc)
                    if staged is not None:
                        loop_desc.stage_packed = 1
                    yhat = yhat_buf.view(yd.shape)
                else:
                    yhat = f(d)
                if yhat.shape != yd.shape:
                    raise ValueError(f'measurements {tuple(yd.shape)} do not match the operator '
                                     f'output {tuple(yhat.shape)}')
                # the adjoint's input and the partial sums of the loss in one launch
                # (csrc/loss.hip; the docstring's s and sums, by the fidelity term)
                r_scaled = t.empty_like(yhat)
                fs.residual(yhat, r_scaled, part_sq[it], stream)
                if not fused:
                    g = f._apply_adjoint(r_scaled, tuple(d.shape), d.dtype, d.device,
                                         trace_order=fs.order is not None)
                elif two_trace:
                    g = t.empty_like(d)
                    f._backproject_fixed_into(r_scaled, g, fixed[0])
                if reduce is not None:
                    reduce(g)          # data-parallel: the sum of every rank's adjoint
                if smooth is not None:
                    # g = g + (G_smooth + g_neg) in place and both regularisers' partial sums
                    # (sphrt_smooth_reg_f64: the NegRegularizer's term folded in, so the
                    # optimiser step below takes none)
                    smooth._launch(d, smooth_wrap, smooth.lam, c_neg, g, g, part_smooth[it],
                                   part_neg[it] if neg is not None else None)
                    if step is not None:
                        step(g, 0.0, None, stream, staged[0] if staged is not None else None)
                elif step is not None:
                    # the regulariser's gradient term and loss partials inside the Adam launch
                    step(g, c_neg, part_neg[it] if neg is not None else None, stream,
                         staged[0] if staged is not None else None)
                elif neg is not None:
                    # g -= lam/N where d < 0, and the partial sums of |clamp(d, max=0)|
                    _lib.check(lib.sphrt_neg_reg_f64(_lib.ptr(d), n_vox, c_neg, _lib.ptr(g),
                                                     _lib.ptr(part_neg[it]), stream),
                               'sphrt_neg_reg_f64')
                if progress_bar:      # (this rank's share of the SquareLoss when data-parallel)
                    fv = float(scaled(part_sq[it].sum(), n_norm, sq.lam))
                    rv = float(scaled(part_neg[it].sum(), n_vox, neg.lam)) if neg is not None else 0
                    if smooth is not None:
                        rv += float(scaled(part_smooth[it].sum(), n_vox, smooth.lam))
                    bar.describe(f'F:{fv:.1e} R:{rv:.1e} O:0')
                if step is None:
                    coeffs.grad = g
                    opt.step()
                done = it + 1
    except KeyboardInterrupt:
        if reduce is not None:
            # data-parallel: the other ranks may have stopped at another iteration, and the
            # loss sums below are reduced over equal lengths only — stop every rank loudly
            raise
    sums = part_sq[:done].sum(-1)
    if reduce is not None:
        reduce(sums)
    if neg is not None:
        sums = t.cat([sums, part_neg[:done].sum(-1)])
    if smooth is not None:
        sums = t.cat([sums, part_smooth[:done].sum(-1)])
    # the return value's forward goes out before the readback waits (best is these coefficients
    # unless no iteration's total was finite, below)
    y_best = f(coeffs)
    # one readback for both terms; the scaling in Python floats (the weights are Python
    # numbers, _direct_plan) is the IEEE float64 division and product the tensor ops would do
    host = sums.cpu().tolist()
    losses[sq] = [scaled(v, n_norm, sq.lam) for v in host[:done]]
    if neg is not None:
        losses[neg] = [scaled(v, n_vox, neg.lam) for v in host[done:2 * done]]
    if smooth is not None:
        losses[smooth] = [scaled(v, n_vox, smooth.lam) for v in host[len(host) - done:]]
    # the reference's bookkeeping: the coefficients once some iteration's total was < inf
    totals = [sum(v) for v in zip(*(losses[fn] for fn in loss_fns))]
    best = coeffs if any(v < float('inf') for v in totals) else None
    return best, (y_best if best is not None else f(best)), losses


def _number(v):
    """A plain Python scalar hyper-parameter (torch's defaults mix ints and floats: weight_decay=0)."""
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _split_adam(opt, coeffs):
    """torch.optim.Adam's step on `coeffs` as one csrc/loss.hip launch, or None.

    The launch runs the per-element arithmetic of the implementation torch itself would pick for
    this optimiser, bitwise: torch._fused_adam_ for Adam(fused=True) (sphrt_adam_neg_f64;
    `test_adam_matches_torch_fused`), the multi-tensor foreach step for the default Adam on a GPU
    tensor (sphrt_adam_foreach_neg_f64; `test_adam_matches_torch_foreach`) — the reference's own
    `optim(optim_vars, **kwargs)` (retrieval.py:84).  Either way it is one launch over the whole
    volume with the NegRegularizer's gradient term folded in, where torch runs ~10 foreach
    launches (or a fused step of one workgroup per 65536 elements: a 64^3 volume is 4 workgroups
    on a 256-CU GPU), and given a brick-staged forward descriptor (stage_of) it writes the
    updated coefficients to its stage too.  The optimiser's own state is left untouched (the loop
    owns the moments and the step count).  Anything else (amsgrad, maximize, capturable,
    differentiable, tensor hyper-parameters, the single-tensor path): None, and opt.step() runs."""
    from . import _lib
    if type(opt) is not t.optim.Adam or len(opt.param_groups) != 1:
        return None
    grp = opt.param_groups[0]
    if not (not grp.get('amsgrad') and not grp.get('maximize') and not grp.get('capturable')
            and not grp.get('differentiable') and not grp.get('decoupled_weight_decay')
            and all(_number(grp[k]) for k in ('lr', 'eps', 'weight_decay'))
            and all(_number(b) for b in grp['betas'])
            and len(grp['params']) == 1 and grp['params'][0] is coeffs):
        return None
    fused, foreach = grp.get('fused'), grp.get('foreach')
    if not fused and foreach is None:       # torch's own resolution (Optimizer defaults)
        try:   # a private torch helper: if it moves or changes, the generic opt.step() runs
            from torch.optim.optimizer import _default_to_fused_or_foreach
            _, foreach = _default_to_fused_or_foreach([coeffs], False, use_fused=False)
        except (ImportError, TypeError):
            return None
    if not fused and not foreach:
        return None
    lib = _lib.load()
    flat = coeffs.detach().view(-1)
    m, v = t.zeros_like(flat), t.zeros_like(flat)
    b1, b2 = (float(b) for b in grp['betas'])
    lr, eps, wd = (float(grp[k]) for k in ('lr', 'eps', 'weight_decay'))
    count = [0]

    def step(g, c_neg, part, stream, stage_of=None):
        count[0] += 1
        stage = ctypes.byref(stage_of) if stage_of is not None else None
        if fused:
            _lib.check(lib.sphrt_adam_neg_f64(
                _lib.ptr(flat), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), flat.numel(), lr, b1, b2,
                eps, wd, float(count[0]), c_neg, _lib.ptr(part), stage, stream),
                'sphrt_adam_neg_f64')
            return
        # the foreach step's bias corrections, as torch computes them (Python floats of the
        # float32 step count)
        st = float(count[0])
        step_size = (lr / (1 - b1 ** st)) * -1
        bc2_sqrt = (1 - b2 ** st) ** 0.5
        _lib.check(lib.sphrt_adam_foreach_neg_f64(
            _lib.ptr(flat), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), flat.numel(), step_size, b1, b2,
            eps, wd, bc2_sqrt, c_neg, _lib.ptr(part), stage, stream), 'sphrt_adam_foreach_neg_f64')
    return step


# ---- conjugate gradients ------------------------------------------------------------------------

def cg(f, y, loss_fns=[SquareLoss()], x0=None, num_iterations=50, damp=0.0, tol=0.0,
       progress_bar=False):
    """Minimise, by conjugate gradients, the total `gd` minimises for the same `loss_fns` when
    that total is quadratic:

        J(x) = lam_f * mean(w * (y - f(x))^2) + lam_s * SmoothRegularizer(kind='square')(x)
               + damp * mean(x^2)

    -> (x, f(x), info).  No learning rate: grad J(x) = N x - b with N = A^T diag(s) A + G + c I
    symmetric positive semi-definite, s = 2 (lam_f / M) w, c = 2 damp / V (M = y.numel(),
    V = x.numel()), G the smooth term's (linear) gradient and b = A^T(s y); the solve starts at
    `x0` (default: zeros of f.grid.shape, float64) with r_0 = -grad J(x0) and runs
    `num_iterations` iterations.  Once |r_k|^2 <= tol^2 |r_0|^2 the iteration freezes (alpha =
    beta = 0 from then on: x no longer changes); nothing is read back during the loop, so there
    is no early exit, and tol = 0 never freezes.  info = {'residual': [|r_k| / |r_0| for k = 0 ..
    num_iterations] (0.0 where r_k is exactly zero), 'converged_at': the first k at or under
    tol, or None}.

    `loss_fns`: exactly one SquareLoss (that type itself; scalar lam, unit volume_mask, a
    projection_mask that is 1 or a tensor `gd`'s direct loop would weigh the residual with) and at
    most one SmoothRegularizer(kind='square') (scalar lam, unit masks).  Anything else is not
    quadratic or not known to be, and raises ValueError naming the term.

    A static Operator (with its trace) or a static MatrixFreeOperator, float32 / float64
    measurements of the operator's ray shape on its GPU and an `x0` that is None or a contiguous
    float64 grid.shape tensor there run `_cg_direct`: the operator's own launches and three
    csrc/loss.hip launches per iteration, the whole solve enqueued without a host sync and —
    over an Operator, or a MatrixFreeOperator with `deterministic` set — bitwise reproducible.
    Everything else (CPU tensors, other operators, dynamic grids, other dtypes) runs the same
    algorithm in plain torch (`_cg_generic`)."""
    sq, smooth = _cg_terms(y, loss_fns, damp, tol, num_iterations)
    bar = _Bar(range(num_iterations), progress_bar)
    if _cg_is_direct(f, y, x0):
        return _cg_direct(f, y, sq, smooth, x0, num_iterations, float(damp), float(tol), bar)
    return _cg_generic(f, y, sq, smooth, x0, num_iterations, float(damp), float(tol), bar)


def _cg_terms(y, loss_fns, damp, tol, num_iterations, who='cg'):
    """(the SquareLoss, the SmoothRegularizer or None) of a total `cg` solves; ValueError naming
    what it does not.  `fista` takes the same totals by the same rules, under its own name."""
    if not isinstance(y, t.Tensor):
        raise ValueError(f'{who} needs measurements y as a tensor, not {type(y).__name__}')
    for name, v in (('damp', damp), ('tol', tol)):
        if not _number(v) or not 0 <= v < float('inf'):
            raise ValueError(f'{who} needs a finite {name} >= 0, not {v!r}')
    if isinstance(num_iterations, bool) or not isinstance(num_iterations, int) \
            or num_iterations < 0:
        raise ValueError(f'{who} needs num_iterations as an integer >= 0, not {num_iterations!r}')
    sq = smooth = None
    for fn in loss_fns:
        name = type(fn).__name__
        if type(fn) is SquareLoss:
            if sq is not None:
                raise ValueError(f'{who} solves for one SquareLoss, not two')
            sq = fn
        elif type(fn) is SmoothRegularizer:
            if smooth is not None:
                raise ValueError(f'{who} solves with at most one SmoothRegularizer, not two')
            if fn.smooth_kind != 'square':
                raise ValueError(f"{who} needs a quadratic total: SmoothRegularizer(kind="
                                 f"{fn.smooth_kind!r}) is not (kind='square' is)")
            smooth = fn
        else:
            raise ValueError(f'{who} needs a quadratic total of one SquareLoss and at most one '
                             f"SmoothRegularizer(kind='square'): {name} is neither (gd takes it)")
        if not fn.use_grad:
            raise ValueError(f'{who}: {name}(use_grad=False) is a monitor, not a term of the total')
        if not _number(fn.lam) or not math.isfinite(fn.lam):
            raise ValueError(f'{who} needs a finite scalar lam, not {name}.lam = {fn.lam!r}')
        if not _unit(fn.volume_mask):
            raise ValueError(f'{who} does not take a volume_mask ({name})')
        if not _unit(fn.projection_mask) and not (fn is sq and _ray_mask(fn.projection_mask, y)):
            raise ValueError(f'{who}: the projection_mask of {name} must be 1' + (
                ' or a bool / float32 / float64 tensor on the device of y that broadcasts to '
                'its shape' if fn is sq else ''))
    if sq is None:
        raise ValueError(f'{who} needs one SquareLoss among loss_fns')
    return sq, smooth


def _cg_is_direct(f, y, x0):
    """Does `_cg_direct` run this solve (`cg`'s docstring)."""
    from .raytracer import MatrixFreeOperator, Operator
    if type(f) is Operator:
        if f.dynamic or f.grid.dynamic or f._csr is None:
            return False
    elif type(f) is MatrixFreeOperator:
        if f.dynamic or f.grid.dynamic:
            return False
    else:
        return False
    if not (y.is_cuda and y.device == f._cdev and y.dtype in (t.float32, t.float64)
            and tuple(y.shape) == tuple(f._ray_shape)):
        return False
    return x0 is None or (isinstance(x0, t.Tensor) and x0.device == f._cdev
                          and x0.dtype == t.float64 and x0.is_contiguous()
                          and tuple(x0.shape) == tuple(f.grid.shape))


def _cg_info(rr, stop):
    """`cg`'s info from the squared residual norms of k = 0 .. K and the freeze threshold (host
    floats; stop None: tol = 0)."""
    rr0 = rr[0]
    hist = [0.0 if v == 0 else math.sqrt(v / rr0) if rr0 > 0 else float('nan') for v in rr]
    at = None if stop is None else next((k for k, v in enumerate(rr) if v <= stop), None)
    return {'residual': hist, 'converged_at': at}


def _normal_generic(f, yd, sq, smooth, x):
    """normal(d, m) = A^T(s (A d - m)) + G d in plain torch, through f(d) and f._apply_adjoint
    alone (m = None: no measurements), for volumes like `x`: what `_cg_generic` and
    `_fista_generic` iterate (the damping term is theirs)."""
    dshape, dtype, dev = tuple(x.shape), x.dtype, x.device
    c_sq = sq.lam / yd.numel()
    s = 2 * c_sq if _unit(sq.projection_mask) else \
        (c_sq * sq.projection_mask.detach().to(t.promote_types(yd.dtype, dtype))) * 2

    def smooth_grad(d):
        # (linear in d: the square kind's gradient, lam and 1 / V included)
        with t.enable_grad():
            leaf = d.detach().requires_grad_()
            g, = t.autograd.grad(smooth(f, yd, leaf, leaf), leaf)
        return g

    def normal(d, m):
        q = f(d)
        h = f._apply_adjoint(s * (q if m is None else q - m), dshape, dtype, dev)
        if smooth is not None:
            h = h + smooth_grad(d)
        return h
    return normal


def _cg_generic(f, y, sq, smooth, x0, num_iterations, damp, tol, bar):
    """`cg` in plain torch, through f(x) and f._apply_adjoint alone: the specification of
    `_cg_direct` (the same guards in the same places; sums in torch's order) and what runs on
    the CPU.  Every scalar stays a 0-dim tensor on the device: no sync inside the loop."""
    with t.no_grad():
        yd = y.detach()
        x = t.zeros(tuple(f.grid.shape), dtype=t.float64, device=yd.device) if x0 is None \
            else t.as_tensor(x0).detach().clone()
        c = 2 * damp / x.numel()
        normal = _normal_generic(f, yd, sq, smooth, x)

        def gradient(d, m):
            """A^T(s (A d - m)) + G d + c d: grad J(d) with m = y, N d with m = None."""
            return t.add(normal(d, m), d, alpha=c)

        def frozen(v):
            return v <= stop if stop is not None else t.zeros_like(v, dtype=t.bool)

        r = -gradient(x, yd)
        p = r.clone()
        rr = (r * r).sum()
        stop = rr * (tol * tol) if tol > 0 else None
        zero, rrs = t.zeros_like(rr), [rr]
        try:
            for _ in bar:
                h = gradient(p, None)
                php = (p * h).sum()
                q = rr / php
                alpha = t.where(frozen(rr) | ~(php > 0) | ~t.isfinite(q), zero, q)
                x = x + alpha * p
                r = r - alpha * h
                rr_new = (r * r).sum()
                beta = t.where(frozen(rr) | ~(rr > 0), zero, rr_new / rr)
                p = r + beta * p
                rr = rr_new
                rrs.append(rr)
        except KeyboardInterrupt:
            pass
        y_hat = f(x)
        host = t.stack(rrs + ([stop] if stop is not None else [])).cpu().tolist()
    return x, y_hat, _cg_info(host[:len(rrs)], host[-1] if stop is not None else None)


def _kernel_sum(part):
    """The sum every workgroup of the cg kernels forms of a row of partial sums (SUM of
    include/sphrt.h, csrc/loss.hip block_totals), restated with elementwise torch adds in the
    same order: the same bits, for each row of `part` (..., n_part <= 1024).  Threads past
    n_part hold +0.0, and x + 0.0 is x for every x the first `0.0 +` can leave."""
    rows = part.reshape(-1, part.shape[-1])
    pad = t.zeros((rows.shape[0], 4, 256), dtype=part.dtype, device=part.device)
    pad.view(rows.shape[0], -1)[:, :rows.shape[1]] = rows
    v = (((0.0 + pad[:, 0]) + pad[:, 1]) + pad[:, 2]) + pad[:, 3]       # a thread's slice
    v = v.view(-1, 4, 64)
    for half in (32, 16, 8, 4, 2, 1):                                   # lane 0 of the butterfly
        v = v[..., :half] + v[..., half:2 * half]
    v = v[..., 0]
    return ((((0.0 + v[:, 0]) + v[:, 1]) + v[:, 2]) + v[:, 3]).reshape(part.shape[:-1])


def _normal_direct(f, y, sq, smooth, x):
    """apply(d) / apply(d, against_y=True) = A^T(s (A d - m)) + G d, m = 0 or y, on the operator's
    own entries (`_cg_is_direct`), for contiguous float64 volumes like `x` on the operator's GPU:
    what `_cg_direct` and `_fista_direct` iterate (the damping term is theirs).  Over a
    MatrixFreeOperator one trace (`_normal_into`: q = A d and A^T(s (q - m))); over an Operator
    the loop's forward, the residual kernel (s (q - m) in the adjoint's order) and the adjoint;
    then, with a smooth term, one sphrt_smooth_reg_f64 launch.  The result is a buffer the next
    application may overwrite.  -> (apply, the count of partial sums of a launch over a volume)."""
    from . import _lib
    lib = _lib.load()
    dev, f64 = f._cdev, t.float64
    fs = _fidelity_stage(f, y, sq, zero_m=True)
    n_meas, n_vox = fs.n_meas, x.numel()
    pn, ps = lib.sphrt_loss_partials(n_vox), lib.sphrt_loss_partials(n_meas)
    part_tmp = t.empty(max(pn, ps), dtype=f64, device=dev)   # (sums nobody reads)
    wrap = smooth.wraps(f) if smooth is not None else None
    q_buf = t.empty(n_meas, dtype=f64, device=dev)
    if fs.fused:
        h_buf = t.empty_like(x)

        def normal(d, against_y):
            """A^T(s (A d - m)), m = y or 0, into h_buf from one trace."""
            if not fs.fixed:
                h_buf.zero_()
            f._normal_into(d, fs.m64 if against_y else fs.zero_m, fs.scale, q_buf, h_buf,
                           *fs.fixed, weighted=fs.weighted)
            return h_buf
    else:
        rs_buf = t.empty(n_meas, dtype=f64, device=dev)

        def normal(d, against_y):
            """A^T(s (A d - m)), m = y or 0: forward, scaled residual, adjoint."""
            if fs.loop_desc is not None:
                f._forward_staged(d, q_buf, fs.loop_desc)
                q = q_buf
            else:
                q = f(d).reshape(-1)
            fs.residual(q, rs_buf, part_tmp, _lib.stream_of(dev), against_y)
            return f._apply_adjoint(rs_buf.view(fs.yd.shape), tuple(d.shape), d.dtype, dev,
                                    trace_order=fs.order is not None)

    def apply(d, against_y=False):
        h = normal(d, against_y)
        if smooth is not None:
            smooth._launch(d, wrap, smooth.lam, 0.0, h, h, part_tmp, None)
        return h
    return apply, pn


def _cg_direct(f, y, sq, smooth, x0, num_iterations, damp, tol, bar):
    """`cg` on the operator's own entries (`_cg_is_direct`).  An iteration is h = N p — over a
    MatrixFreeOperator one trace (`_normal_into` against zero measurements: q = A p and
    A^T(s q)), over an Operator the loop's forward, the residual kernel against zero
    measurements (s q in the adjoint's order) and the adjoint; then, with a smooth term, one
    sphrt_smooth_reg_f64 launch (h += G p): `_normal_direct`, which `_fista_direct` shares —
    followed by three csrc/loss.hip launches:
    sphrt_cg_curvature_f64 (h += c p, partial sums of p h), sphrt_cg_update_f64 (alpha from the
    partial sums; x += alpha p, r -= alpha h, partial sums of r r) and sphrt_cg_direction_f64
    (beta; p = r + beta p).  alpha, beta and the freeze live on the device, formed by every
    workgroup from the partial sums in one fixed order (`_kernel_sum` restates it), so nothing
    is read back before the loop ends; the residual history is then one row of partial sums per
    iteration.  The first residual goes through the same launches: g = grad J(x0) from the
    operator's entries against y, the smooth launch and the curvature launch on x0, and an update
    launch with alpha = 1 on zeroed r and p (r = -g, x unchanged, the partial sums of r r)."""
    from . import _lib
    lib = _lib.load()
    dev, f64 = f._cdev, t.float64
    with t.no_grad(), t.cuda.device(dev):
        x = t.zeros(tuple(f.grid.shape), dtype=f64, device=dev) if x0 is None \
            else x0.detach().clone()
        n_vox = x.numel()
        c = 2 * damp / n_vox
        r, p = t.zeros_like(x), t.zeros_like(x)
        apply, pn = _normal_direct(f, y, sq, smooth, x)
        part_rr = t.empty((num_iterations + 1, pn), dtype=f64, device=dev)
        part_php = t.empty(pn, dtype=f64, device=dev)

        def curvature(d, against_y):
            """h = A^T(s (A d - m)) + G d + c d and the partial sums of d h (part_php)."""
            h = apply(d, against_y)
            _lib.check(lib.sphrt_cg_curvature_f64(_lib.ptr(d), _lib.ptr(h), n_vox, c,
                                                  _lib.ptr(part_php), _lib.stream_of(dev)),
                       'sphrt_cg_curvature_f64')
            return h

        def update(h, rr_in, php_in, stop, rr_out):
            _lib.check(lib.sphrt_cg_update_f64(
                _lib.ptr(x), _lib.ptr(r), _lib.ptr(p), _lib.ptr(h), n_vox, _lib.ptr(rr_in),
                _lib.ptr(php_in), pn, _lib.ptr(stop), _lib.ptr(rr_out), _lib.stream_of(dev)),
                'sphrt_cg_update_f64')

        # r_0 = -grad J(x0) and its partial sums: an update with alpha = 1 / 1 on r = p = 0
        # (a fill launch: `one[0] = 1.0` copies a host scalar into the 0-dim view, a pageable
        # copy that synchronises the host with the stream)
        one = t.zeros(pn, dtype=f64, device=dev)
        one[:1].fill_(1.0)
        update(curvature(x, True), one, one, None, part_rr[0])
        p.copy_(r)
        stop = (_kernel_sum(part_rr[0]) * (tol * tol)).reshape(1) if tol > 0 else None
        done = 0
        try:
            for it in bar:
                h = curvature(p, False)
                update(h, part_rr[it], part_php, stop, part_rr[it + 1])
                _lib.check(lib.sphrt_cg_direction_f64(
                    _lib.ptr(p), _lib.ptr(r), n_vox, _lib.ptr(part_rr[it + 1]),
                    _lib.ptr(part_rr[it]), pn, _lib.ptr(stop), _lib.stream_of(dev)),
                    'sphrt_cg_direction_f64')
                done = it + 1
        except KeyboardInterrupt:
            pass
        y_hat = f(x)       # (goes out before the readback waits)
        sums = _kernel_sum(part_rr[:done + 1])
        host = (t.cat([sums, stop]) if stop is not None else sums).cpu().tolist()
    return x, y_hat, _cg_info(host[:done + 1], host[-1] if stop is not None else None)


# ---- bound-constrained solver: projected gradient with momentum -----------------------------------

# The step-size estimate ("Bound-constrained solver": the study that chose them).
_FISTA_POWER_ITERATIONS = 10
_FISTA_MARGIN = 0.3


def fista(f, y, loss_fns=[SquareLoss()], x0=None, num_iterations=100, damp=0.0, lower=0.0,
          upper=None, lipschitz=None, power_iterations=_FISTA_POWER_ITERATIONS,
          progress_bar=False):
    """Minimise the total `cg` solves,

        J(x) = lam_f * mean(w * (y - f(x))^2) + lam_s * SmoothRegularizer(kind='square')(x)
               + damp * mean(x^2),

    subject to lower <= x <= upper elementwise, by FISTA with a fixed step 1 / L and a gradient
    restart -> (x, f(x), info).  Every iterate, the returned one included, satisfies the bounds
    exactly.  `lower` / `upper`: Python numbers with lower < upper, None for no bound on that
    side.  `loss_fns`, `damp` and `num_iterations` by `cg`'s rules (anything not quadratic raises
    ValueError naming the term).

    With grad J(x) = N x - b (`cg`'s docstring), x_0 = z_0 = clamp(x0 or zeros), j = 0 and the
    momentum table OMEGA (`_fista_omega`), iteration k is

        g  = N z - b                       (the damping term by one fma: g = fma(c, z, .))
        u  = fma(-1 / L, g, z);  x_{k+1} = u < lower ? lower : (u > upper ? upper : u)
        GD = sum g (x_{k+1} - x_k);  MM = sum (z - x_{k+1})^2
        j  = 1 if GD > 0 else j + 1        (the restart; a NaN GD does not restart)
        z  = fma(OMEGA[j], x_{k+1} - x_k, x_{k+1})

    L must be at least the largest eigenvalue of N.  `lipschitz`: a finite number > 0, or None:
    the Rayleigh quotient after `power_iterations` steps of the power method on N from the
    all-ones volume, times 1 + 0.3 (it is a lower bound; the margin and the default count are
    measured in DESIGN §5).  info = {'residual': [sqrt(MM_k / MM_0) for k = 0 .. K - 1] (0.0
    where MM_k is exactly zero), 'restarts': the iterations k >= 1 at which j was reset,
    'lipschitz': L}.  There is no tolerance and no early exit.

    The inputs `cg` runs directly (`_cg_is_direct`) run `_fista_direct`: the operator's own
    launches and two csrc/loss.hip launches per iteration, L, the step and the restart decision
    on the device, the whole solve enqueued without a host sync and bitwise reproducible where
    the adjoint is.  Everything else runs the same algorithm in plain torch (`_fista_generic`)."""
    sq, smooth = _cg_terms(y, loss_fns, damp, 0.0, num_iterations, who='fista')
    bounds = _fista_args(lower, upper, lipschitz, power_iterations)
    bar = _Bar(range(num_iterations), progress_bar)
    run = _fista_direct if _cg_is_direct(f, y, x0) else _fista_generic
    return run(f, y, sq, smooth, x0, num_iterations, float(damp), bounds[0], bounds[1],
               None if lipschitz is None else float(lipschitz), power_iterations, bar)


def _fista_args(lower, upper, lipschitz, power_iterations, who='fista'):
    """(lower, upper) as floats, None being no bound; ValueError naming the argument that is
    not what `fista` takes.  `primal_dual` takes the same arguments, under its own name."""
    bounds = []
    for name, v, none in (('lower', lower, -math.inf), ('upper', upper, math.inf)):
        if v is None:
            v = none
        if not _number(v) or math.isnan(v):
            raise ValueError(f'{who} needs {name} as a number (not NaN) or None, not {v!r}')
        bounds.append(float(v))
    if not bounds[0] < bounds[1]:
        raise ValueError(f'{who} needs lower < upper, not lower = {lower!r}, upper = {upper!r}')
    if lipschitz is not None and (not _number(lipschitz) or not 0 < lipschitz < math.inf):
        raise ValueError(f'{who} needs a finite lipschitz > 0 (or None), not {lipschitz!r}')
    if isinstance(power_iterations, bool) or not isinstance(power_iterations, int) \
            or power_iterations < 1:
        raise ValueError(f'{who} needs power_iterations as an integer >= 1, not '
                         f'{power_iterations!r}')
    return bounds


def _fista_omega(num_iterations):
    """The momentum table as Python floats, length num_iterations + 1: OMEGA[0] = OMEGA[1] = 0
    and OMEGA[j] = (t_j - 1) / t_{j+1} with t_1 = 1, t_{j+1} = (1 + sqrt(1 + 4 t_j^2)) / 2."""
    omega, tj = [0.0], 1.0
    for _ in range(num_iterations):
        tn = (1.0 + math.sqrt(1.0 + 4.0 * tj * tj)) / 2.0
        omega.append((tj - 1.0) / tn)
        tj = tn
    return omega


def _fista_step(matvec, like, lipschitz, power_iterations):
    """(L, 1 / L) as one-element tensors on the device of `like`, nothing read back.  lipschitz
    None: v = ones; `power_iterations` times: w = N v (`matvec`), rho = v.w / v.v, v = w / |w|;
    L = rho (1 + margin).  An L that is not > 0 (N = 0: every x is a minimiser) gives a step of 0
    instead of a division by it."""
    if lipschitz is not None:
        L = t.full((1,), lipschitz, dtype=like.dtype, device=like.device)
    else:
        v = t.ones_like(like)
        for _ in range(power_iterations):
            w = matvec(v)
            rho = (v * w).sum() / (v * v).sum()
            v = w / w.norm()
        L = (rho * (1.0 + _FISTA_MARGIN)).reshape(1)
    return L, t.where(L > 0, 1.0 / L, t.zeros_like(L))


def _fista_info(mm, jrec, L):
    """`fista`'s info from MM_k (k = 0 .. K - 1), the record of j (K + 1 entries) and L, on the
    host."""
    mm0 = mm[0] if mm else 0.0
    hist = [0.0 if v == 0 else math.sqrt(v / mm0) if mm0 > 0 else float('nan') for v in mm]
    return {'residual': hist, 'lipschitz': L,
            'restarts': [k for k in range(1, len(jrec) - 1) if jrec[k + 1] == 1]}


def _fista_generic(f, y, sq, smooth, x0, num_iterations, damp, lower, upper, lipschitz,
                   power_iterations, bar):
    """`fista` in plain torch, through f(x) and f._apply_adjoint alone: the specification of
    `_fista_direct` (sums in torch's order) and what runs on the CPU.  Every scalar, j included,
    stays a tensor on the device: no sync inside the loop."""
    with t.no_grad():
        yd = y.detach()
        x = t.zeros(tuple(f.grid.shape), dtype=t.float64, device=yd.device) if x0 is None \
            else t.as_tensor(x0).detach().clone()
        c = 2 * damp / x.numel()
        normal = _normal_generic(f, yd, sq, smooth, x)
        lo, hi = (t.full((), v, dtype=x.dtype, device=x.device) for v in (lower, upper))

        def clamp(u):
            return t.where(u < lo, lo, t.where(u > hi, hi, u))

        L, step = _fista_step(lambda v: t.add(normal(v, None), v, alpha=c), x, lipschitz,
                              power_iterations)
        x = clamp(x)
        z = x
        omega = t.tensor(_fista_omega(num_iterations), dtype=x.dtype, device=x.device)
        j = t.zeros(1, dtype=t.int64, device=x.device)
        one, mms, js = t.ones_like(j), [], [j]
        try:
            for _ in bar:
                g = t.add(normal(z, yd), z, alpha=c)
                x_new = clamp(t.addcmul(z, g, -step))
                gd = (g * (x_new - x)).sum()
                mm = ((z - x_new) ** 2).sum()
                j = t.where(gd > 0, one, j + 1)
                z = t.addcmul(x_new, x_new - x, omega.index_select(0, j))
                x = x_new
                mms.append(mm)
                js.append(j)
        except KeyboardInterrupt:
            pass
        y_hat = f(x)
        done = len(mms)
        host = t.cat([t.stack(mms).to(t.float64) if done else L.new_zeros(0).to(t.float64),
                      t.cat(js).to(t.float64), L.to(t.float64)]).cpu().tolist()
    return x, y_hat, _fista_info(host[:done], host[done:2 * done + 1], host[-1])


def _fista_direct(f, y, sq, smooth, x0, num_iterations, damp, lower, upper, lipschitz,
                  power_iterations, bar):
    """`fista` on the operator's own entries (`_cg_is_direct`).  An iteration is g = N z - b
    without the damping term (`_normal_direct` against y: over a MatrixFreeOperator one trace,
    over an Operator its forward, residual and adjoint launches; the smooth launch with a smooth
    term) followed by two csrc/loss.hip launches: sphrt_pg_step_f64 (the damping term, the step,
    the clamp into the other of two x buffers, partial sums of GD and MM) and
    sphrt_pg_momentum_f64 (GD from the partial sums in every workgroup, j, z, and j into the next
    slot of a (K + 1,) int64 record).  The step 1 / L is a one-element device tensor the step
    launch reads through a pointer — the power method runs in torch over the same application —
    so nothing is read back before the loop ends; then MM_k is one row of partial sums per
    iteration (`_kernel_sum`), and the record of j gives the restarts."""
    from . import _lib
    lib = _lib.load()
    dev, f64 = f._cdev, t.float64
    with t.no_grad(), t.cuda.device(dev):
        x = t.zeros(tuple(f.grid.shape), dtype=f64, device=dev) if x0 is None \
            else x0.detach().clone()
        n_vox = x.numel()
        c = 2 * damp / n_vox
        apply, pn = _normal_direct(f, y, sq, smooth, x)
        L, step = _fista_step(lambda v: t.add(apply(v), v, alpha=c), x, lipschitz,
                              power_iterations)
        lo, hi = (t.full((), v, dtype=f64, device=dev) for v in (lower, upper))
        x = t.where(x < lo, lo, t.where(x > hi, hi, x))
        x_new, z = t.empty_like(x), x.clone()
        # (from pinned memory, not waited for: a tensor built on the device from a Python list is
        # a pageable copy, which synchronises the host with the stream)
        omega = t.tensor(_fista_omega(num_iterations), dtype=f64, pin_memory=True).to(
            dev, non_blocking=True)
        jrec = t.zeros(num_iterations + 1, dtype=t.int64, device=dev)
        part_gd = t.empty(pn, dtype=f64, device=dev)
        part_mm = t.empty((max(num_iterations, 1), pn), dtype=f64, device=dev)
        done = 0
        try:
            for it in bar:
                g = apply(z, True)
                stream = _lib.stream_of(dev)
                _lib.check(lib.sphrt_pg_step_f64(
                    _lib.ptr(z), _lib.ptr(g), _lib.ptr(x), _lib.ptr(x_new), n_vox, c,
                    _lib.ptr(step), lower, upper, _lib.ptr(part_gd), _lib.ptr(part_mm[it]),
                    stream), 'sphrt_pg_step_f64')
                _lib.check(lib.sphrt_pg_momentum_f64(
                    _lib.ptr(z), _lib.ptr(x_new), _lib.ptr(x), n_vox, _lib.ptr(part_gd), pn,
                    _lib.ptr(omega), omega.numel(), _lib.ptr(jrec[it:]), _lib.ptr(jrec[it + 1:]),
                    stream), 'sphrt_pg_momentum_f64')
                x, x_new = x_new, x
                done = it + 1
        except KeyboardInterrupt:
            pass
        y_hat = f(x)       # (goes out before the readback waits)
        mm = _kernel_sum(part_mm[:done]) if done else L.new_zeros(0)
        host = t.cat([mm, jrec[:done + 1].to(f64), L]).cpu().tolist()
    return x, y_hat, _fista_info(host[:done], host[done:2 * done + 1], host[-1])


# ---- total variation: a primal-dual solver ---------------------------------------------------------

def primal_dual(f, y, loss_fns, x0=None, num_iterations=100, damp=0.0, lower=0.0, upper=None,
                lipschitz=None, power_iterations=_FISTA_POWER_ITERATIONS, dual_ratio=1.0,
                progress_bar=False):
    """Minimise, subject to lower <= x <= upper elementwise, the total `fista` solves plus an
    anisotropic total variation,

        J(x) = lam_f * mean(w * (y - f(x))^2) + lam_s * SmoothRegularizer(kind='square')(x)
               + damp * mean(x^2) + lam_tv * SmoothRegularizer(kind='abs')(x),

    by the primal-dual iteration of Condat and Vu -> (x, f(x), info).  `loss_fns`: one SquareLoss
    and at most one SmoothRegularizer(kind='square') by `cg`'s rules, and exactly one
    SmoothRegularizer(kind='abs') with a scalar lam > 0 and unit masks, at least one of whose
    axes has edges on this grid (weight > 0 and length > 1; its time_weight must be 0 unless
    the volume is 3-D, where the class ignores it).  `lower`, `upper`, `lipschitz`,
    `power_iterations`, `damp` and `num_iterations` as `fista` takes them; `dual_ratio`: a
    finite number > 0.  Anything else raises ValueError naming the offender.

    With grad of the smooth part N x - b (`cg`'s docstring), V = x.numel(), c_ax = lam_tv w_ax /
    V, D the forward differences along the axes that have edges (an edge belongs to its lower
    voxel, the azimuth wrap edge to the ring's last voxel: sphrt_smooth_reg_f64's edges), a dual
    q of shape (3,) + x.shape that is +0.0 where there is no edge, B = 4 (number of axes with
    edges) >= |D|^2 and L as `fista` estimates it,

        tau = 1 / ((1 + dual_ratio) L),   sigma = dual_ratio L / B      (0 both when L is not > 0)

    (1 / tau - sigma |D|^2 >= L > L / 2: Condat's condition).  From x_0 = clamp(x0 or
    zeros), q_0 = 0, iteration k is

        gp  = fma(c, x, N x - b),  c = 2 damp / V
        s   = D^T q
        u   = fma(-tau, gp + s, x);  x+ = u < lower ? lower : (u > upper ? upper : u)
        xb  = fma(2, x+, -x)
        q_ax <- v < -c_ax ? -c_ax : (v > c_ax ? c_ax : v),  v = fma(sigma, (D xb)_ax, q_ax)
        MM_k = sum (x+ - x)^2;  QQ_k = sum (q+ - q)^2

    info = {'primal_change': [sqrt(MM_k / MM_0)] (0.0 where MM_k is exactly 0), 'dual_change':
    [sqrt(QQ_k)], 'lipschitz': L, 'tau', 'sigma', 'dual': q (the tensor: with x it certifies
    optimality)}.  No tolerance, no early exit; every iterate satisfies the bounds and every
    |q_ax| <= c_ax exactly.

    Isotropic TV: exactly one IsoTVRegularizer may stand in place of the abs term (under the same
    rules: a scalar lam > 0, unit masks, use_grad, an axis with edges; both, or two of them,
    raise ValueError).  The term is r sum_i |(Dw x)_i|_2 with Dw_ax = w_ax D_ax and r = lam_tv / V;
    B = 4 sum of w_ax^2 over the axes with edges >= |Dw|^2, s = Dw^T q, and the dual step is the
    projection of each voxel's triple onto the ball of radius r:

        v_ax = fma(sigma, (Dw xb)_ax, q_ax);  nrm = sqrt(sum_ax v_ax^2)
        q_ax <- v_ax (r / nrm) if nrm > r else v_ax                 (include/sphrt_iso.h)

    info keeps its keys; info['dual'] has shape (3,) + x.shape and certifies optimality with
    |q_i|_2 <= r up to sum_ax q_ax^2 <= r^2 (1 + 12 * 2^-53) (the header derives the bound; scale q
    by 1 / (1 + 12 * 2^-53) before using it as a feasible point).

    The inputs `cg` runs directly (`_cg_is_direct`) run `_primal_dual_direct`: the operator's own
    launches and two csrc/loss.hip launches per iteration (include/sphrt_pd.h, or with an
    IsoTVRegularizer include/sphrt_iso.h's two in their place), the whole solve
    enqueued without a host sync and bitwise reproducible where the adjoint is.  Everything else
    runs the same algorithm in plain torch (`_primal_dual_generic`)."""
    who = 'primal_dual'
    tvs = [fn for fn in loss_fns if type(fn) is SmoothRegularizer and fn.smooth_kind == 'abs']
    isos = [fn for fn in loss_fns if type(fn) is IsoTVRegularizer]
    rest = [fn for fn in loss_fns if not any(fn is v for v in tvs + isos)]
    sq, smooth = _cg_terms(y, rest, damp, 0.0, num_iterations, who=who)
    if isos and tvs:
        raise ValueError(f"{who} solves with one TV term: an IsoTVRegularizer beside a "
                         "SmoothRegularizer(kind='abs') is not built")
    if len(isos) > 1:
        raise ValueError(f'{who} solves with one IsoTVRegularizer, not {len(isos)}')
    if not tvs and not isos:
        raise ValueError(f"{who} needs one SmoothRegularizer(kind='abs') among loss_fns (fista "
                         'solves the total without it)')
    if len(tvs) > 1:
        raise ValueError(f"{who} solves with one SmoothRegularizer(kind='abs'), not {len(tvs)}")
    term = (isos or tvs)[0]
    label = 'IsoTVRegularizer' if isos else "SmoothRegularizer(kind='abs')"
    _term_rules(who, term, type(term).__name__, label, f' on {label}, not lam = {term.lam!r}')
    bounds = _fista_args(lower, upper, lipschitz, power_iterations, who=who)
    if not _number(dual_ratio) or not 0 < dual_ratio < math.inf:
        raise ValueError(f'{who} needs a finite dual_ratio > 0, not {dual_ratio!r}')
    tv = _tv_on_volume(who, term, f, x0)
    bar = _Bar(range(num_iterations), progress_bar)
    run = _primal_dual_direct if _cg_is_direct(f, y, x0) else _primal_dual_generic
    return run(f, y, sq, smooth, tv, x0, num_iterations, float(damp), bounds[0], bounds[1],
               None if lipschitz is None else float(lipschitz), power_iterations,
               float(dual_ratio), bar)


def _term_rules(who, fn, cls, label, lam_text, rays=None):
    """The rules `primal_dual` and `chambolle_pock` share for a term of their totals, in the order
    both check them: a term of the total, a finite scalar lam > 0 (`lam_text`: the solver's own
    end of that sentence), unit masks — but for a fidelity term, whose projection_mask may be a
    tensor `gd`'s direct loop would weigh the residual with (`rays`: the measurements, then)."""
    if not fn.use_grad:
        raise ValueError(f'{who}: {cls}(use_grad=False) is a monitor, not a term of the total')
    if not _number(fn.lam) or not 0 < fn.lam < math.inf:
        raise ValueError(f'{who} needs a finite scalar lam > 0{lam_text}')
    if not _unit(fn.volume_mask):
        raise ValueError(f'{who} does not take a volume_mask ({label})')
    if not _unit(fn.projection_mask) and not (rays is not None
                                              and _ray_mask(fn.projection_mask, rays)):
        raise ValueError(f'{who}: the projection_mask of {label} must be 1' + (
            ' or a bool / float32 / float64 tensor on the device of y that broadcasts to '
            'its shape' if rays is not None else ''))


class _TVTerm:
    """The TV term of `primal_dual` and `chambolle_pock` on a volume of `shape` over `f`, as the
    refusals, the generic maps (`_tv_maps`) and the direct launches (`_tv_stage`) read it.  `term`:
    a SmoothRegularizer(kind='abs'), an IsoTVRegularizer, or None (`chambolle_pock` without TV:
    no axis has edges).

        has      [has_r, has_e, has_a]: which of the trailing axes have edges
        ring     the azimuth ring is closed (and longer than 1)
        iso      the term is an IsoTVRegularizer: the weights sit in the differences and the dual
                 is projected onto the ball of `radius` = lam / V; otherwise the differences are
                 unweighted and axis ax is clamped to `clamps`[ax] = lam w_ax / V
        bound    B / 4 of the difference operator, B >= |D|^2: the number of axes with edges, or
                 for the iso term the sum of w_ax^2 over them (each 1-D difference operator's
                 bound of 4, scaled by its weight and stacked)
        label    the term as the refusals name it"""

    def __init__(self, term, f, shape):
        self.term, self.iso = term, type(term) is IsoTVRegularizer
        self.weights = term.weights if term is not None else (0.0, 0.0, 0.0)
        self.lam, self.n_vox = term.lam if term is not None else 0.0, math.prod(shape)
        self.has = [w > 0 and n > 1 for w, n in zip(self.weights, shape[-3:])]
        self.ring = bool(term is not None and len(shape) > 0 and shape[-1] > 1 and term.wraps(f))
        self.bound = sum(w * w for w, h in zip(self.weights, self.has) if h) if self.iso \
            else sum(self.has)
        self.label = f'IsoTVRegularizer(weights={self.weights!r})' if self.iso \
            else f"SmoothRegularizer(kind='abs', weights={self.weights!r})"

    @property
    def clamps(self):
        return [self.lam * w / self.n_vox for w in self.weights]

    @property
    def radius(self):
        return self.lam / self.n_vox


def _tv_on_volume(who, term, f, x0):
    """The `_TVTerm` of `term` on the volume a solve from `x0` runs on (the grid's, or x0's own
    shape); ValueError where that volume gives the term nothing to act on."""
    shape = tuple(f.grid.shape) if x0 is None else tuple(t.as_tensor(x0).shape)
    tv = _TVTerm(term, f, shape)
    if term is None:
        return tv
    if len(shape) < 3:
        raise ValueError(f'{who} needs a volume with axes (..., r, e, a), not shape {shape}')
    if len(shape) > 3 and not tv.iso and term.time_weight > 0:
        raise ValueError(f"{who}: SmoothRegularizer(kind='abs', time_weight={term.time_weight!r}) "
                         'on a volume with a time axis is not built (time_weight=0 is)')
    if not any(tv.has):
        raise ValueError(f'{who}: {tv.label} has no edges on a volume of shape {shape} (an axis '
                         'needs a weight > 0 and a length > 1)')
    return tv


def _clamp(u, a, b):
    return t.where(u < a, a, t.where(u > b, b, u))


def _start(f, x0, dev, lower, upper):
    """(x_0, lower, upper) of the bounded loops: zeros on the grid (float64, on `dev`) or a copy of
    `x0`, clamped into the bounds, and the bounds as 0-dim tensors beside it."""
    x = t.zeros(tuple(f.grid.shape), dtype=t.float64, device=dev) if x0 is None \
        else t.as_tensor(x0).detach().clone()
    lo, hi = (t.full((), v, dtype=x.dtype, device=x.device) for v in (lower, upper))
    return _clamp(x, lo, hi), lo, hi


def _tv_stage(tv, shape, per_voxel=False):
    """The two volume launches of the direct loops over a volume of `shape` = (nr, ne, na), bound
    once -> (primal, dual):

        primal(x, g, q, x_new, c, tau, lower, upper, part, stream)
        dual(x_new, x, q, sigma, part, stream)

    include/sphrt_pd.h's entries with the has_* flags and the clamps, for the iso term
    include/sphrt_iso.h's with the weights and the radius; `per_voxel`: sphrt_dp_primal_f64 (tau
    one step per voxel: include/sphrt_dp.h; never with the iso term).  Without a TV term the
    primal launch gets zero flags — it never reads q then, but refuses a null or an overlapping
    one — and `dual` launches nothing."""
    from . import _lib
    lib = _lib.load()
    grid = (*shape, int(tv.ring))
    if tv.iso:
        p_name, d_name = 'sphrt_iso_primal_f64', 'sphrt_iso_dual_f64'
        p_axes, d_axes = list(tv.weights), [*tv.weights, tv.radius]
    else:
        p_name = 'sphrt_dp_primal_f64' if per_voxel else 'sphrt_pd_primal_f64'
        d_name = 'sphrt_pd_dual_f64'
        p_axes = [int(h) for h in tv.has]
        d_axes = p_axes + tv.clamps
    p_entry, d_entry = getattr(lib, p_name), getattr(lib, d_name)

    def primal(x, g, q, x_new, c, tau, lower, upper, part, stream):
        _lib.check(p_entry(_lib.ptr(x), _lib.ptr(g), _lib.ptr(q), _lib.ptr(x_new), *grid, *p_axes,
                           c, _lib.ptr(tau), lower, upper, _lib.ptr(part), stream), p_name)

    def dual(x_new, x, q, sigma, part, stream):
        if tv.term is not None:
            _lib.check(d_entry(_lib.ptr(x_new), _lib.ptr(x), _lib.ptr(q), *grid, *d_axes,
                               _lib.ptr(sigma), _lib.ptr(part), stream), d_name)
    return primal, dual


def _pd_steps(L, dual_ratio, n_axes):
    """(tau, sigma) as one-element tensors beside L: 1 / ((1 + ratio) L) and ratio L / B with
    B = 4 n_axes (`_TVTerm.bound`); both 0 when L is not > 0 (`_fista_step`'s rule for its step)."""
    zero = t.zeros_like(L)
    tau = t.where(L > 0, 1.0 / ((1.0 + dual_ratio) * L), zero)
    sigma = t.where(L > 0, (dual_ratio * L) / (4.0 * n_axes), zero)
    return tau, sigma


def _change_history(mm, ref):
    """[sqrt(MM_k / ref)], 0.0 where MM_k is exactly 0 (NaN where the reference is not > 0)."""
    return [0.0 if v == 0 else math.sqrt(v / ref) if ref > 0 else float('nan') for v in mm]


def _pd_info(mm, qq, L, tau, sigma, q, ref=None):
    """`primal_dual`'s info from MM_k and QQ_k (k = 0 .. K - 1) and the steps, on the host (`ref`:
    the MM the primal changes are relative to, MM_0 unless given)."""
    if ref is None:
        ref = mm[0] if mm else 0.0
    return {'primal_change': _change_history(mm, ref),
            'dual_change': [math.sqrt(v) if v >= 0 else float('nan') for v in qq],
            'lipschitz': L, 'tau': tau, 'sigma': sigma, 'dual': q}


def _tv_maps(tv, x):
    """The TV term's two maps in plain torch (narrow / roll differences) over the r, e, a axes of
    every slice of volumes like `x`, for `_primal_dual_generic` and `_chambolle_pock_generic`: the
    specification of the launches of include/sphrt_pd.h and include/sphrt_iso.h and the CPU path
    -> (adjoint, dual).  adjoint(q) = Dw^T q and dual(q, xb, sigma) = the dual step from
    v = q + sigma Dw xb, a new tensor, with Dw_ax = w_ax D_ax.  kind='abs': w = 1 (no multiply;
    an alpha of 1.0 is exact) and v_ax clamped to +-c_ax; the iso term: each voxel's triple v
    projected onto the ball of radius lam / V (v itself where its norm is not greater; a slot
    without an edge holds +0.0 and adds nothing to the norm)."""
    has, wts = tv.has, tv.weights if tv.iso else (1.0, 1.0, 1.0)
    cax = [t.full((), c, dtype=x.dtype, device=x.device) for c in tv.clamps]
    radius = t.full((), tv.radius, dtype=x.dtype, device=x.device)

    def edges(v, ax):
        """The views (lower voxels, upper voxels) of `v` along axis ax, or None for the ring
        (every voxel has its edge: roll)."""
        if ax == 2 and tv.ring:
            return None
        n = v.shape[ax - 3]
        return v.narrow(ax - 3, 0, n - 1), v.narrow(ax - 3, 1, n - 1)

    def adjoint(q):
        s = t.zeros_like(q[0])     # Dw^T q: the arriving edge, then the leaving one
        for ax in range(3):
            if not has[ax]:
                continue
            if edges(s, ax) is None:
                s.add_(t.roll(q[ax], 1, -1), alpha=wts[ax])
                s.sub_(q[ax], alpha=wts[ax])
            else:
                edges(s, ax)[1].add_(edges(q[ax], ax)[0], alpha=wts[ax])
                edges(s, ax)[0].sub_(edges(q[ax], ax)[0], alpha=wts[ax])
        return s

    def project(v):
        n2 = t.zeros_like(v[0])
        for ax in range(3):
            if has[ax]:
                n2 = n2 + v[ax] * v[ax]
        nrm = t.sqrt(n2)
        outside = nrm > radius
        scale = radius / t.where(outside, nrm, t.ones_like(nrm))
        return t.where(outside, v * scale, v)

    def dual(q, xb, sigma):
        v = q.clone()
        for ax in range(3):
            if not has[ax]:
                continue
            if edges(xb, ax) is None:
                d, q_ax, slot = t.roll(xb, -1, -1) - xb, q[ax], v[ax]
            else:
                below, above = edges(xb, ax)
                d, q_ax, slot = above - below, edges(q[ax], ax)[0], edges(v[ax], ax)[0]
            step = t.addcmul(q_ax, wts[ax] * d if tv.iso else d, sigma)
            slot.copy_(step if tv.iso else _clamp(step, -cax[ax], cax[ax]))
        return project(v) if tv.iso else v
    return adjoint, dual


def _primal_dual_generic(f, y, sq, smooth, tv, x0, num_iterations, damp, lower, upper, lipschitz,
                         power_iterations, dual_ratio, bar):
    """`primal_dual` in plain torch, through f(x) and f._apply_adjoint alone: the specification
    of `_primal_dual_direct` (narrow / roll differences, sums in torch's order) and what runs on
    the CPU.  Every scalar stays a tensor on the device: no sync inside the loop."""
    with t.no_grad():
        yd = y.detach()
        x, lo, hi = _start(f, x0, yd.device, lower, upper)
        c = 2 * damp / x.numel()
        normal = _normal_generic(f, yd, sq, smooth, x)
        tv_adjoint, tv_dual = _tv_maps(tv, x)
        L, _ = _fista_step(lambda v: t.add(normal(v, None), v, alpha=c), x, lipschitz,
                           power_iterations)
        tau, sigma = _pd_steps(L, dual_ratio, tv.bound)
        q = x.new_zeros((3,) + tuple(x.shape))
        mms, qqs = [], []
        try:
            for _ in bar:
                gp = t.add(normal(x, yd), x, alpha=c)
                x_new = _clamp(t.addcmul(x, gp + tv_adjoint(q), -tau), lo, hi)
                q_new = tv_dual(q, 2 * x_new - x, sigma)
                mms.append(((x_new - x) ** 2).sum())
                qqs.append(((q_new - q) ** 2).sum())
                x, q = x_new, q_new
        except KeyboardInterrupt:
            pass
        y_hat = f(x)
        done = len(mms)
        host = t.cat([t.stack(mms + qqs).to(t.float64) if done else L.new_zeros(0).to(t.float64),
                      L.to(t.float64), tau.to(t.float64), sigma.to(t.float64)]).cpu().tolist()
    return x, y_hat, _pd_info(host[:done], host[done:2 * done], *host[-3:], q)


def _primal_dual_direct(f, y, sq, smooth, tv, x0, num_iterations, damp, lower, upper, lipschitz,
                        power_iterations, dual_ratio, bar):
    """`primal_dual` on the operator's own entries (`_cg_is_direct`).  An iteration is g = N x - b
    without the damping term (`_normal_direct` against y: over a MatrixFreeOperator one trace,
    over an Operator its forward, residual and adjoint launches; the smooth launch with a square
    smooth term) followed by the two launches of include/sphrt_pd.h: sphrt_pd_primal_f64 (the
    damping term, D^T q, the step, the clamp into the other of two x buffers, partial sums of
    MM) and sphrt_pd_dual_f64 (2 x+ - x on the fly, the dual step and clamp in place, partial
    sums of QQ).  tau and sigma are one-element device tensors the launches read through
    pointers — L comes from the power method in torch over the same application — so nothing is
    read back before the loop ends; MM_k and QQ_k are then one row of partial sums each per
    iteration (`_kernel_sum`).  Ctrl-C ends the loop after the last iteration whose dual launch
    went out: the x returned and info['dual'] are always the pair of one iteration."""
    from . import _lib
    dev, f64 = f._cdev, t.float64
    with t.no_grad(), t.cuda.device(dev):
        x, _, _ = _start(f, x0, dev, lower, upper)
        c = 2 * damp / x.numel()
        primal, dual = _tv_stage(tv, x.shape)
        apply, pn = _normal_direct(f, y, sq, smooth, x)
        L, _ = _fista_step(lambda v: t.add(apply(v), v, alpha=c), x, lipschitz, power_iterations)
        tau, sigma = _pd_steps(L, dual_ratio, tv.bound)
        x_new = t.empty_like(x)
        q = t.zeros((3,) + tuple(x.shape), dtype=f64, device=dev)
        rows = max(num_iterations, 1)
        part_mm = t.empty((rows, pn), dtype=f64, device=dev)
        part_qq = t.empty((rows, pn), dtype=f64, device=dev)
        # (done: iterations whose x is current; dual_out: the iteration whose dual launch, the
        # only writer of q, has gone out)
        done, dual_out = 0, -1
        try:
            for it in bar:
                g = apply(x, True)
                stream = _lib.stream_of(dev)
                primal(x, g, q, x_new, c, tau, lower, upper, part_mm[it], stream)
                dual(x_new, x, q, sigma, part_qq[it], stream)
                dual_out = it
                x, x_new, done = x_new, x, it + 1      # (one statement: not separable)
        except KeyboardInterrupt:
            # Ctrl-C inside an iteration: before its dual launch q is still the q of x (the
            # iteration is dropped); after it, q is one step ahead, and so is x_new: finish
            # the iteration, so that the x returned and info['dual'] belong together
            if dual_out == done:
                x, x_new, done = x_new, x, done + 1
        y_hat = f(x)       # (goes out before the readback waits)
        sums = _kernel_sum(t.cat([part_mm[:done], part_qq[:done]])) if done else L.new_zeros(0)
        host = t.cat([sums, L, tau, sigma]).cpu().tolist()
    return x, y_hat, _pd_info(host[:done], host[done:2 * done], *host[-3:], q)


# ---- robust and Poisson fidelity with TV and bounds: Chambolle-Pock ---------------------------------

# sigma = dual_ratio * (lam / M) / |K|: the ratio tools/cp_study.py chose (DESIGN §5,
# "Chambolle-Pock solver").
_CP_DUAL_RATIO = 1.0


def chambolle_pock(f, y, loss_fns, x0=None, num_iterations=100, damp=0.0, lower=0.0, upper=None,
                   norm=None, power_iterations=_FISTA_POWER_ITERATIONS,
                   dual_ratio=_CP_DUAL_RATIO, progress_bar=False, precondition=None):
    """Minimise, subject to lower <= x <= upper elementwise,

        J(x) = sum_i phi_i((A x)_i) + damp * mean(x^2) + lam_tv * SmoothRegularizer(kind='abs')(x)

    by the primal-dual hybrid gradient of Chambolle and Pock in Condat's form, the fidelity term
    dualised as `primal_dual` dualises the TV term -> (x, f(x), info).  No Lipschitz constant of
    the fidelity is needed, only the proximal map of its conjugate, which is closed-form and
    elementwise over the rays for all four fidelity classes.

    `loss_fns`: exactly one fidelity term, of exact type SquareLoss, AbsLoss, HuberLoss or
    PoissonLoss (a finite scalar lam > 0, unit volume_mask, a projection_mask that is 1 or a tensor
    `gd`'s direct loop would weigh the residual with; its entries must be >= 0, which is not
    checked — reading the mask back would synchronise the host — and a negative entry turns that
    ray's clamp interval inside out: the result is then meaningless), and at most one
    SmoothRegularizer(kind='abs') under `primal_dual`'s rules for it (on a volume with a time axis
    its time_weight must be 0).  `lower`, `upper`, `power_iterations`, `damp` and `num_iterations`
    as `fista` takes them; `norm`: the caller's own |A|^2, a finite number > 0, as `lipschitz=` is
    for `fista`; `dual_ratio`: a finite number > 0.  Anything else raises ValueError naming the
    offender, before the operator is touched.

    With M = y.numel(), V = x.numel(), s_i = lam w_i / M and z = A x, phi_i(z) is what the loss
    classes compute: s (z - y)^2, s |z - y|, s huber_delta(z - y) (torch's), s (z - y log(z +
    eps)).  `y` is not checked for sign: a negative count under PoissonLoss gives what IEEE gives
    (a negative discriminant: NaN).  A ray that misses the grid has (A x)_i = 0 whatever x is;
    under PoissonLoss a positive count on it (background) leaves its dual heading for -s_i y_i /
    eps, which no iteration count reaches: x is unaffected, but info['ray_dual'] and a duality
    gap formed from it mean nothing on such rays.  Give them weight 0 in the projection_mask
    (then p_i = +0.0 and the ray leaves the total).  State: x, the ray dual p (the shape of y), the TV dual q (as
    in `primal_dual`) and z.  With c = 2 damp / V, iteration k is

        g  = A^T p
        x+ = clamp(fma(-tau, fma(c, x, g) + D^T q, x))             (sphrt_pd_primal_f64)
        q  <- clamp(fma(sigma, D(2 x+ - x), q), +-c_ax)            (sphrt_pd_dual_f64; with TV)
        z+ = A x+
        p  <- prox_{sigma phi*}(a),  a = fma(sigma, fma(2, z+, -z), p)   (sphrt_cp_ray_dual_f64)

    and with t = a - sigma y the prox is: abs clamp(t, +-s); huber clamp(t / (1 + sigma / s),
    +-s delta); square t / (1 + sigma / (2 s)); poisson, with a' = a + sigma eps,
    min(s, ((a' + s) - sqrt((a' - s)^2 + 4 sigma s y)) / 2); a ray with s_i = 0 always gets +0.0.

    Steps: Kn^2 = L_A + B, L_A an upper estimate of |A|^2 (`fista`'s power method and margin on
    v -> A^T(A v), or `norm`), B = 4 (number of TV axes with edges), 0 without TV; with sbar =
    lam / M, sigma = dual_ratio sbar / Kn and 1 / tau = sigma Kn^2 + c (Condat's condition
    1 / tau - sigma |K|^2 >= c / 2; both 0 when Kn is not > 0).

    info = {'primal_change': [sqrt(MM_k / MM_ref)] (as `primal_dual`, but MM_ref is the first MM_k
    that is not zero: from p_0 = 0 the first step moves x only through the damping term),
    'dual_change': [sqrt(QQ_k)] (zeros without TV), 'ray_dual_change': [sqrt(sum (p+ - p)^2)], 'fidelity': [sum_i phi_i(z+_i)],
    'norm': L_A, 'tau', 'sigma', 'dual': q or None without TV, 'ray_dual': p}.  Every iterate
    satisfies the bounds exactly, and so do the duals: |q_ax| <= c_ax, |p_i| <= s_i (abs),
    |p_i| <= s_i delta (huber), p_i <= s_i (poisson), each clamp storing the bound's own bits.
    There is no tolerance and no early exit.

    `precondition`: None (the scalar steps above) or 'diagonal': the steps of Pock and Chambolle
    (2011), Lemma 2 with alpha = 1, for K = [A; D], one per voxel and one per ray.  A >= 0
    entrywise, so |K|'s sums are plain sums: row_i = (A 1)_i and col_j = (A^T 1)_j (one forward and
    one adjoint of ones: no power method, `power_iterations` is ignored and a given `norm` raises
    ValueError), deg_j the number of TV edges at voxel j (0 .. 6; every edge row of |D| sums to
    2).  With rho = dual_ratio sbar:

        sigma_i = rho / row_i          (+0.0 where row_i is not > 0: the ray misses the grid and
                                        its dual never moves)
        sigma_tv = rho / 2
        tau_j = 1 / fma(rho, col_j + deg_j, c)    (+0.0 where that is not > 0: no ray, no edge
                                                   and no damping act on the voxel; it stays put)

    and the iteration above runs with tau_j, sigma_tv and sigma_i in place of tau, sigma (TV) and
    sigma (rays): sphrt_dp_primal_f64, sphrt_pd_dual_f64, sphrt_dp_ray_dual_f64
    (include/sphrt_dp.h).  With T = diag(tau), S = diag(sigma_i, sigma_tv), the lemma gives
    |S^(1/2) K T^(1/2)| <= 1 for every rho (rho cancels), and, beyond it, T^-1 - K^T S K >= c I:
    Condat's condition with the damping term's Lipschitz constant c.  info['tau'] is then a tensor
    of x's shape, info['sigma'] one of y's shape (geometry order), info['sigma_tv'] a float and
    info['norm'] None; the histories keep their meaning.  Whether it pays depends on the problem:
    README and DESIGN section 8 record the measurement.

    Isotropic TV: one IsoTVRegularizer may stand in place of the abs term, under `primal_dual`'s
    rules for it and with its dual step (the projection of each voxel's triple onto the ball of
    radius lam_tv / V; sphrt_iso_primal_f64 and sphrt_iso_dual_f64 in place of the two launches
    of sphrt_pd.h); B = 4 sum of w_ax^2 over the axes with edges in Kn^2.  info['dual'] then has
    shape (3,) + x.shape and certifies with |q_i|_2 <= r up to sum_ax q_ax^2 <= r^2 (1 + 12 *
    2^-53).  precondition='diagonal' with it raises ValueError: the lemma's per-row steps do not
    fit a prox that couples three rows.

    The inputs `cg` runs directly (`_cg_is_direct`) run `_chambolle_pock_direct`: the operator's
    own launches and three csrc/loss.hip launches per iteration (two without TV), the whole solve
    enqueued without a host sync and bitwise reproducible where the adjoint is.  Over a
    MatrixFreeOperator an iteration is two traces (the forward and the back-projection: the
    prox sits between them), not `primal_dual`'s one.  Everything else — CPU tensors, dynamic
    operators, other dtypes, a non-contiguous x0 — runs the same algorithm in plain torch
    (`_chambolle_pock_generic`)."""
    who = 'chambolle_pock'
    fid, term = _cp_terms(y, loss_fns, damp, num_iterations, who)
    bounds = _fista_args(lower, upper, None, power_iterations, who=who)
    if norm is not None and (not _number(norm) or not 0 < norm < math.inf):
        raise ValueError(f'{who} needs a finite norm > 0 (or None), not {norm!r}')
    if not _number(dual_ratio) or not 0 < dual_ratio < math.inf:
        raise ValueError(f'{who} needs a finite dual_ratio > 0, not {dual_ratio!r}')
    if precondition is not None and not (isinstance(precondition, str)
                                         and precondition == 'diagonal'):
        raise ValueError(f"{who} needs precondition None or 'diagonal', not {precondition!r}")
    if precondition is not None and norm is not None:
        raise ValueError(f"{who}: precondition='diagonal' takes its steps from the operator's row "
                         f'and column sums, not from a norm (norm={norm!r})')
    if precondition is not None and type(term) is IsoTVRegularizer:
        raise ValueError(f"{who}: precondition='diagonal' with an IsoTVRegularizer is not built "
                         '(per-row steps do not fit a prox that couples three rows; '
                         "SmoothRegularizer(kind='abs') and precondition=None are)")
    tv = _tv_on_volume(who, term, f, x0)
    bar = _Bar(range(num_iterations), progress_bar)
    run = _chambolle_pock_direct if _cg_is_direct(f, y, x0) else _chambolle_pock_generic
    return run(f, y, fid, tv, x0, num_iterations, float(damp), bounds[0], bounds[1],
               None if norm is None else float(norm), power_iterations, float(dual_ratio), bar,
               diagonal=precondition is not None)


def _cp_terms(y, loss_fns, damp, num_iterations, who):
    """(the fidelity term, the TV term or None) of a total `chambolle_pock` solves; ValueError
    naming what it does not, worded as `_cg_terms` words it."""
    if not isinstance(y, t.Tensor):
        raise ValueError(f'{who} needs measurements y as a tensor, not {type(y).__name__}')
    if not _number(damp) or not 0 <= damp < float('inf'):
        raise ValueError(f'{who} needs a finite damp >= 0, not {damp!r}')
    if isinstance(num_iterations, bool) or not isinstance(num_iterations, int) \
            or num_iterations < 0:
        raise ValueError(f'{who} needs num_iterations as an integer >= 0, not {num_iterations!r}')
    fid = tv = None
    for fn in loss_fns:
        name, tv_iso = type(fn).__name__, type(tv) is IsoTVRegularizer
        if type(fn) in _FIDELITY:
            if fid is not None:
                raise ValueError(f'{who} solves for one fidelity term, not two')
            fid = fn
        elif type(fn) is SmoothRegularizer:
            if fn.smooth_kind != 'abs':
                raise ValueError(f"{who} takes a smooth term as total variation only: "
                                 f"SmoothRegularizer(kind={fn.smooth_kind!r}) is not built "
                                 "(kind='abs' is)")
            if tv_iso:
                raise ValueError(f"{who} solves with at most one TV term: a SmoothRegularizer("
                                 "kind='abs') beside an IsoTVRegularizer is not built")
            if tv is not None:
                raise ValueError(f"{who} solves with at most one SmoothRegularizer(kind='abs'), "
                                 'not two')
            tv = fn
        elif type(fn) is IsoTVRegularizer:
            if tv_iso:
                raise ValueError(f'{who} solves with at most one IsoTVRegularizer, not two')
            if tv is not None:
                raise ValueError(f"{who} solves with at most one TV term: an IsoTVRegularizer "
                                 "beside a SmoothRegularizer(kind='abs') is not built")
            tv = fn
        else:
            raise ValueError(f'{who} needs a total of one SquareLoss, AbsLoss, HuberLoss or '
                             f"PoissonLoss and at most one SmoothRegularizer(kind='abs'): {name} "
                             'is neither (gd takes it)')
        _term_rules(who, fn, name, name, f', not {name}.lam = {fn.lam!r}',
                    rays=y if fn is fid else None)
    if fid is None:
        raise ValueError(f'{who} needs one SquareLoss, AbsLoss, HuberLoss or PoissonLoss among '
                         'loss_fns')
    return fid, tv


def _cp_kind(fid):
    """(kind, delta or eps) of a fidelity term as sphrt_cp_ray_dual_f64 takes them."""
    from . import _lib
    if type(fid) is AbsLoss:
        return _lib.CP_ABS, 0.0
    if type(fid) is HuberLoss:
        return _lib.CP_HUBER, float(fid.delta)
    if type(fid) is PoissonLoss:
        return _lib.CP_POISSON, float(fid.eps)
    return _lib.CP_SQUARE, 0.0


def _cp_prox(kind, par, a, sigma, s, m):
    """prox_{sigma phi*}(a) per ray in plain torch, the operations of include/sphrt_cp.h in its
    order (torch's multiply-adds are not fused): `s` the rays' factors, `m` the measurements,
    `sigma` a one-element tensor, `par` the Huber delta or the Poisson eps."""
    tt = t.addcmul(a, m, -sigma)
    if kind == 0:
        pn = tt / (1.0 + sigma / (2.0 * s))
    elif kind == 1:
        pn = t.where(tt < -s, -s, t.where(tt > s, s, tt))
    elif kind == 2:
        u, b = tt / (1.0 + sigma / s), s * par
        pn = t.where(u < -b, -b, t.where(u > b, b, u))
    else:
        a1 = a + sigma * par
        d, e = a1 - s, a1 + s
        v = 0.5 * (e - t.sqrt(d * d + ((4.0 * sigma) * s) * m))
        pn = t.where(v > s, s, v)
    return t.where(s == 0, t.zeros_like(pn), pn)


def _cp_rho(kind, par, z, m):
    """rho(z, m) per ray, as the loss classes form it."""
    if kind == 0:
        return (z - m) ** 2
    if kind == 1:
        return (z - m).abs()
    if kind == 2:
        return t.nn.functional.huber_loss(z, m, reduction='none', delta=par)
    return z - m * t.log(z + par)


def _cp_steps(LA, n_axes, s_bar, c, dual_ratio):
    """(tau, sigma) as one-element tensors beside L_A: Kn^2 = L_A + 4 n_axes, sigma = ratio
    sbar / Kn, tau = 1 / (sigma Kn^2 + c); both 0 when Kn is not > 0."""
    kn2 = LA + 4.0 * n_axes
    kn, zero = t.sqrt(kn2), t.zeros_like(LA)
    ok = kn > 0
    sigma = t.where(ok, (dual_ratio * s_bar) / kn, zero)
    tau = t.where(ok, 1.0 / (sigma * kn2 + c), zero)
    return tau, sigma


def _cp_info(mm, qq, pp, fid, LA, tau, sigma, q, p):
    """`chambolle_pock`'s info from the per-iteration sums and the steps, on the host."""
    # (p_0 = 0: without damping the first step does not move x, so the reference is the first
    # MM_k that is not zero)
    info = _pd_info(mm, qq, LA, tau, sigma, q, ref=next((v for v in mm if v > 0), 0.0))
    info['norm'] = info.pop('lipschitz')
    info['ray_dual_change'] = [math.sqrt(v) if v >= 0 else float('nan') for v in pp]
    info['fidelity'] = fid
    info['ray_dual'] = p
    return info


def _dp_degree(has, ring, x):
    """deg_j, the number of TV edges at each voxel of the trailing three axes of `x` (has: which
    axes have edges; ring: the azimuth ring is closed) -> a tensor of that shape, 0 .. 6."""
    deg = t.zeros(tuple(x.shape[-3:]), dtype=x.dtype, device=x.device)
    for ax in range(3):
        if not has[ax]:
            continue
        if ax == 2 and ring:
            deg += 2
        else:
            n = deg.shape[ax]
            deg.narrow(ax, 0, n - 1).add_(1)       # the edge leaving the voxel
            deg.narrow(ax, 1, n - 1).add_(1)       # the edge arriving at it
    return deg


def _dp_steps(row, col, deg, rho, c):
    """(tau like col, sigma like row) of the diagonal preconditioning in plain torch:
    1 / (rho (col + deg) + c) and rho / row, +0.0 where a denominator is not > 0."""
    d = rho * (col + deg) + c
    tau = t.where(d > 0, 1.0 / d, t.zeros_like(d))
    sigma = t.where(row > 0, rho / row, t.zeros_like(row))
    return tau, sigma


def _dp_info(info, tau, sigma, sigma_tv):
    """`chambolle_pock`'s info with the steps of the diagonal preconditioning."""
    info.update(norm=None, tau=tau, sigma=sigma, sigma_tv=sigma_tv)
    return info


def _chambolle_pock_generic(f, y, fid, tv, x0, num_iterations, damp, lower, upper, norm,
                            power_iterations, dual_ratio, bar, diagonal=False):
    """`chambolle_pock` in plain torch, through f(x) and f._apply_adjoint alone: the
    specification of `_chambolle_pock_direct` (sums in torch's order) and what runs on the CPU.
    Every scalar stays a tensor on the device: no sync inside the loop."""
    with t.no_grad():
        yd = y.detach()
        x, lo, hi = _start(f, x0, yd.device, lower, upper)
        dshape, dtype, dev = tuple(x.shape), x.dtype, x.device
        pdt = t.promote_types(yd.dtype, dtype)
        m = yd.to(pdt)
        n_vox, n_meas = x.numel(), yd.numel()
        c = 2 * damp / n_vox
        kind, par = _cp_kind(fid)
        s_bar = fid.lam / n_meas
        w = None if _unit(fid.projection_mask) else \
            fid.projection_mask.detach().to(pdt).expand(yd.shape)
        s = t.full_like(m, s_bar) if w is None else s_bar * w
        with_tv = tv.term is not None
        tv_adjoint, tv_dual = _tv_maps(tv, x)
        if diagonal:
            # row and column sums of A >= 0: one forward and one adjoint of ones
            rho_s = dual_ratio * s_bar
            row = f(t.ones_like(x)).to(pdt)
            col = f._apply_adjoint(t.ones_like(m), dshape, dtype, dev)
            deg = _dp_degree(tv.has, tv.ring, x) if with_tv else 0.0
            tau, sigma = _dp_steps(row, col, deg, rho_s, c)
            sigma_tv = t.full((), rho_s / 2, dtype=dtype, device=dev)
            LA = t.zeros(1, dtype=dtype, device=dev)
        else:
            # |A|^2: v -> A^T(A v) is `_normal_generic` of a SquareLoss whose factor 2 lam / M is 1
            ata = _normal_generic(f, yd, SquareLoss(lam=n_meas / 2), None, x)
            LA, _ = _fista_step(lambda v: ata(v, None), x, norm, power_iterations)
            tau, sigma = _cp_steps(LA, tv.bound, s_bar, c, dual_ratio)
            sigma_tv = sigma
        q = x.new_zeros((3,) + dshape) if with_tv else None
        z = f(x)
        p = t.zeros_like(m)
        mms, qqs, pps, fids, done = [], [], [], [], 0
        try:
            for _ in bar:
                g = f._apply_adjoint(p, dshape, dtype, dev)
                gp = t.add(g, x, alpha=c)
                if with_tv:
                    gp = gp + tv_adjoint(q)
                x_new = _clamp(t.addcmul(x, gp, -tau), lo, hi)
                q_new = tv_dual(q, 2 * x_new - x, sigma_tv) if with_tv else None
                z_new = f(x_new)
                p_new = _cp_prox(kind, par, t.addcmul(p, 2 * z_new - z, sigma), sigma, s, m)
                rho = _cp_rho(kind, par, z_new.to(pdt), m)
                fids.append(s_bar * (rho if w is None else w * rho).sum())
                mms.append(((x_new - x) ** 2).sum())
                pps.append(((p_new - p) ** 2).sum())
                if with_tv:
                    qqs.append(((q_new - q) ** 2).sum())
                x, z, p, q, done = x_new, z_new, p_new, q_new, done + 1
        except KeyboardInterrupt:
            pass
        for sums in (mms, qqs, pps, fids):      # (Ctrl-C: the sums of an iteration not kept)
            del sums[done:]
        y_hat = f(x)
        if not with_tv:
            qqs = [LA.new_zeros(()) for _ in range(done)]
        sums = t.stack(mms + qqs + pps + fids).to(t.float64) if done \
            else LA.new_zeros(0).to(t.float64)
        if diagonal:
            host = sums.cpu().tolist()
            return x, y_hat, _dp_info(
                _cp_info(*(host[k * done:(k + 1) * done] for k in range(4)), None, None, None, q,
                         p), tau, sigma, float(sigma_tv))
        host = t.cat([sums, LA.to(t.float64), tau.to(t.float64),
                      sigma.to(t.float64)]).cpu().tolist()
    return x, y_hat, _cp_info(*(host[k * done:(k + 1) * done] for k in range(4)), *host[-3:], q, p)


def _chambolle_pock_direct(f, y, fid, tv, x0, num_iterations, damp, lower, upper, norm,
                           power_iterations, dual_ratio, bar, diagonal=False):
    """`chambolle_pock` on the operator's own entries (`_cg_is_direct`).  An iteration is
    g = A^T p — over an Operator its adjoint on the dual in the adjoint's order, over a
    MatrixFreeOperator the atomic back-projection, or with `deterministic` set
    `_backproject_fixed_into` — then sphrt_pd_primal_f64 (the damping term, D^T q, the step, the
    clamp into the other of two x buffers, partial sums of MM), with a TV term sphrt_pd_dual_f64,
    the forward z+ = A x+ into the other of two z buffers (the loop's forward, or
    `_forward_into`: a second trace) and sphrt_cp_ray_dual_f64 (include/sphrt_cp.h: the ray
    dual's prox in place, its copy in the adjoint's order, partial sums of its change and of the
    fidelity).  Measurements, weights and the ray order over an Operator are arranged as
    `_normal_direct` arranges them (`_fidelity_stage`); p lives in the order the loop's
    forward writes and info['ray_dual'] is put back into geometry order at the end.  tau and
    sigma are one-element device tensors the launches read through pointers — L_A comes from the
    power method in torch over `_normal_direct`'s application of A^T A — so nothing is read back
    before the loop ends; the histories are then rows of partial sums (`_kernel_sum`).  Ctrl-C
    inside an iteration drops it if nothing was written in place yet, and otherwise sends out
    its remaining steps, so that the x, q and p returned are those of one iteration — with the
    care `_primal_dual_direct` takes and its one gap: an interrupt that lands between the return
    of an in-place launch and the `stage += 1` after it is not seen as that launch (counting
    first instead would lose the launch itself to an interrupt during its argument list, a
    longer stretch of bytecode).

    `diagonal` (precondition='diagonal'): no power method; row = A 1 (geometry order) and
    col = A^T 1 come from one forward and one adjoint of ones on the same launches, and one
    sphrt_dp_steps_f64 launch (include/sphrt_dp.h) writes tau per voxel and sigma per ray — in the
    order the loop's forward writes, through the trace-position list where that differs — from
    the host numbers rho and c.  The iteration then launches sphrt_dp_primal_f64 and
    sphrt_dp_ray_dual_f64 where the scalar one launches sphrt_pd_primal_f64 and
    sphrt_cp_ray_dual_f64, and sphrt_pd_dual_f64 reads sigma_tv = rho / 2 from a device scalar:
    the same count of launches, 8 bytes more per voxel and per ray."""
    from . import _lib
    from .raytracer import MatrixFreeOperator
    lib = _lib.load()
    dev, f64 = f._cdev, t.float64
    fused = isinstance(f, MatrixFreeOperator)
    with t.no_grad(), t.cuda.device(dev):
        x, _, _ = _start(f, x0, dev, lower, upper)
        dshape = tuple(x.shape)
        n_vox = x.numel()
        with_tv = tv.term is not None
        c = 2 * damp / n_vox
        kind, par = _cp_kind(fid)
        # (the ray dual's factors: s = s_bar w, arrays for every term; p lives in y_ray's order)
        fs = _fidelity_stage(f, y, fid, gradient=False)
        yd, n_meas, s_bar, y_f64 = fs.yd, fs.n_meas, fs.c, fs.y_f64
        y_ray, w_ray, s_ray = fs.y_res, fs.w_res, fs.s_res
        order, res_order, loop_desc, positions = fs.order, fs.res_order, fs.loop_desc, fs.positions
        fixed = fs.fixed[0] if fs.fixed else None
        if diagonal:
            pn = lib.sphrt_loss_partials(n_vox)
            LA = t.zeros(1, dtype=f64, device=dev)
        else:
            # |A|^2 on the operator's own launches: `_normal_direct` of a SquareLoss whose factor
            # 2 lam / M is 1 applies v -> A^T(A v)
            ata, pn = _normal_direct(f, y, SquareLoss(lam=n_meas / 2), None, x)
            LA, _ = _fista_step(ata, x, norm, power_iterations)
            del ata
            tau, sigma = _cp_steps(LA, tv.bound, s_bar, c, dual_ratio)
            sigma_tv = sigma
        ps = lib.sphrt_loss_partials(n_meas)
        g_buf = t.empty_like(x) if fused else None
        z, z_new = (t.empty(n_meas, dtype=f64, device=dev) for _ in range(2))
        p = t.zeros(n_meas, dtype=f64, device=dev)
        p_adj = t.zeros(n_meas, dtype=f64, device=dev) if res_order is not None else None

        def forward(d, out):
            """A d in the loop's ray order -> the buffer that holds it."""
            if fused:
                f._forward_into(d, out)
            elif loop_desc is not None:
                f._forward_staged(d, out, loop_desc)
            else:
                return f(d).reshape(-1)
            return out

        def adjoint(v=None):
            """A^T p (or A^T v, v in the adjoint's order) -> a buffer the next application may
            overwrite."""
            if not fused:
                if v is None:
                    v = p if p_adj is None else p_adj
                return f._apply_adjoint(v.view(yd.shape), dshape, f64, dev,
                                        trace_order=order is not None)
            v = p if v is None else v
            if fixed is None:
                return f._apply_adjoint(v.view(yd.shape), dshape, f64, dev)
            f._backproject_fixed_into(v, g_buf, fixed)
            return g_buf

        if diagonal:
            # (ones are ones in every ray order; row in geometry order, sigma where the loop's
            # forward writes)
            rho = dual_ratio * s_bar
            row = f(t.ones_like(x)).reshape(-1)
            col = adjoint(t.ones(n_meas, dtype=f64, device=dev))
            tau, sigma = t.empty_like(x), t.empty(n_meas, dtype=f64, device=dev)
            _lib.check(lib.sphrt_dp_steps_f64(
                _lib.ptr(col), _lib.ptr(row), n_meas, *dshape, int(tv.ring),
                *(int(h) for h in tv.has), rho, c,
                _lib.ptr(order if positions else None), _lib.ptr(tau), _lib.ptr(sigma),
                _lib.stream_of(dev)), 'sphrt_dp_steps_f64')
            del row, col
            sigma_tv = t.full((1,), rho / 2, dtype=f64, device=dev)
        primal, tv_dual = _tv_stage(tv, dshape, per_voxel=diagonal)
        ray_dual_name = 'sphrt_dp_ray_dual_f64' if diagonal else 'sphrt_cp_ray_dual_f64'
        ray_dual = getattr(lib, ray_dual_name)
        x_new = t.empty_like(x)
        # (without TV the primal launch never reads q, but wants the buffer: it stays, untouched)
        q = t.zeros((3,) + dshape, dtype=f64, device=dev)
        rows = max(num_iterations, 1)
        part_mm = t.empty((rows, pn), dtype=f64, device=dev)
        part_qq = t.zeros((rows, pn), dtype=f64, device=dev)
        part_pp = t.empty((rows, ps), dtype=f64, device=dev)
        part_fid = t.empty((rows, ps), dtype=f64, device=dev)
        z = forward(x, z)
        # (done: iterations whose x, z, q and p are current; stage: how many of the next
        # iteration's four steps have gone out — the second and the fourth write q and p in place)
        done, stage, zn = 0, 0, None

        def advance(it):
            """The steps of iteration `it` that have not gone out yet, in order."""
            nonlocal stage, zn
            while stage < 4:
                stream = _lib.stream_of(dev)
                if stage == 0:
                    g = adjoint()
                    primal(x, g, q, x_new, c, tau, lower, upper, part_mm[it], stream)
                elif stage == 1:
                    tv_dual(x_new, x, q, sigma_tv, part_qq[it], stream)
                elif stage == 2:
                    zn = forward(x_new, z_new)
                else:
                    _lib.check(ray_dual(
                        _lib.ptr(zn), _lib.ptr(z), _lib.ptr(y_ray), y_f64, n_meas, kind, par,
                        _lib.ptr(s_ray), _lib.ptr(w_ray), _lib.ptr(sigma), _lib.ptr(res_order),
                        _lib.ptr(p), _lib.ptr(p_adj), _lib.ptr(part_pp[it]),
                        _lib.ptr(part_fid[it]), stream), ray_dual_name)
                stage += 1

        try:
            for it in bar:
                advance(it)
                x, x_new, z, z_new, done, stage = x_new, x, zn, z, it + 1, 0   # (one statement)
        except KeyboardInterrupt:
            # Ctrl-C inside an iteration: before its TV-dual launch (without TV: its ray-dual
            # launch) nothing has been written in place, and the iteration is dropped; after it,
            # q (or p) is one step ahead of x: the remaining steps go out, so that the x, q and p
            # returned belong to one iteration
            if done < num_iterations and stage >= (2 if with_tv else 4):
                advance(done)
                x, x_new, z, z_new, done, stage = x_new, x, zn, z, done + 1, 0
        y_hat = f(x)       # (goes out before the readback waits)
        if done:
            sums = t.cat([_kernel_sum(t.cat([part_mm[:done], part_qq[:done]])),
                          _kernel_sum(t.cat([part_pp[:done], part_fid[:done]]))])
        else:
            sums = LA.new_zeros(0)
        host = t.cat([sums, LA] + ([] if diagonal else [tau, sigma])).cpu().tolist()
        if positions:      # (trace positions back to geometry rays)
            p = t.empty_like(p).index_copy_(0, f._ray_id_long(), p)
            if diagonal:
                sigma = t.empty_like(sigma).index_copy_(0, f._ray_id_long(), sigma)
        fids = [s_bar * v for v in host[3 * done:4 * done]]
        if diagonal:
            return x, y_hat, _dp_info(
                _cp_info(host[:done], host[done:2 * done], host[2 * done:3 * done], fids, None,
                         None, None, q if with_tv else None, p.view(yd.shape)),
                tau, sigma.view(yd.shape), rho / 2)
    return x, y_hat, _cp_info(host[:done], host[done:2 * done], host[2 * done:3 * done], fids,
                              *host[-3:], q if with_tv else None, p.view(yd.shape))
