// loss.hip — the elementwise tails of the static_retrieval.py loop (retrieval._gd_direct), fused.
//
// SquareLoss (loss.py:87-110 of the reference: lam * mean((y - f(d))^2)) and NegRegularizer
// (loss.py:140-162: lam * mean(|clamp(d, max=0)|)) need, per iteration, the residual, its scaled
// copy (the adjoint's input) and its mean square (the loss value) and, for the regulariser, the
// mean absolute negative part and -lam/N on the gradient of every negative voxel.  Through torch
// that is ~9 elementwise launches plus two mean reductions (a memset and a reduce each) of
// 5-9 us on a 64^3 problem; here it is two launches, each leaving its workgroups' partial sums
// of the loss (summed for every iteration at once after the loop).  The residual launch is one
// kernel, residual_kernel, for every fidelity term — a masked SquareLoss, AbsLoss, HuberLoss and
// PoissonLoss beside the plain one: a term is a small policy struct (SqFid .. PoissonFid) that
// gives the adjoint's input and the loss's share per ray, its penalty from the rho_* helpers the
// ray dual below shares, behind the four C entries and one host helper (residual_launch).
//
// The elementwise values are single IEEE operations, the ones torch's elementwise ops give (the
// library is built with -ffp-contract=off), so the gradient and hence the iterates stay bitwise
// those of the autograd loop.  The means are deterministic (fixed per-thread strides, a fixed
// reduction tree, the partials summed in a fixed order) but their order differs from
// torch.mean's: loss values agree with it to rounding (~1e-16).
//
// The vector side of retrieval.cg's iteration (two dot products, alpha, beta, three updates) is
// here too, as three launches of the same shape that pass their scalars through partial sums.
// So is the vector side of retrieval.fista's (step, clamp, restart, momentum), as two launches,
// and that of retrieval.primal_dual's (primal step and clamp, dual step and clamp), as two more.
// retrieval.chambolle_pock adds the ray side: one launch for the fidelity's dual (sphrt_cp.h),
// and its diagonal preconditioning the same two with a step per element and the launch that forms
// those steps (sphrt_dp.h).
#include "common.hpp"
#include "stage.hpp"
#include "sphrt_pd.h"
#include "sphrt_cp.h"
#include "sphrt_dp.h"
#include "sphrt_iso.h"

namespace sphrt {

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 1024;   // (a 64^3 volume: one element per thread)

// Workgroup sum in a fixed order (wave shuffles, then the four wave totals in order); thread 0
// stores it.  No cross-workgroup step: the partials of every iteration are summed after the loop
// (deterministic; a last-workgroup reduction would need an agent-scope release per workgroup,
// i.e. an L2 write-back on a chip of eight L2s: +6 us per launch at C5).
__device__ __forceinline__ void block_partial(double v, double* out) {
    __shared__ double sh[kLossThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < kLossThreads / 64; ++i) s += sh[i];
        out[blockIdx.x] = s;
    }
}

// The per-ray penalty rho of the fidelity terms, written once: the residual policies below and
// cp_ray_dual_kernel both call these, so their sums are op for op the same.
// Square: r * r.  Abs: |r|.  Huber (delta > 0): with z = |r|, z < delta ? (0.5 * z) * z :
// delta * (z - 0.5 * delta) — torch's huber_loss forward, operation by operation (a NaN residual
// fails the compare and stays NaN).  Poisson: p - m * log(q) with q = p + eps formed by the caller
// (one rounding) — torch's poisson_nll_loss forward, the device's log; no guards: q <= 0 gives
// NaN or -+inf as in torch.
__device__ __forceinline__ double rho_square(double r) { return r * r; }
__device__ __forceinline__ double rho_abs(double r) { return __builtin_fabs(r); }
__device__ __forceinline__ double rho_huber(double r, double delta) {
    const double z = __builtin_fabs(r);
    return z < delta ? (0.5 * z) * z : delta * (z - 0.5 * delta);
}
__device__ __forceinline__ double rho_poisson(double p, double q, double m) {
#pragma clang fp contract(off)
    const double t = m * log(q);
    return p - t;
}

// A fidelity term as residual_kernel sees it: at(p, m, i, term) returns the adjoint's input for
// the forward value p and the measurement m of ray i and leaves the ray's share of the loss in
// `term`; null() is the host's refusal of a missing per-ray array.
//   SqFid      SquareLoss, lam * mean((y - f(d))^2): r * scale, and r * r.
//   WsqFid     SquareLoss(projection_mask=w): r * ray_scale[i], and weight[i] * (r * r) — two
//              roundings, the order torch's mask * (y - f)**2 takes.
//   RobustFid  AbsLoss (delta == 0) and HuberLoss (delta > 0): psi(r) * ray_scale[i] (robust_psi,
//              common.hpp: the sign of r, or r clamped to +-delta), and weight[i] * rho(r).
//   PoissonFid PoissonLoss, lam * mean(w * (p - y * log(p + eps))): with q = p + eps,
//              ray_scale[i] + ((-ray_scale[i]) * m) / q (poisson_weight, common.hpp: autograd's
//              gradient at p for an incoming ray_scale[i]), and weight[i] * (p - m * log(q)).
struct SqFid {
    double scale;
    bool null() const { return false; }
    __device__ __forceinline__ double at(double p, double m, int64_t, double& term) const {
        const double r = p - m;
        term = rho_square(r);
        return r * scale;
    }
};
struct PerRay {
    const double* __restrict__ ray_scale;
    const double* __restrict__ weight;
    bool null() const { return !ray_scale || !weight; }
};
struct WsqFid : PerRay {
    __device__ __forceinline__ double at(double p, double m, int64_t i, double& term) const {
        const double r = p - m;
        term = weight[i] * rho_square(r);
        return r * ray_scale[i];
    }
};
struct RobustFid : PerRay {
    double delta;
    __device__ __forceinline__ double at(double p, double m, int64_t i, double& term) const {
        const double r = p - m;
        term = weight[i] * (delta > 0.0 ? rho_huber(r, delta) : rho_abs(r));
        return robust_psi(r, delta) * ray_scale[i];
    }
};
struct PoissonFid : PerRay {
    double eps;
    __device__ __forceinline__ double at(double p, double m, int64_t i, double& term) const {
        const double q = p + eps;
        term = weight[i] * rho_poisson(p, q, m);
        return poisson_weight(q, m, ray_scale[i]);
    }
};

// The residual launch of every fidelity term: for each j, i = order ? order[j] : j (a trace's
// row -> geometry ray map: r_scaled is then the transposed adjoint's input in trace order,
// without a separate permutation), p = yhat[i], m = y[i] (float32 or float64, promoted exactly),
// r_scaled[j] = fid.at(p, m, i, term), and the workgroup's partial sum of the terms.  Every
// value a single IEEE operation (no contraction); fixed strides and a fixed tree.
template <typename TY, class FID>
__global__ __launch_bounds__(kLossThreads) void residual_kernel(
    const double* __restrict__ yhat, const TY* __restrict__ y, int64_t n, FID fid,
    const int32_t* __restrict__ order, double* __restrict__ r_scaled, double* __restrict__ part) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; j < n;
         j += (int64_t)gridDim.x * kLossThreads) {
        const int64_t i = order ? (int64_t)order[j] : j;
        double term;
        r_scaled[j] = fid.at(yhat[i], (double)y[i], i, term);
        acc += term;
    }
    block_partial(acc, part);
}

// g -= c_neg where d < 0 (g.sub_(d.lt(0), alpha=c): g - c * 0 is g itself, signed zeros
// included); partial sums of |clamp(d, max=0)| (NaN stays NaN).
__global__ __launch_bounds__(kLossThreads) void neg_reg_kernel(
    const double* __restrict__ d, int64_t n, double c_neg, double* __restrict__ g,
    double* __restrict__ part) {
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kLossThreads) {
        const double v = d[i];
        const double c = v > 0.0 ? 0.0 : v;                // clamp(max=0): NaN and -0 pass
        acc += __builtin_fabs(c);
        if (v < 0.0) g[i] = g[i] - c_neg;
    }
    block_partial(acc, part);
}

// SmoothRegularizer (loss.py): the difference penalty over the axes (t, r, e, a) of a density,
//   P(d) = (1/N) sum_ax w_ax sum_{edges i -> i+1 along ax} rho(d[i+1] - d[i]),
// rho = r^2 (kind 0), |r| (SPHRT_RESID_ABS) or torch's huber_loss (SPHRT_RESID_HUBER); with `wrap`
// the azimuth ring closes: one more edge from a = na - 1 to a = 0 (na = 2: two edges between the
// pair).  An axis of length 1 or of weight 0 has no edges (and is not read: no 0 * inf).
struct SmoothDesc {
    uint32_t nt, nr, ne, na;    // axis lengths (every axis before t is batch: no edges across it)
    double wt, wr, we, wa;
    int kind;                   // 0, SPHRT_RESID_ABS, SPHRT_RESID_HUBER
    double delta;               // robust_psi's: > 0 for HUBER, 0 for ABS
    int wrap;                   // the azimuth ring is closed (and na > 1)
};

// rho'(r): 2r, sign(r) or r clamped to +-delta.
__device__ __forceinline__ double smooth_psi(double r, int kind, double delta) {
    return kind == 0 ? 2.0 * r : robust_psi(r, delta);
}

// rho(r); HUBER operation by operation as rho_huber.
__device__ __forceinline__ double smooth_rho(double r, int kind, double delta) {
    if (kind == 0) return r * r;
    const double z = __builtin_fabs(r);
    if (kind == SPHRT_RESID_ABS) return z;
    return z < delta ? (0.5 * z) * z : delta * (z - 0.5 * delta);
}

// One axis of voxel i (value v, coordinate c of n along the axis, element stride s): the lower
// then the upper neighbour's w * rho'(v - d_nb) onto S, and the upper edge's w * rho onto `edges`
// (every edge counted by its lower voxel; the wrap edge by the ring's last voxel).
__device__ __forceinline__ void smooth_axis(const double* __restrict__ d, uint32_t i, double v,
                                            uint32_t c, uint32_t n, uint32_t s, double w,
                                            bool wrap, int kind, double delta, double& S,
                                            double& edges) {
    if (!(w > 0.0) || n < 2) return;
    if (c > 0 || wrap) {
        const double lo = d[c > 0 ? i - s : i + (n - 1) * s];
        S += w * smooth_psi(v - lo, kind, delta);
    }
    if (c + 1 < n || wrap) {
        const double hi = d[c + 1 < n ? i + s : i - (n - 1) * s];
        S += w * smooth_psi(v - hi, kind, delta);
        edges += w * smooth_rho(hi - v, kind, delta);
    }
}

// S_i = sum over the present neighbours of w_ax * rho'(d_i - d_nb), in the fixed order t-, t+,
// r-, r+, e-, e+, a-, a+ (the one function every caller's gradient comes from: the same bits);
// `edges` receives the voxel's share of the penalty's sum.  Coordinates from 32-bit divisions
// (n < 2^31); every neighbour index stays inside the voxel's own (t, r, e, a) block.
__device__ __forceinline__ double smooth_sum(const double* __restrict__ d, uint32_t i, double v,
                                             const SmoothDesc& p, double& edges) {
    const uint32_t q1 = i / p.na, a = i - q1 * p.na;
    const uint32_t q2 = q1 / p.ne, e = q1 - q2 * p.ne;
    const uint32_t q3 = q2 / p.nr, r = q2 - q3 * p.nr;
    const uint32_t tt = q3 % p.nt;
    const uint32_t se = p.na, sr = p.ne * p.na, st = p.nr * sr;
    double S = 0.0;
    smooth_axis(d, i, v, tt, p.nt, st, p.wt, false, p.kind, p.delta, S, edges);
    smooth_axis(d, i, v, r, p.nr, sr, p.wr, false, p.kind, p.delta, S, edges);
    smooth_axis(d, i, v, e, p.ne, se, p.we, false, p.kind, p.delta, S, edges);
    smooth_axis(d, i, v, a, p.na, 1u, p.wa, p.wrap != 0, p.kind, p.delta, S, edges);
    return S;
}

// g_out = (g_in +) G, G_i = (S_i * inv_n) * lam — two roundings, in that order — and the partial
// sums of the penalty's edges.  With part_neg the NegRegularizer's term is folded in as
// neg_reg_kernel applies it (G - c_neg where d < 0; partial sums of |clamp(d, max=0)|), so that
// g_out = g_in + (G + neg): the order autograd leaves for [fidelity, the two regularisers].
// g_in may be g_out (each thread reads its own element first); d may not (neighbours are read).
__global__ __launch_bounds__(kLossThreads) void smooth_reg_kernel(
    const double* __restrict__ d, uint32_t n, SmoothDesc p, double inv_n, double lam, double c_neg,
    const double* g_in, double* g_out, double* __restrict__ part_smooth,
    double* __restrict__ part_neg) {
    double acc = 0.0, acc_neg = 0.0;
    for (uint32_t i = blockIdx.x * kLossThreads + threadIdx.x; i < n;
         i += gridDim.x * kLossThreads) {
        const double v = d[i];
        const double S = smooth_sum(d, i, v, p, acc);
        double h = (S * inv_n) * lam;
        if (part_neg) {                                    // as neg_reg_kernel
            const double c = v > 0.0 ? 0.0 : v;
            acc_neg += __builtin_fabs(c);
            if (v < 0.0) h = h - c_neg;
        }
        g_out[i] = g_in ? g_in[i] + h : h;
    }
    block_partial(acc, part_smooth);
    if (part_neg) {
        __syncthreads();                                   // (block_partial's LDS is reused)
        block_partial(acc_neg, part_neg);
    }
}

// Adam on float64 coefficients, with the NegRegularizer's gradient term and loss partials folded
// in: one launch where the loop made three or more (neg_reg, the step-count add, the optimiser's
// own launches).  Two arithmetics, each the per-element operation sequence of one of torch's
// implementations (amsgrad and maximize off):
//  - FOREACH = false: torch.optim.Adam(fused=True), torch._fused_adam_.  The multiply-adds are
//    the fused ones torch's ROCm build emits for `beta1 * m + (1 - beta1) * g` and
//    `beta2 * v + (1 - beta2) * g * g` (fma of the left product, and of p * weight_decay + g),
//    written out here since this library builds with -ffp-contract=off: measured bitwise equal
//    to torch._fused_adam_ over 20 steps with and without weight decay, where the unfused and the
//    right-product forms differ from step 1 (`test_adam_matches_torch_fused`).  Bias corrections
//    from the device's pow and sqrt, as torch's kernel computes them from its float32 step count.
//  - FOREACH = true: the default Adam on GPU tensors (torch.optim.adam._multi_tensor_adam, what
//    the reference's `optim(optim_vars, **kwargs)`, retrieval.py:84, runs on a CUDA/ROCm device):
//    _foreach_add(g, p, alpha=wd), _foreach_lerp_(m, g, 1 - beta1), _foreach_mul_(v, beta2),
//    _foreach_addcmul_(v, g, g, 1 - beta2), sqrt, / sqrt(1 - beta2^t), + eps,
//    _foreach_addcdiv_(p, m, denom, -lr / (1 - beta1^t)); each functor's `a + s * x` is one
//    fma in torch's ROCm build.  The bias corrections come from the host (Python floats, as
//    torch computes them): `step_size` is the negative step, `bc2s` sqrt(1 - beta2^t).
template <bool FOREACH>
__global__ __launch_bounds__(kLossThreads) void adam_neg_kernel(
    double* __restrict__ param, const double* __restrict__ grad, double* __restrict__ exp_avg,
    double* __restrict__ exp_avg_sq, int64_t n, double lr, double beta1, double beta2, double eps,
    double weight_decay, double step, double c_neg, double* __restrict__ part, StageMap sm,
    double* __restrict__ stage) {
    // the bias corrections once per workgroup (wave 0), under the first element's loads
    __shared__ double bc[2];
    const int64_t i0 = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    const bool in0 = i0 < n;
    double p0 = 0.0, g0 = 0.0, m0 = 0.0, v0 = 0.0;
    if (in0) {
        p0 = param[i0];
        g0 = grad[i0];
        m0 = exp_avg[i0];
        v0 = exp_avg_sq[i0];
    }
    double step_size, bc2s;
    if constexpr (FOREACH) {
        step_size = lr;            // (host: -lr / (1 - beta1^t))
        bc2s = step;               // (host: sqrt(1 - beta2^t))
    } else {
        if (threadIdx.x < 64) {
            const double b1 = 1 - pow(beta1, step), b2s = sqrt(1 - pow(beta2, step));
            if (threadIdx.x == 0) {
                bc[0] = b1;
                bc[1] = b2s;
            }
        }
        __syncthreads();
        step_size = lr / bc[0];
        bc2s = bc[1];
    }
    const double ob1 = 1 - beta1, ob2 = 1 - beta2;
    double acc = 0.0;
    for (int64_t i = i0; i < n; i += (int64_t)gridDim.x * kLossThreads) {
        const bool first = i == i0;
        double p = first ? p0 : param[i], g = first ? g0 : grad[i];
        const double mo = first ? m0 : exp_avg[i], vo = first ? v0 : exp_avg_sq[i];
        if (part) {                                        // as neg_reg_kernel
            const double c = p > 0.0 ? 0.0 : p;
            acc += __builtin_fabs(c);
            if (p < 0.0) g = g - c_neg;
        }
        double m, v, pn;
        if constexpr (FOREACH) {
            if (weight_decay != 0) g = fma(weight_decay, p, g);
            // lerp(m, g, w) with w = 1 - beta1 (ATen Lerp.h: the small-weight form below 0.5)
            m = __builtin_fabs(ob1) < 0.5 ? fma(ob1, g - mo, mo) : fma(-(g - mo), 1.0 - ob1, g);
            v = fma(ob2, g * g, vo * beta2);
            double den = sqrt(v);
            den = den / bc2s;
            den = den + eps;
            pn = fma(step_size, m / den, p);
        } else {
            if (weight_decay != 0) g = fma(p, weight_decay, g);
            m = fma(beta1, mo, ob1 * g);
            v = fma(beta2, vo, ob2 * g * g);
            const double denom = sqrt(v) / bc2s + eps;
            pn = p - step_size * m / denom;
        }
        param[i] = pn;
        if (stage) stage[stage_col((uint32_t)i, sm)] = pn;   // the next forward's brick copy
        exp_avg[i] = m;
        exp_avg_sq[i] = v;
    }
    if (part) block_partial(acc, part);
}

// ---- conjugate gradients (retrieval.cg): the vector side of an iteration in three launches ------
// The scalars alpha and beta are never on the host: each launch leaves its workgroups' partial
// sums of a dot product, and the next one has every workgroup sum those partials itself, all in
// the same fixed order, so the scalar has the same bits in every workgroup:
//   thread t adds the partials t, t + 256, t + 512, t + 768 (those below n_part <= 1024), in
//   that order, onto +0.0; the wave's 64 values by the xor butterfly 32, 16, 8, 4, 2, 1 (both
//   lanes of a pair form the same sum: IEEE addition commutes); the four wave totals, in order,
//   onto +0.0.
// Two sums at once (a launch needs at most two); every thread returns with both totals.
__device__ __forceinline__ void block_totals(const double* __restrict__ pa,
                                             const double* __restrict__ pb, int n_part,
                                             double& ta, double& tb) {
    __shared__ double sh[2][kLossThreads / 64];
    double a = 0.0, b = 0.0;
    for (int j = threadIdx.x; j < n_part; j += kLossThreads) {
        a += pa[j];
        b += pb[j];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[0][threadIdx.x >> 6] = a;
        sh[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    ta = tb = 0.0;
    for (int i = 0; i < kLossThreads / 64; ++i) {
        ta += sh[0][i];
        tb += sh[1][i];
    }
}

// h = c_damp * p + h (one fma: the damping term of N p onto A^T(s A p) + G p) and the partial
// sums of p * h over the new h.
__global__ __launch_bounds__(kLossThreads) void cg_curvature_kernel(
    const double* __restrict__ p, double* __restrict__ h, int64_t n, double c_damp,
    double* __restrict__ part) {
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kLossThreads) {
        const double pi = p[i];
        const double hi = fma(c_damp, pi, h[i]);
        h[i] = hi;
        acc += pi * hi;
    }
    block_partial(acc, part);
}

// alpha = RR / PHP — 0 once RR <= *rr_stop (the solve is frozen), when PHP is not > 0 (a zero
// right-hand side; a NaN fails the compare) and when the quotient is not finite; x += alpha p,
// r -= alpha h (one fma each) and the partial sums of the new r * r.  The thread's first
// elements are loaded before the partials are summed (their latencies overlap).
__global__ __launch_bounds__(kLossThreads) void cg_update_kernel(
    double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
    const double* __restrict__ h, int64_t n, const double* __restrict__ part_rr,
    const double* __restrict__ part_php, int n_part, const double* __restrict__ rr_stop,
    double* __restrict__ part_out) {
    const int64_t i0 = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    double x0 = 0.0, r0 = 0.0, p0 = 0.0, h0 = 0.0;
    if (i0 < n) {
        x0 = x[i0];
        r0 = r[i0];
        p0 = p[i0];
        h0 = h[i0];
    }
    double RR, PHP;
    block_totals(part_rr, part_php, n_part, RR, PHP);
    const double q = RR / PHP;
    const bool off = (rr_stop && RR <= *rr_stop) || !(PHP > 0.0) || !__builtin_isfinite(q);
    const double alpha = off ? 0.0 : q;
    double acc = 0.0;
    for (int64_t i = i0; i < n; i += (int64_t)gridDim.x * kLossThreads) {
        const bool first = i == i0;
        const double xi = first ? x0 : x[i], ri = first ? r0 : r[i];
        const double pi = first ? p0 : p[i], hi = first ? h0 : h[i];
        x[i] = fma(alpha, pi, xi);
        const double rn = fma(-alpha, hi, ri);
        r[i] = rn;
        acc += rn * rn;
    }
    block_partial(acc, part_out);
}

// beta = RR_new / RR_old — 0 once RR_old <= *rr_stop and when RR_old is not > 0; p = beta p + r
// (one fma).
__global__ __launch_bounds__(kLossThreads) void cg_direction_kernel(
    double* __restrict__ p, const double* __restrict__ r, int64_t n,
    const double* __restrict__ part_new, const double* __restrict__ part_old, int n_part,
    const double* __restrict__ rr_stop) {
    const int64_t i0 = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    double p0 = 0.0, r0 = 0.0;
    if (i0 < n) {
        p0 = p[i0];
        r0 = r[i0];
    }
    double RRn, RRo;
    block_totals(part_new, part_old, n_part, RRn, RRo);
    const bool off = (rr_stop && RRo <= *rr_stop) || !(RRo > 0.0);
    const double beta = off ? 0.0 : RRn / RRo;
    for (int64_t i = i0; i < n; i += (int64_t)gridDim.x * kLossThreads) {
        const bool first = i == i0;
        p[i] = fma(beta, first ? p0 : p[i], first ? r0 : r[i]);
    }
}

// ---- projected gradient with momentum (retrieval.fista): the vector side in two launches --------
// The step 1 / L is read through a pointer (it is estimated on the device) and the restart
// decision GD = SUM(part_gd) is formed by every workgroup of the second launch, in block_totals'
// order, so neither reaches the host during a solve.

// block_partial for two sums at once.
__device__ __forceinline__ void block_partial2(double a, double b, double* out_a, double* out_b) {
    __shared__ double sh[2][kLossThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[0][threadIdx.x >> 6] = a;
        sh[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sb = 0.0;
        for (int i = 0; i < kLossThreads / 64; ++i) {
            sa += sh[0][i];
            sb += sh[1][i];
        }
        out_a[blockIdx.x] = sa;
        out_b[blockIdx.x] = sb;
    }
}

// block_totals for one sum (the same order).
__device__ __forceinline__ double block_total(const double* __restrict__ pa, int n_part) {
    __shared__ double sh[kLossThreads / 64];
    double a = 0.0;
    for (int j = threadIdx.x; j < n_part; j += kLossThreads) a += pa[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    double ta = 0.0;
    for (int i = 0; i < kLossThreads / 64; ++i) ta += sh[i];
    return ta;
}

// g' = c_damp z + g, u = z - step g' (one fma each), x_new = u clamped by two compares (a NaN u
// fails both and stays NaN; a bound that is hit is stored with the bound's own bits), and the
// partial sums of g' (x_new - x_old) and of (z - x_new)^2.
__global__ __launch_bounds__(kLossThreads) void pg_step_kernel(
    const double* __restrict__ z, const double* __restrict__ g, const double* __restrict__ x_old,
    double* __restrict__ x_new, int64_t n, double c_damp, const double* __restrict__ step,
    double lower, double upper, double* __restrict__ part_gd, double* __restrict__ part_mm) {
    const double neg_step = -*step;
    double gd = 0.0, mm = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kLossThreads) {
        const double zi = z[i];
        const double gp = fma(c_damp, zi, g[i]);
        const double u = fma(neg_step, gp, zi);
        const double xn = u < lower ? lower : (u > upper ? upper : u);
        x_new[i] = xn;
        const double dx = xn - x_old[i];
        gd += gp * dx;
        const double dz = zi - xn;
        mm += dz * dz;
    }
    block_partial2(gd, mm, part_gd, part_mm);
}

// GD = SUM(part_gd); j = GD > 0 ? 1 : min(*j_in + 1, n_omega - 1) (a NaN GD fails the compare:
// no restart); z = x_new + omega[j] (x_new - x_old) (one fma).  The thread's first elements are
// loaded before the partials are summed.  j is kept inside the table whatever *j_in holds.
__global__ __launch_bounds__(kLossThreads) void pg_momentum_kernel(
    double* __restrict__ z, const double* __restrict__ x_new, const double* __restrict__ x_old,
    int64_t n, const double* __restrict__ part_gd, int n_part, const double* __restrict__ omega,
    int64_t n_omega, const int64_t* __restrict__ j_in, int64_t* __restrict__ j_out) {
    const int64_t i0 = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    double a0 = 0.0, b0 = 0.0;
    if (i0 < n) {
        a0 = x_new[i0];
        b0 = x_old[i0];
    }
    const int64_t jp = *j_in;
    const double GD = block_total(part_gd, n_part);
    int64_t j = GD > 0.0 ? 1 : (jp >= n_omega - 1 ? n_omega - 1 : jp + 1);
    if (j < 0) j = 0;
    const double w = omega[j];
    for (int64_t i = i0; i < n; i += (int64_t)gridDim.x * kLossThreads) {
        const bool first = i == i0;
        const double xn = first ? a0 : x_new[i], xo = first ? b0 : x_old[i];
        z[i] = fma(w, xn - xo, xn);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *j_out = j;
}

// ---- primal-dual (retrieval.primal_dual): the vector side in two launches -------------------------
// For min F(x) + sum_ax c_ax |D_ax x|_1 over lower <= x <= upper (include/sphrt_pd.h): the
// steps tau and sigma are read through pointers (they come from an L estimated on the device).
// Both kernels stream their vectors once with plain loads and take the neighbours from cache;
// index arithmetic as smooth_sum's (32-bit divisions, n < 2^31), and every neighbour index stays
// inside the volume.  Contraction is switched off in each body, so the products that feed the
// sums stay plain multiplies under any -ffp-contract, as sphrt_pd.h promises.
struct PdDesc {
    uint32_t nr, ne, na;
    int has_r, has_e, has_a;    // the axis has edges (host: flag set and length > 1)
    int wrap;                   // the azimuth ring is closed (and na > 1)
};

// Voxel i as (r, e, a), with the element strides sr and se of the r and e axes (a's is 1).
struct PdVoxel {
    uint32_t r, e, a, sr, se;
};
__device__ __forceinline__ PdVoxel pd_voxel(const PdDesc& p, uint32_t i) {
    const uint32_t q1 = i / p.na, a = i - q1 * p.na;
    const uint32_t r = q1 / p.ne, e = q1 - r * p.ne;
    return PdVoxel{r, e, a, p.ne * p.na, p.na};
}

// One axis of (D^T q)[i]: + q_ax[lower neighbour] for the edge arriving at i, then - q_ax[i] for
// the edge leaving it (coordinate c of n along the axis, element stride s).
// (WEIGHTED — sphrt_iso_primal_f64, include/sphrt_iso.h: the edges carry the axis' weight w, one
// fma each; with w = 1 the product is exact and the sum is the plain one's, bit for bit)
template <bool WEIGHTED>
__device__ __forceinline__ void pd_axis_adjoint(const double* __restrict__ qa, uint32_t i,
                                                uint32_t c, uint32_t n, uint32_t s, bool wrap,
                                                double w, double& S) {
#pragma clang fp contract(off)
    if (c > 0 || wrap) {
        const double ql = qa[c > 0 ? i - s : i + (n - 1) * s];
        S = WEIGHTED ? fma(w, ql, S) : S + ql;
    }
    if (c + 1 < n || wrap) S = WEIGHTED ? fma(-w, qa[i], S) : S - qa[i];
}

// (PER_VOXEL: tau holds n steps, one per voxel — sphrt_dp_primal_f64 — instead of one)
// (WEIGHTED: the adjoint of the weighted differences, w_ax per axis; otherwise w_* are not read)
template <bool PER_VOXEL, bool WEIGHTED = false>
__global__ __launch_bounds__(kLossThreads) void pd_primal_kernel(
    const double* __restrict__ x, const double* __restrict__ g, const double* __restrict__ q,
    double* __restrict__ x_new, uint32_t n, PdDesc p, double c_damp,
    const double* __restrict__ tau, double lower, double upper, double* __restrict__ part_mm,
    double w_r = 1.0, double w_e = 1.0, double w_a = 1.0) {
#pragma clang fp contract(off)
    const double neg_tau0 = PER_VOXEL ? 0.0 : -*tau;
    double mm = 0.0;
    for (uint32_t i = blockIdx.x * kLossThreads + threadIdx.x; i < n;
         i += gridDim.x * kLossThreads) {
        const PdVoxel v = pd_voxel(p, i);
        const double xi = x[i];
        const double gp = fma(c_damp, xi, g[i]);
        double S = 0.0;
        if (p.has_r) pd_axis_adjoint<WEIGHTED>(q, i, v.r, p.nr, v.sr, false, w_r, S);
        if (p.has_e) pd_axis_adjoint<WEIGHTED>(q + n, i, v.e, p.ne, v.se, false, w_e, S);
        if (p.has_a)
            pd_axis_adjoint<WEIGHTED>(q + 2 * (size_t)n, i, v.a, p.na, 1u, p.wrap != 0, w_a, S);
        const double neg_tau = PER_VOXEL ? -tau[i] : neg_tau0;
        const double u = fma(neg_tau, gp + S, xi);
        const double xn = u < lower ? lower : (u > upper ? upper : u);
        x_new[i] = xn;
        const double dx = xn - xi;
        mm += dx * dx;
    }
    block_partial(mm, part_mm);
}

// One axis of v = q + sigma Dw xb at voxel i (xb = 2 x_new - x_old, xb_i that of i), for the edge
// leaving i, if any (coordinate c of n along the axis, element stride s; its upper voxel j) ->
// whether there is one; qo its old dual, v = fma(sigma, w (xb_j - xb_i), qo) the stepped one.
// (WEIGHTED — include/sphrt_iso.h: the multiply by the axis' weight w; otherwise w is not read)
template <bool WEIGHTED>
__device__ __forceinline__ bool pd_edge_step(const double* __restrict__ x_new,
                                             const double* __restrict__ x_old, const double* qa,
                                             uint32_t i, double xb_i, uint32_t c, uint32_t n,
                                             uint32_t s, bool wrap, double sigma, double w,
                                             double& qo, double& v) {
#pragma clang fp contract(off)
    if (!(c + 1 < n || wrap)) return false;
    const uint32_t j = c + 1 < n ? i + s : i - (n - 1) * s;
    const double xb_j = fma(2.0, x_new[j], -x_old[j]);
    qo = qa[i];
    const double d = WEIGHTED ? w * (xb_j - xb_i) : xb_j - xb_i;
    v = fma(sigma, d, qo);
    return true;
}

// One axis of the dual update at voxel i: the edge leaving i, if any, takes the stepped v clamped
// to +-c, and its squared change goes onto t.
__device__ __forceinline__ void pd_axis_dual(const double* __restrict__ x_new,
                                             const double* __restrict__ x_old, double* qa,
                                             uint32_t i, double xb_i, uint32_t c, uint32_t n,
                                             uint32_t s, bool wrap, double sigma, double cax,
                                             double& t) {
#pragma clang fp contract(off)
    double qo, v;
    if (!pd_edge_step<false>(x_new, x_old, qa, i, xb_i, c, n, s, wrap, sigma, 1.0, qo, v)) return;
    const double qn = v < -cax ? -cax : (v > cax ? cax : v);
    qa[i] = qn;
    const double dq = qn - qo;
    t += dq * dq;
}

// (q is read and written at the thread's own slots only: in place; not __restrict__-qualified
// against itself, and distinct from x_new / x_old by the host's overlap check)
__global__ __launch_bounds__(kLossThreads) void pd_dual_kernel(
    const double* __restrict__ x_new, const double* __restrict__ x_old, double* q, uint32_t n,
    PdDesc p, double c_r, double c_e, double c_a, const double* __restrict__ sigma,
    double* __restrict__ part_qq) {
#pragma clang fp contract(off)
    const double sg = *sigma;
    double qq = 0.0;
    for (uint32_t i = blockIdx.x * kLossThreads + threadIdx.x; i < n;
         i += gridDim.x * kLossThreads) {
        const PdVoxel v = pd_voxel(p, i);
        const double xb = fma(2.0, x_new[i], -x_old[i]);
        double t = 0.0;
        if (p.has_r) pd_axis_dual(x_new, x_old, q, i, xb, v.r, p.nr, v.sr, false, sg, c_r, t);
        if (p.has_e) pd_axis_dual(x_new, x_old, q + n, i, xb, v.e, p.ne, v.se, false, sg, c_e, t);
        if (p.has_a)
            pd_axis_dual(x_new, x_old, q + 2 * (size_t)n, i, xb, v.a, p.na, 1u, p.wrap != 0, sg,
                         c_a, t);
        qq += t;
    }
    block_partial(qq, part_qq);
}

// The dual step of isotropic TV (include/sphrt_iso.h): the voxel's triple v of weighted edge
// steps projected onto the ball of `radius` — one
// square root and one division per voxel over pd_dual_kernel, the same bytes.  (q in place at the
// thread's own slots, as in pd_dual_kernel.)
__global__ __launch_bounds__(kLossThreads) void iso_dual_kernel(
    const double* __restrict__ x_new, const double* __restrict__ x_old, double* q, uint32_t n,
    PdDesc p, double w_r, double w_e, double w_a, double radius,
    const double* __restrict__ sigma, double* __restrict__ part_qq) {
#pragma clang fp contract(off)
    const double sg = *sigma;
    double* const q_r = q;
    double* const q_e = q + n;
    double* const q_a = q + 2 * (size_t)n;
    double qq = 0.0;
    for (uint32_t i = blockIdx.x * kLossThreads + threadIdx.x; i < n;
         i += gridDim.x * kLossThreads) {
        const PdVoxel c = pd_voxel(p, i);
        const double xb = fma(2.0, x_new[i], -x_old[i]);
        double o_r = 0.0, o_e = 0.0, o_a = 0.0, v_r = 0.0, v_e = 0.0, v_a = 0.0;
        const bool on_r = p.has_r && pd_edge_step<true>(x_new, x_old, q_r, i, xb, c.r, p.nr, c.sr,
                                                        false, sg, w_r, o_r, v_r);
        const bool on_e = p.has_e && pd_edge_step<true>(x_new, x_old, q_e, i, xb, c.e, p.ne, c.se,
                                                        false, sg, w_e, o_e, v_e);
        const bool on_a = p.has_a && pd_edge_step<true>(x_new, x_old, q_a, i, xb, c.a, p.na, 1u,
                                                        p.wrap != 0, sg, w_a, o_a, v_a);
        double n2 = 0.0;
        if (on_r) n2 = n2 + v_r * v_r;
        if (on_e) n2 = n2 + v_e * v_e;
        if (on_a) n2 = n2 + v_a * v_a;
        const double nrm = sqrt(n2);
        const bool outside = nrm > radius;              // (a NaN fails the compare: v is stored)
        const double scale = outside ? radius / nrm : 1.0;
        double t = 0.0;
        if (on_r) {
            const double qn = outside ? v_r * scale : v_r;
            q_r[i] = qn;
            const double dq = qn - o_r;
            t = t + dq * dq;
        }
        if (on_e) {
            const double qn = outside ? v_e * scale : v_e;
            q_e[i] = qn;
            const double dq = qn - o_e;
            t = t + dq * dq;
        }
        if (on_a) {
            const double qn = outside ? v_a * scale : v_a;
            q_a[i] = qn;
            const double dq = qn - o_a;
            t = t + dq * dq;
        }
        qq += t;
    }
    block_partial(qq, part_qq);
}

// The ray side of retrieval.chambolle_pock (include/sphrt_cp.h: the operation order of every
// kind): p <- prox_{sigma phi*}(p + sigma (2 z_new - z_old)) in place at the thread's own slot
// i = order[j], its copy in the adjoint's order, and the partial sums of (p+ - p)^2 and of
// weight * rho(z_new, y) — rho the residual policies' own (rho_square .. rho_poisson).  48 bytes read and
// 8 or 16 written per ray, coalesced but for the gathers through `order`.  PER_RAY: sigma holds
// n steps, indexed as ray_scale is (sphrt_dp_ray_dual_f64), instead of one.
template <typename TY, int KIND, bool PER_RAY>
__global__ __launch_bounds__(kLossThreads) void cp_ray_dual_kernel(
    const double* __restrict__ z_new, const double* __restrict__ z_old, const TY* __restrict__ y,
    int64_t n, double par, const double* __restrict__ ray_scale,
    const double* __restrict__ weight, const double* __restrict__ sigma,
    const int32_t* __restrict__ order, double* p, double* __restrict__ p_adj,
    double* __restrict__ part_pp, double* __restrict__ part_fid) {
#pragma clang fp contract(off)
    const double sg0 = PER_RAY ? 0.0 : *sigma;
    double pp = 0.0, fid = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; j < n;
         j += (int64_t)gridDim.x * kLossThreads) {
        const int64_t i = order ? (int64_t)order[j] : j;
        const double zn = z_new[i], m = (double)y[i], s = ray_scale[i], po = p[i];
        const double sg = PER_RAY ? sigma[i] : sg0;
        const double zb = fma(2.0, zn, -z_old[i]);
        const double a = fma(sg, zb, po);
        const double t = fma(-sg, m, a);
        const double r = zn - m;
        double pn, h;
        if constexpr (KIND == SPHRT_CP_SQUARE) {
            pn = t / (1.0 + sg / (2.0 * s));
            h = rho_square(r);
        } else if constexpr (KIND == SPHRT_CP_ABS) {
            pn = t < -s ? -s : (t > s ? s : t);
            h = rho_abs(r);
        } else if constexpr (KIND == SPHRT_CP_HUBER) {
            const double u = t / (1.0 + sg / s), b = s * par;
            pn = u < -b ? -b : (u > b ? b : u);
            h = rho_huber(r, par);
        } else {
            const double a1 = fma(sg, par, a);
            const double d = a1 - s, e = a1 + s;
            const double disc = fma((4.0 * sg) * s, m, d * d);
            const double v = 0.5 * (e - sqrt(disc));
            pn = v > s ? s : v;
            const double qe = zn + par;
            h = rho_poisson(zn, qe, m);
        }
        if (s == 0.0) pn = 0.0;
        p[i] = pn;
        if (order) p_adj[j] = pn;
        const double dp = pn - po;
        pp += dp * dp;
        const double wh = weight[i] * h;
        fid += wh;
    }
    block_partial2(pp, fid, part_pp, part_fid);
}

// The steps of the diagonally preconditioned iteration (include/sphrt_dp.h): tau per voxel from
// the column sums and the voxel's edge count — index arithmetic as pd_primal_kernel's, no memory
// — and sigma per ray from the row sums, in one launch over the longer of the two.
__global__ __launch_bounds__(kLossThreads) void dp_steps_kernel(
    const double* __restrict__ col, const double* __restrict__ row, uint32_t n_vox,
    uint32_t n_ray, PdDesc p, double rho, double c, const int32_t* __restrict__ order,
    double* __restrict__ tau, double* __restrict__ sigma) {
#pragma clang fp contract(off)
    const uint32_t n = n_vox > n_ray ? n_vox : n_ray;
    for (uint32_t j = blockIdx.x * kLossThreads + threadIdx.x; j < n;
         j += gridDim.x * kLossThreads) {
        if (j < n_vox) {
            const PdVoxel v = pd_voxel(p, j);
            int deg = 0;
            if (p.has_r) deg += (v.r > 0) + (v.r + 1 < p.nr);
            if (p.has_e) deg += (v.e > 0) + (v.e + 1 < p.ne);
            if (p.has_a) deg += p.wrap ? 2 : (v.a > 0) + (v.a + 1 < p.na);
            const double d = fma(rho, col[j] + (double)deg, c);
            tau[j] = d > 0.0 ? 1.0 / d : 0.0;
        }
        if (j < n_ray) {
            const double r = row[order ? (uint32_t)order[j] : j];
            sigma[j] = r > 0.0 ? rho / r : 0.0;
        }
    }
}

static unsigned loss_grid(int64_t n) {
    const int64_t b = (n + kLossThreads - 1) / kLossThreads;
    return (unsigned)(b < kLossMaxBlocks ? (b > 0 ? b : 1) : kLossMaxBlocks);
}

// Do two buffers of na and nb bytes share a byte (addresses compared as integers; nothing read).
static bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb ? pb - pa < (uintptr_t)na : pa - pb < (uintptr_t)nb;
}

// The alias refusal of the pd, iso, dp and cp entries: each of the first n_outputs of the n
// buffers against every buffer after it (all of them: n_outputs = n); a null one — an optional
// buffer left out — is skipped.
static int refuse_aliased(const char* me, const void* const* buf, const int64_t* len,
                          int n_outputs, int n) {
    for (int a = 0; a < n_outputs; ++a)
        for (int b = a + 1; b < n; ++b)
            if (buf[a] && buf[b] && overlap(buf[a], len[a], buf[b], len[b]))
                return fail("%s: aliased buffers", me);
    return 0;
}

// The host refusals the three cg entries share: the length and the count of partial sums that a
// launch over that length leaves (nothing is dereferenced).
static int refuse_cg(const char* me, int64_t n, int64_t n_part, bool check_part) {
    if (n <= 0) return fail("%s: empty vector (n %lld)", me, (long long)n);
    if (check_part && n_part != (int64_t)loss_grid(n))
        return fail("%s: n_part %lld, a launch over %lld elements leaves %u partial sums", me,
                    (long long)n_part, (long long)n, loss_grid(n));
    return 0;
}

// The host side of the four residual entries: the refusals in their order (`me`: the entry's
// name), the stream's device, residual_kernel for y's type, and the launch check under `label`.
template <class FID>
static int residual_launch(const char* me, const char* label, FID fid, const double* yhat,
                           const void* y, int y_is_f64, int64_t n, const int32_t* order,
                           double* r_scaled, double* partial_sums, void* stream) {
    if (n <= 0) return fail("%s: empty measurement", me);
    if (!yhat || !y || fid.null() || !r_scaled || !partial_sums) return fail("null buffer");
    StreamGuard guard(stream);
    const dim3 grid(loss_grid(n)), block(kLossThreads);
    if (y_is_f64)
        hipLaunchKernelGGL((residual_kernel<double, FID>), grid, block, 0, (hipStream_t)stream,
                           yhat, (const double*)y, n, fid, order, r_scaled, partial_sums);
    else
        hipLaunchKernelGGL((residual_kernel<float, FID>), grid, block, 0, (hipStream_t)stream,
                           yhat, (const float*)y, n, fid, order, r_scaled, partial_sums);
    return check_launch(label);
}

}  // namespace sphrt

using namespace sphrt;

extern "C" int64_t sphrt_loss_partials(int64_t n) { return n > 0 ? (int64_t)loss_grid(n) : 0; }

extern "C" int sphrt_sq_residual_f64(const double* yhat, const void* y, int y_is_f64, int64_t n,
                                     double scale, const int32_t* order, double* r_scaled,
                                     double* partial_sums, void* stream) {
    return residual_launch("sphrt_sq_residual_f64", "sq_residual", SqFid{scale}, yhat, y, y_is_f64,
                           n, order, r_scaled, partial_sums, stream);
}

extern "C" int sphrt_wsq_residual_f64(const double* yhat, const void* y, int y_is_f64, int64_t n,
                                      const double* ray_scale, const double* weight,
                                      const int32_t* order, double* r_scaled,
                                      double* partial_sums, void* stream) {
    return residual_launch("sphrt_wsq_residual_f64", "wsq_residual", WsqFid{{ray_scale, weight}},
                           yhat, y, y_is_f64, n, order, r_scaled, partial_sums, stream);
}

extern "C" int sphrt_robust_residual_f64(const double* yhat, const void* y, int y_is_f64,
                                         int64_t n, int kind, double delta,
                                         const double* ray_scale, const double* weight,
                                         const int32_t* order, double* r_scaled,
                                         double* partial_sums, void* stream) {
    double rd;
    if (int e = refuse_robust(kind, delta, rd)) return e;
    return residual_launch("sphrt_robust_residual_f64", "robust_residual",
                           RobustFid{{ray_scale, weight}, rd}, yhat, y, y_is_f64, n, order,
                           r_scaled, partial_sums, stream);
}

extern "C" int sphrt_poisson_residual_f64(const double* yhat, const void* y, int y_is_f64,
                                          int64_t n, double eps, const double* ray_scale,
                                          const double* weight, const int32_t* order,
                                          double* r_scaled, double* partial_sums, void* stream) {
    if (int e = refuse_poisson(eps)) return e;
    return residual_launch("sphrt_poisson_residual_f64", "poisson_residual",
                           PoissonFid{{ray_scale, weight}, eps}, yhat, y, y_is_f64, n, order,
                           r_scaled, partial_sums, stream);
}

extern "C" int sphrt_neg_reg_f64(const double* d, int64_t n, double c_neg, double* g,
                                 double* partial_sums, void* stream) {
    if (n <= 0) return fail("sphrt_neg_reg_f64: empty volume");
    if (!d || !g || !partial_sums) return fail("null buffer");
    StreamGuard guard(stream);
    hipLaunchKernelGGL(neg_reg_kernel, dim3(loss_grid(n)), dim3(kLossThreads), 0,
                       (hipStream_t)stream, d, n, c_neg, g, partial_sums);
    return check_launch("neg_reg");
}

extern "C" int sphrt_smooth_reg_f64(const double* d, int64_t n_batch, int nt, int nr, int ne, int na,
                                    double wt, double wr, double we, double wa, int kind,
                                    double delta, int wrap_a, double inv_n, double lam,
                                    double c_neg, const double* g_in, double* g_out,
                                    double* part_smooth, double* part_neg, void* stream) {
    const char* me = "sphrt_smooth_reg_f64";
    if (nt < 1 || nr < 1 || ne < 1 || na < 1)
        return fail("%s: axis lengths (%d, %d, %d, %d) must be >= 1", me, nt, nr, ne, na);
    if (n_batch < 1) return fail("%s: empty volume (n_batch %lld)", me, (long long)n_batch);
    const int64_t lim = (int64_t)1 << 31;
    int64_t n = n_batch;                      // (every factor < 2^31: no int64 overflow below)
    for (int len : {nt, nr, ne, na}) {
        if (n >= lim) break;
        n *= len;
    }
    if (n >= lim) return fail("%s: the volume must have fewer than 2^31 voxels", me);
    for (double w : {wt, wr, we, wa})
        if (!(w >= 0.0) || __builtin_isinf(w))           // (a NaN fails the compare)
            return fail("%s: the axis weights must be finite and >= 0, not %g", me, w);
    if (__builtin_isnan(inv_n) || __builtin_isinf(inv_n) || __builtin_isnan(lam) ||
        __builtin_isinf(lam))
        return fail("%s: inv_n and lam must be finite, not %g and %g", me, inv_n, lam);
    double rd = 0.0;
    if (kind != 0)
        if (int e = refuse_robust(kind, delta, rd)) return e;
    if (!part_smooth) return fail("%s: null part_smooth", me);
    if (!g_out) return fail("%s: null g_out", me);
    if (!d) return fail("%s: null density", me);
    if (d == g_out) return fail("%s: d and g_out must not be the same buffer", me);
    SmoothDesc p{(uint32_t)nt, (uint32_t)nr, (uint32_t)ne, (uint32_t)na, wt, wr, we, wa,
                 kind, rd, wrap_a && na > 1};
    StreamGuard guard(stream);
    hipLaunchKernelGGL(smooth_reg_kernel, dim3(loss_grid(n)), dim3(kLossThreads), 0,
                       (hipStream_t)stream, d, (uint32_t)n, p, inv_n, lam, c_neg, g_in, g_out,
                       part_smooth, part_neg);
    return check_launch("smooth_reg");
}

static int adam_launch(bool foreach, double* param, const double* grad, double* exp_avg,
                       double* exp_avg_sq, int64_t n, double a, double beta1, double beta2,
                       double eps, double weight_decay, double b, double c_neg,
                       double* partial_sums, const sphrt_csr* stage_of, void* stream,
                       const char* what) {
    if (n <= 0) return fail("%s: empty volume", what);
    if (!param || !grad || !exp_avg || !exp_avg_sq) return fail("null buffer");
    StageMap sm{};
    double* stage = nullptr;
    if (stage_of && staged(stage_of)) {
        if (!stage_map(stage_of, sm)) return fail("inconsistent brick staging fields");
        if (stage_of->n_cols != n)
            return fail("%s: %lld voxels, the CSR has %lld columns", what, (long long)n,
                        (long long)stage_of->n_cols);
        if (!stage_of->stage || (int64_t)sizeof(double) * stage_of->stage_cols > stage_of->stage_bytes)
            return fail("brick stage buffer missing or too small");
        stage = (double*)stage_of->stage;
    }
    StreamGuard guard(stream);
    if (foreach)
        hipLaunchKernelGGL(adam_neg_kernel<true>, dim3(loss_grid(n)), dim3(kLossThreads), 0,
                           (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, a, beta1,
                           beta2, eps, weight_decay, b, c_neg, partial_sums, sm, stage);
    else
        hipLaunchKernelGGL(adam_neg_kernel<false>, dim3(loss_grid(n)), dim3(kLossThreads), 0,
                           (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, a, beta1,
                           beta2, eps, weight_decay, b, c_neg, partial_sums, sm, stage);
    return check_launch(what);
}

extern "C" int sphrt_adam_neg_f64(double* param, const double* grad, double* exp_avg,
                                  double* exp_avg_sq, int64_t n, double lr, double beta1,
                                  double beta2, double eps, double weight_decay, double step,
                                  double c_neg, double* partial_sums, const sphrt_csr* stage_of,
                                  void* stream) {
    if (!(step >= 1)) return fail("sphrt_adam_neg_f64: step counts from 1");
    return adam_launch(false, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps,
                       weight_decay, step, c_neg, partial_sums, stage_of, stream,
                       "sphrt_adam_neg_f64");
}

extern "C" int sphrt_adam_foreach_neg_f64(double* param, const double* grad, double* exp_avg,
                                          double* exp_avg_sq, int64_t n, double step_size,
                                          double beta1, double beta2, double eps,
                                          double weight_decay, double bc2_sqrt, double c_neg,
                                          double* partial_sums, const sphrt_csr* stage_of,
                                          void* stream) {
    if (!(bc2_sqrt > 0)) return fail("sphrt_adam_foreach_neg_f64: bias correction must be > 0");
    return adam_launch(true, param, grad, exp_avg, exp_avg_sq, n, step_size, beta1, beta2, eps,
                       weight_decay, bc2_sqrt, c_neg, partial_sums, stage_of, stream,
                       "sphrt_adam_foreach_neg_f64");
}

extern "C" int sphrt_cg_curvature_f64(const double* p, double* h, int64_t n, double c_damp,
                                      double* part_php, void* stream) {
    const char* me = "sphrt_cg_curvature_f64";
    if (int e = refuse_cg(me, n, 0, false)) return e;
    if (!p || !h || !part_php) return fail("%s: null buffer", me);
    StreamGuard guard(stream);
    hipLaunchKernelGGL(cg_curvature_kernel, dim3(loss_grid(n)), dim3(kLossThreads), 0,
                       (hipStream_t)stream, p, h, n, c_damp, part_php);
    return check_launch("cg_curvature");
}

extern "C" int sphrt_cg_update_f64(double* x, double* r, const double* p, const double* h,
                                   int64_t n, const double* part_rr, const double* part_php,
                                   int64_t n_part, const double* rr_stop, double* part_rr_new,
                                   void* stream) {
    const char* me = "sphrt_cg_update_f64";
    if (int e = refuse_cg(me, n, n_part, true)) return e;
    if (!x || !r || !p || !h || !part_rr || !part_php || !part_rr_new)
        return fail("%s: null buffer", me);
    StreamGuard guard(stream);
    hipLaunchKernelGGL(cg_update_kernel, dim3(loss_grid(n)), dim3(kLossThreads), 0,
                       (hipStream_t)stream, x, r, p, h, n, part_rr, part_php, (int)n_part,
                       rr_stop, part_rr_new);
    return check_launch("cg_update");
}

extern "C" int sphrt_cg_direction_f64(double* p, const double* r, int64_t n,
                                      const double* part_rr_new, const double* part_rr,
                                      int64_t n_part, const double* rr_stop, void* stream) {
    const char* me = "sphrt_cg_direction_f64";
    if (int e = refuse_cg(me, n, n_part, true)) return e;
    if (!p || !r || !part_rr_new || !part_rr) return fail("%s: null buffer", me);
    StreamGuard guard(stream);
    hipLaunchKernelGGL(cg_direction_kernel, dim3(loss_grid(n)), dim3(kLossThreads), 0,
                       (hipStream_t)stream, p, r, n, part_rr_new, part_rr, (int)n_part, rr_stop);
    return check_launch("cg_direction");
}

extern "C" int sphrt_pg_step_f64(const double* z, const double* g, const double* x_old,
                                 double* x_new, int64_t n, double c_damp, const double* step,
                                 double lower, double upper, double* part_gd, double* part_mm,
                                 void* stream) {
    const char* me = "sphrt_pg_step_f64";
    if (int e = refuse_cg(me, n, 0, false)) return e;
    if (!z || !g || !x_old || !x_new || !step || !part_gd || !part_mm)
        return fail("%s: null buffer", me);
    if (lower != lower || upper != upper || !(lower < upper))
        return fail("%s: bounds need lower < upper, neither NaN (%g, %g)", me, lower, upper);
    const int64_t nb = n * (int64_t)sizeof(double), pb = (int64_t)loss_grid(n) * sizeof(double);
    const void* vec[4] = {z, g, x_old, x_new};
    for (int a = 0; a < 4; ++a) {
        for (int b = a + 1; b < 4; ++b)
            if (overlap(vec[a], nb, vec[b], nb)) return fail("%s: aliased vectors", me);
        if (overlap(vec[a], nb, part_gd, pb) || overlap(vec[a], nb, part_mm, pb) ||
            overlap(vec[a], nb, step, sizeof(double)))
            return fail("%s: a vector aliased with the partial sums or the step", me);
    }
    if (overlap(part_gd, pb, part_mm, pb) || overlap(part_gd, pb, step, sizeof(double)) ||
        overlap(part_mm, pb, step, sizeof(double)))
        return fail("%s: aliased partial sums", me);
    StreamGuard guard(stream);
    hipLaunchKernelGGL(pg_step_kernel, dim3(loss_grid(n)), dim3(kLossThreads), 0,
                       (hipStream_t)stream, z, g, x_old, x_new, n, c_damp, step, lower, upper,
                       part_gd, part_mm);
    return check_launch("pg_step");
}

extern "C" int sphrt_pg_momentum_f64(double* z, const double* x_new, const double* x_old,
                                     int64_t n, const double* part_gd, int64_t n_part,
                                     const double* omega, int64_t n_omega, const int64_t* j_in,
                                     int64_t* j_out, void* stream) {
    const char* me = "sphrt_pg_momentum_f64";
    if (int e = refuse_cg(me, n, n_part, true)) return e;
    if (!z || !x_new || !x_old || !part_gd || !omega || !j_in || !j_out)
        return fail("%s: null buffer", me);
    if (n_omega < 2) return fail("%s: n_omega %lld, the table holds at least two factors", me,
                                 (long long)n_omega);
    const int64_t nb = n * (int64_t)sizeof(double), pb = n_part * (int64_t)sizeof(double);
    if (overlap(z, nb, x_new, nb) || overlap(z, nb, x_old, nb) || overlap(x_new, nb, x_old, nb))
        return fail("%s: aliased vectors", me);
    if (overlap(j_in, sizeof(int64_t), j_out, sizeof(int64_t)))
        return fail("%s: aliased j_in and j_out", me);
    if (overlap(z, nb, part_gd, pb) || overlap(z, nb, omega, n_omega * (int64_t)sizeof(double)) ||
        overlap(z, nb, j_in, sizeof(int64_t)) || overlap(z, nb, j_out, sizeof(int64_t)))
        return fail("%s: z aliased with an input", me);
    StreamGuard guard(stream);
    hipLaunchKernelGGL(pg_momentum_kernel, dim3(loss_grid(n)), dim3(kLossThreads), 0,
                       (hipStream_t)stream, z, x_new, x_old, n, part_gd, (int)n_part, omega,
                       n_omega, j_in, j_out);
    return check_launch("pg_momentum");
}

// The host refusals the two primal-dual entries share -> the voxel count through n (nothing is
// dereferenced).
static int refuse_pd(const char* me, int nr, int ne, int na, int64_t& n) {
    if (nr < 1 || ne < 1 || na < 1)
        return fail("%s: axis lengths (%d, %d, %d) must be >= 1", me, nr, ne, na);
    n = (int64_t)nr * ne;                      // (< 2^62)
    if (n < ((int64_t)1 << 31)) n *= na;
    if (n >= ((int64_t)1 << 31))
        return fail("%s: the volume must have fewer than 2^31 voxels", me);
    return 0;
}

static PdDesc pd_desc(int nr, int ne, int na, int wrap_a, int has_r, int has_e, int has_a) {
    return PdDesc{(uint32_t)nr, (uint32_t)ne, (uint32_t)na, has_r && nr > 1, has_e && ne > 1,
                  has_a && na > 1, wrap_a && na > 1};
}

// include/sphrt_iso.h: the weights' refusal the two entries share (a NaN fails the compare).
static int refuse_iso_weights(const char* me, const double* w) {
    for (int ax = 0; ax < 3; ++ax)
        if (!(w[ax] >= 0.0) || __builtin_isinf(w[ax]))
            return fail("%s: the weights w_ax must be finite and >= 0, not %g", me, w[ax]);
    return 0;
}

// sphrt_pd_primal_f64, sphrt_dp_primal_f64 (per_voxel: one step per voxel behind `tau`, not one)
// and sphrt_iso_primal_f64 (w: the three weights, null for the other two).
static int pd_primal_entry(const char* me, bool per_voxel, const double* w, const double* x,
                           const double* g, const double* q, double* x_new, int nr, int ne, int na,
                           int wrap_a, int has_r, int has_e, int has_a, double c_damp,
                           const double* tau, double lower, double upper, double* part_mm,
                           void* stream) {
    int64_t n = 0;
    if (int e = refuse_pd(me, nr, ne, na, n)) return e;
    if (!x || !g || !q || !x_new || !tau || !part_mm) return fail("%s: null buffer", me);
    if (w)
        if (int e = refuse_iso_weights(me, w)) return e;
    if (lower != lower || upper != upper || !(lower < upper))
        return fail("%s: bounds need lower < upper, neither NaN (%g, %g)", me, lower, upper);
    const int64_t nb = n * (int64_t)sizeof(double), pb = (int64_t)loss_grid(n) * sizeof(double);
    const void* buf[6] = {x, g, x_new, q, part_mm, tau};
    const int64_t len[6] = {nb, nb, nb, 3 * nb, pb, per_voxel ? nb : (int64_t)sizeof(double)};
    if (int e = refuse_aliased(me, buf, len, 6, 6)) return e;
    StreamGuard guard(stream);
    const PdDesc desc = pd_desc(nr, ne, na, wrap_a, has_r, has_e, has_a);
    const dim3 grid(loss_grid(n)), block(kLossThreads);
    hipStream_t st = (hipStream_t)stream;
    if (w)
        hipLaunchKernelGGL((pd_primal_kernel<false, true>), grid, block, 0, st, x, g, q, x_new,
                           (uint32_t)n, desc, c_damp, tau, lower, upper, part_mm, w[0], w[1], w[2]);
    else if (per_voxel)
        hipLaunchKernelGGL(pd_primal_kernel<true>, grid, block, 0, st, x, g, q, x_new, (uint32_t)n,
                           desc, c_damp, tau, lower, upper, part_mm);
    else
        hipLaunchKernelGGL(pd_primal_kernel<false>, grid, block, 0, st, x, g, q, x_new,
                           (uint32_t)n, desc, c_damp, tau, lower, upper, part_mm);
    return check_launch(w ? "iso_primal" : per_voxel ? "dp_primal" : "pd_primal");
}

extern "C" int sphrt_pd_primal_f64(const double* x, const double* g, const double* q,
                                   double* x_new, int nr, int ne, int na, int wrap_a, int has_r,
                                   int has_e, int has_a, double c_damp, const double* tau,
                                   double lower, double upper, double* part_mm, void* stream) {
    return pd_primal_entry("sphrt_pd_primal_f64", false, nullptr, x, g, q, x_new, nr, ne, na,
                           wrap_a, has_r, has_e, has_a, c_damp, tau, lower, upper, part_mm, stream);
}

extern "C" int sphrt_dp_primal_f64(const double* x, const double* g, const double* q,
                                   double* x_new, int nr, int ne, int na, int wrap_a, int has_r,
                                   int has_e, int has_a, double c_damp, const double* tau,
                                   double lower, double upper, double* part_mm, void* stream) {
    return pd_primal_entry("sphrt_dp_primal_f64", true, nullptr, x, g, q, x_new, nr, ne, na,
                           wrap_a, has_r, has_e, has_a, c_damp, tau, lower, upper, part_mm, stream);
}

extern "C" int sphrt_iso_primal_f64(const double* x, const double* g, const double* q,
                                    double* x_new, int nr, int ne, int na, int wrap_a, double w_r,
                                    double w_e, double w_a, double c_damp, const double* tau,
                                    double lower, double upper, double* part_mm, void* stream) {
    const double w[3] = {w_r, w_e, w_a};
    return pd_primal_entry("sphrt_iso_primal_f64", false, w, x, g, q, x_new, nr, ne, na, wrap_a,
                           w_r > 0.0, w_e > 0.0, w_a > 0.0, c_damp, tau, lower, upper, part_mm,
                           stream);
}

// sphrt_pd_dual_f64 (ax: the clamps c_ax) and sphrt_iso_dual_f64 (iso: ax the weights, and the
// ball's radius).
static int pd_dual_entry(const char* me, bool iso, const double* x_new, const double* x_old,
                         double* q, int nr, int ne, int na, int wrap_a, int has_r, int has_e,
                         int has_a, const double* ax, double radius, const double* sigma,
                         double* part_qq, void* stream) {
    int64_t n = 0;
    if (int e = refuse_pd(me, nr, ne, na, n)) return e;
    if (!x_new || !x_old || !q || !sigma || !part_qq) return fail("%s: null buffer", me);
    if (iso) {
        if (int e = refuse_iso_weights(me, ax)) return e;
        if (!(radius >= 0.0) || __builtin_isinf(radius))
            return fail("%s: the radius must be finite and >= 0, not %g", me, radius);
    } else {
        for (int k = 0; k < 3; ++k)
            if (!(ax[k] >= 0.0) || __builtin_isinf(ax[k]))         // (a NaN fails the compare)
                return fail("%s: the clamps c_ax must be finite and >= 0, not %g", me, ax[k]);
    }
    const int64_t nb = n * (int64_t)sizeof(double), pb = (int64_t)loss_grid(n) * sizeof(double);
    const void* buf[5] = {x_new, x_old, q, part_qq, sigma};
    const int64_t len[5] = {nb, nb, 3 * nb, pb, (int64_t)sizeof(double)};
    if (int e = refuse_aliased(me, buf, len, 5, 5)) return e;
    StreamGuard guard(stream);
    const PdDesc desc = pd_desc(nr, ne, na, wrap_a, has_r, has_e, has_a);
    const dim3 grid(loss_grid(n)), block(kLossThreads);
    if (iso)
        hipLaunchKernelGGL(iso_dual_kernel, grid, block, 0, (hipStream_t)stream, x_new, x_old, q,
                           (uint32_t)n, desc, ax[0], ax[1], ax[2], radius, sigma, part_qq);
    else
        hipLaunchKernelGGL(pd_dual_kernel, grid, block, 0, (hipStream_t)stream, x_new, x_old, q,
                           (uint32_t)n, desc, ax[0], ax[1], ax[2], sigma, part_qq);
    return check_launch(iso ? "iso_dual" : "pd_dual");
}

extern "C" int sphrt_pd_dual_f64(const double* x_new, const double* x_old, double* q, int nr,
                                 int ne, int na, int wrap_a, int has_r, int has_e, int has_a,
                                 double c_r, double c_e, double c_a, const double* sigma,
                                 double* part_qq, void* stream) {
    const double c[3] = {c_r, c_e, c_a};
    return pd_dual_entry("sphrt_pd_dual_f64", false, x_new, x_old, q, nr, ne, na, wrap_a, has_r,
                         has_e, has_a, c, 0.0, sigma, part_qq, stream);
}

extern "C" int sphrt_iso_dual_f64(const double* x_new, const double* x_old, double* q, int nr,
                                  int ne, int na, int wrap_a, double w_r, double w_e, double w_a,
                                  double radius, const double* sigma, double* part_qq,
                                  void* stream) {
    const double w[3] = {w_r, w_e, w_a};
    return pd_dual_entry("sphrt_iso_dual_f64", true, x_new, x_old, q, nr, ne, na, wrap_a,
                         w_r > 0.0, w_e > 0.0, w_a > 0.0, w, radius, sigma, part_qq, stream);
}

template <typename TY, bool PER_RAY>
static void cp_launch(int kind, unsigned grid, hipStream_t st, const double* z_new,
                      const double* z_old, const TY* y, int64_t n, double par,
                      const double* ray_scale, const double* weight, const double* sigma,
                      const int32_t* order, double* p, double* p_adj, double* part_pp,
                      double* part_fid) {
#define SPHRT_CP_CASE(K)                                                                      \
    case K:                                                                                   \
        hipLaunchKernelGGL((cp_ray_dual_kernel<TY, K, PER_RAY>), dim3(grid),                  \
                           dim3(kLossThreads), 0, st, z_new, z_old, y, n, par, ray_scale,     \
                           weight, sigma, order, p, p_adj, part_pp, part_fid);                \
        break;
    switch (kind) {
        SPHRT_CP_CASE(SPHRT_CP_SQUARE)
        SPHRT_CP_CASE(SPHRT_CP_ABS)
        SPHRT_CP_CASE(SPHRT_CP_HUBER)
        SPHRT_CP_CASE(SPHRT_CP_POISSON)
    }
#undef SPHRT_CP_CASE
}

// sphrt_cp_ray_dual_f64 and sphrt_dp_ray_dual_f64: one step behind `sigma`, or one per ray.
template <bool PER_RAY>
static int cp_ray_dual_entry(const char* me, const double* z_new, const double* z_old,
                             const void* y, int y_is_f64, int64_t n, int kind,
                             double delta_or_eps, const double* ray_scale, const double* weight,
                             const double* sigma, const int32_t* order, double* p, double* p_adj,
                             double* part_pp, double* part_fid, void* stream) {
    if (n <= 0) return fail("%s: empty measurement (n %lld)", me, (long long)n);
    if (kind < SPHRT_CP_SQUARE || kind > SPHRT_CP_POISSON)
        return fail("%s: unknown kind %d (SPHRT_CP_SQUARE .. SPHRT_CP_POISSON)", me, kind);
    double par = 0.0;
    if (kind == SPHRT_CP_HUBER) {
        if (int e = refuse_robust(SPHRT_RESID_HUBER, delta_or_eps, par)) return e;
    } else if (kind == SPHRT_CP_POISSON) {
        if (int e = refuse_poisson(delta_or_eps)) return e;
        par = delta_or_eps;
    }
    if (!z_new || !z_old || !y || !ray_scale || !weight || !sigma || !p || !part_pp || !part_fid)
        return fail("%s: null buffer", me);
    if ((order == nullptr) != (p_adj == nullptr))
        return fail("%s: null buffer (order and p_adj go together)", me);
    const int64_t nb = n * (int64_t)sizeof(double), pb = (int64_t)loss_grid(n) * sizeof(double);
    const void* buf[11] = {p, p_adj, part_pp, part_fid, z_new, z_old, y, ray_scale, weight,
                           sigma, order};
    const int64_t len[11] = {nb, nb, pb, pb, nb, nb, y_is_f64 ? nb : nb / 2, nb, nb,
                             PER_RAY ? nb : (int64_t)sizeof(double),
                             n * (int64_t)sizeof(int32_t)};
    if (int e = refuse_aliased(me, buf, len, 4, 11)) return e;   // (p, p_adj and the partial sums)
    StreamGuard guard(stream);
    hipStream_t st = (hipStream_t)stream;
    if (y_is_f64)
        cp_launch<double, PER_RAY>(kind, loss_grid(n), st, z_new, z_old, (const double*)y, n, par,
                                   ray_scale, weight, sigma, order, p, p_adj, part_pp, part_fid);
    else
        cp_launch<float, PER_RAY>(kind, loss_grid(n), st, z_new, z_old, (const float*)y, n, par,
                                  ray_scale, weight, sigma, order, p, p_adj, part_pp, part_fid);
    return check_launch(PER_RAY ? "dp_ray_dual" : "cp_ray_dual");
}

extern "C" int sphrt_cp_ray_dual_f64(const double* z_new, const double* z_old, const void* y,
                                     int y_is_f64, int64_t n, int kind, double delta_or_eps,
                                     const double* ray_scale, const double* weight,
                                     const double* sigma, const int32_t* order, double* p,
                                     double* p_adj, double* part_pp, double* part_fid,
                                     void* stream) {
    return cp_ray_dual_entry<false>("sphrt_cp_ray_dual_f64", z_new, z_old, y, y_is_f64, n, kind,
                                    delta_or_eps, ray_scale, weight, sigma, order, p, p_adj,
                                    part_pp, part_fid, stream);
}

extern "C" int sphrt_dp_ray_dual_f64(const double* z_new, const double* z_old, const void* y,
                                     int y_is_f64, int64_t n, int kind, double delta_or_eps,
                                     const double* ray_scale, const double* weight,
                                     const double* sigma, const int32_t* order, double* p,
                                     double* p_adj, double* part_pp, double* part_fid,
                                     void* stream) {
    return cp_ray_dual_entry<true>("sphrt_dp_ray_dual_f64", z_new, z_old, y, y_is_f64, n, kind,
                                   delta_or_eps, ray_scale, weight, sigma, order, p, p_adj,
                                   part_pp, part_fid, stream);
}

extern "C" int sphrt_dp_steps_f64(const double* col, const double* row, int64_t n_ray, int nr,
                                  int ne, int na, int wrap_a, int has_r, int has_e, int has_a,
                                  double rho, double c, const int32_t* order, double* tau,
                                  double* sigma, void* stream) {
    const char* me = "sphrt_dp_steps_f64";
    int64_t n_vox = 0;
    if (int e = refuse_pd(me, nr, ne, na, n_vox)) return e;
    if (n_ray < 1 || n_ray >= ((int64_t)1 << 31))
        return fail("%s: n_ray %lld, the measurement must have 1 .. 2^31 - 1 rays", me,
                    (long long)n_ray);
    if (!(rho > 0.0) || __builtin_isinf(rho))                   // (a NaN fails the compare)
        return fail("%s: rho must be finite and > 0, not %g", me, rho);
    if (!(c >= 0.0) || __builtin_isinf(c))
        return fail("%s: c must be finite and >= 0, not %g", me, c);
    if (!col || !row || !tau || !sigma) return fail("%s: null buffer", me);
    const int64_t vb = n_vox * (int64_t)sizeof(double), rb = n_ray * (int64_t)sizeof(double);
    const void* buf[5] = {tau, sigma, col, row, order};
    const int64_t len[5] = {vb, rb, vb, rb, n_ray * (int64_t)sizeof(int32_t)};
    if (int e = refuse_aliased(me, buf, len, 2, 5)) return e;    // (tau and sigma)
    StreamGuard guard(stream);
    hipLaunchKernelGGL(dp_steps_kernel, dim3(loss_grid(n_vox > n_ray ? n_vox : n_ray)),
                       dim3(kLossThreads), 0, (hipStream_t)stream, col, row, (uint32_t)n_vox,
                       (uint32_t)n_ray, pd_desc(nr, ne, na, wrap_a, has_r, has_e, has_a), rho, c,
                       order, tau, sigma);
    return check_launch("dp_steps");
}
