// common.hpp — plan object, ray-batch descriptor and error plumbing shared by the .hip units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "sphrt.h"
#include "solve.hpp"

struct sphrt_plan {
    int device;
    sphrt::GridDev dev;   // device pointers below
    void* table_mem;      // one hipMalloc holding every boundary table
};

namespace sphrt {

constexpr int kMaxDims = SPHRT_MAX_DIMS;

struct RaysDev {
    int ndim;
    int64_t n;
    int64_t shape[kMaxDims];
    int64_t xs_stride[kMaxDims];
    int64_t rays_stride[kMaxDims];
    const double* xs;
    const double* rays;
    const int32_t* start;
    int fresh;    // reference-mode trace: each solver normalises its own copy (exact_list)
};

int fail(const char* fmt, ...);   // records the message, returns -1
int check_launch(const char* what);

// Makes `dev` the calling thread's current HIP device for the scope (restored afterwards).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        int cur = -1;
        if (dev < 0 || hipGetDevice(&cur) != hipSuccess || cur == dev) return;
        if (hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Device a stream belongs to (the current device for the null stream), -1 on error.
inline int stream_device(void* stream) {
    int dev = -1;
    if (stream == nullptr) return hipGetDevice(&dev) == hipSuccess ? dev : -1;
    hipDevice_t d;
    return hipStreamGetDevice((hipStream_t)stream, &d) == hipSuccess ? (int)d : -1;
}

// Every launching entry point runs on its stream's device, whatever device is current in the
// calling thread (the caller's buffers live on that device too).
struct StreamGuard {
    DeviceGuard g;
    explicit StreamGuard(void* stream) : g(stream_device(stream)) {}
};

// The robust residuals (SPHRT_RESID_*): psi of the residual r, shared by the trace's sink and the
// loss tail.  delta > 0: r clamped to [-delta, delta] (HUBER; a NaN fails both compares and
// passes through, as in torch's huber_loss backward).  delta == 0: the sign of r, -1, 0 or +1
// (ABS; +-0 and NaN give +0: torch.sign's (0 < r) - (r < 0)).
__device__ __forceinline__ double robust_psi(double r, double delta) {
    if (delta > 0.0) return r < -delta ? -delta : (r > delta ? delta : r);
    return (double)((int)(0.0 < r) - (int)(r < 0.0));
}
// The robust entries' own host refusals: an unknown kind, and for HUBER a delta that is not
// finite and > 0.  -> the delta robust_psi takes in `rd` (0 for ABS).
inline int refuse_robust(int kind, double delta, double& rd) {
    rd = 0.0;
    if (kind == SPHRT_RESID_ABS) return 0;
    if (kind != SPHRT_RESID_HUBER)
        return fail("unknown residual kind %d (SPHRT_RESID_ABS or SPHRT_RESID_HUBER)", kind);
    if (!(delta > 0.0) || __builtin_isinf(delta))   // (a NaN fails the compare)
        return fail("the Huber delta must be finite and > 0, not %g", delta);
    rd = delta;
    return 0;
}

// The Poisson fidelity (PoissonLoss: p - y * log(p + eps), torch's poisson_nll_loss with
// log_input=False), shared by the trace's sink and the loss tail.  q = p + eps, one rounding.
// poisson_weight: the gradient autograd leaves at p for an incoming gradient s — the sub, mul
// and log backward of ATen's composite input - target * log(input + eps): s + ((-s) * y) / q.
// Plain multiplies and a plain division, whatever -ffp-contract says; no guards: q <= 0, inf and
// NaN give what IEEE gives, as in torch.
__device__ __forceinline__ double poisson_weight(double q, double y, double s) {
#pragma clang fp contract(off)
    const double t = (-s) * y;
    const double u = t / q;
    return s + u;
}
// The Poisson entries' own host refusal: an eps that is not finite and > 0.
inline int refuse_poisson(double eps) {
    if (!(eps > 0.0) || __builtin_isinf(eps))       // (a NaN fails the compare)
        return fail("the Poisson eps must be finite and > 0, not %g", eps);
    return 0;
}

// Validate plan + batch and convert to the by-value kernel argument forms.
inline int resolve(const sphrt_plan* plan, const sphrt_rays* rays, GridDev& G, RaysDev& R,
                   void* stream) {
    if (!plan) return fail("null plan");
    const int sdev = stream_device(stream);
    if (sdev != plan->device)
        return fail("stream is on device %d but the plan's tables are on device %d", sdev,
                    plan->device);
    if (!rays) return fail("null ray batch");
    if (rays->ndim < 0 || rays->ndim > kMaxDims) return fail("ray batch rank %d out of range", rays->ndim);
    if (!rays->xs || !rays->rays || !rays->start) return fail("null ray batch pointer");
    G = plan->dev;
    R.ndim = rays->ndim;
    R.n = 1;
    for (int d = 0; d < kMaxDims; ++d) {
        R.shape[d] = d < rays->ndim ? rays->shape[d] : 1;
        R.xs_stride[d] = d < rays->ndim ? rays->xs_stride[d] : 0;
        R.rays_stride[d] = d < rays->ndim ? rays->rays_stride[d] : 0;
        if (d < rays->ndim) {
            if (rays->shape[d] < 0) return fail("negative ray-batch extent");
            R.n *= rays->shape[d];
        }
    }
    R.xs = rays->xs;
    R.rays = rays->rays;
    R.start = rays->start;
    R.fresh = 0;
    return 0;
}

}  // namespace sphrt
