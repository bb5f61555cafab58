// fixed.hip — the scale record and the finalize pass of the fixed-point accumulator (fixed.hpp),
// and the host mirrors of its arithmetic.  The adds themselves are the trace's (trace.hip,
// MODE_SCATTER_FIXED / MODE_NORMAL_FIXED); sphrt_fixed_accumulate_f64 runs the same device add on
// a caller's list of terms.
#include "common.hpp"
#include "fixed.hpp"

namespace sphrt {

// max |x_i| as the largest bit pattern of |x|: the pattern orders non-negative doubles, and a
// NaN's sorts above infinity's, so one NaN makes the bound non-finite.  One atomic per wave.
__global__ __launch_bounds__(256) void fixed_max_kernel(const double* __restrict__ x, int64_t n,
                                                        unsigned long long* cell) {
    unsigned long long m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned long long b =
            (unsigned long long)__double_as_longlong(x[i]) & 0x7fffffffffffffffull;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long u = __shfl_xor(m, off);
        m = u > m ? u : m;
    }
    if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(cell, m);
}

// One thread: B = fa * max|a| + fb * max|b| from the two cells (the record's own 16 bytes), then
// the record over them.
__global__ void fixed_record_kernel(unsigned long long* rec, double fa, double fb, int have_b) {
    const double ma = __longlong_as_double((long long)rec[0]);
    const double mb = __longlong_as_double((long long)rec[1]);
    double B = fa * ma;
    if (have_b) B += fb * mb;
    const FixedScale s = fixed_exponent(B);
    int32_t* out = reinterpret_cast<int32_t*>(rec);
    out[0] = s.E;
    out[1] = s.flags;
    rec[1] = 0;
}

__global__ __launch_bounds__(256) void fixed_finalize_kernel(const longlong2* __restrict__ acc,
                                                             int64_t n, const int32_t* rec,
                                                             double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const FixedScale s{rec[0], rec[1]};
    const longlong2 v = acc[i];
    out[i] = fixed_value((int64_t)v.x, (int64_t)v.y, s);
}

// acc element index[i] += terms[i], one thread per term, as the trace adds a segment's term
// (fixed_accumulate); nothing when the record's flags are set.
__global__ __launch_bounds__(256) void fixed_accumulate_kernel(const double* __restrict__ terms,
                                                               const int64_t* __restrict__ index,
                                                               int64_t n, const int32_t* rec,
                                                               int64_t* acc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || rec[1] != 0) return;
    fixed_accumulate(acc, index[i], terms[i], kFixedBits - rec[0]);
}

}  // namespace sphrt

using namespace sphrt;

extern "C" int sphrt_fixed_scale_f64(const double* a, int64_t na, double fa, const double* b,
                                     int64_t nb, double fb, void* scale_rec, void* stream) {
    if (!scale_rec) return fail("null scale record");
    if (na < 0 || nb < 0) return fail("negative scale length");
    if ((!a && na > 0) || (!b && nb > 0)) return fail("null scale input with a non-zero length");
    if (!(fa >= 0.0) || (b && !(fb >= 0.0)))      // (NaN too; +inf makes the bound non-finite)
        return fail("negative or NaN scale factor");
    StreamGuard guard(stream);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* rec = (unsigned long long*)scale_rec;
    if (hipMemsetAsync(rec, 0, 16, st) != hipSuccess) return fail("memset failed");
    const struct { const double* x; int64_t n; int cell; } in[2] = {{a, na, 0}, {b, nb, 1}};
    for (const auto& v : in) {
        if (!v.x || v.n == 0) continue;
        int64_t g = (v.n + 2047) / 2048;      // 8 values per thread, at most 1024 workgroups
        g = g > 1024 ? 1024 : g;
        hipLaunchKernelGGL(fixed_max_kernel, dim3((unsigned)g), dim3(256), 0, st, v.x, v.n,
                           rec + v.cell);
        if (int e = check_launch("fixed_max_kernel")) return e;
    }
    hipLaunchKernelGGL(fixed_record_kernel, dim3(1), dim3(1), 0, st, rec, fa, fb, b ? 1 : 0);
    return check_launch("fixed_record_kernel");
}

extern "C" int sphrt_fixed_finalize_f64(const int64_t* acc, int64_t n_elems, const void* scale_rec,
                                        double* out, void* stream) {
    if (!scale_rec) return fail("null scale record");
    if (n_elems < 0) return fail("negative finalize length");
    if (n_elems == 0) return 0;
    if (!acc || !out) return fail("null finalize argument (acc or out)");
    const int64_t blocks = (n_elems + 255) / 256;
    if (blocks > INT32_MAX) return fail("finalize too large");
    StreamGuard guard(stream);
    hipLaunchKernelGGL(fixed_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const longlong2*>(acc), n_elems,
                       reinterpret_cast<const int32_t*>(scale_rec), out);
    return check_launch("fixed_finalize_kernel");
}

extern "C" int sphrt_fixed_accumulate_f64(const double* terms, const int64_t* index, int64_t n,
                                          const void* scale_rec, int64_t* acc, void* stream) {
    if (!scale_rec) return fail("null scale record");
    if (n < 0) return fail("negative accumulate length");
    if (n == 0) return 0;
    if (!terms || !index || !acc) return fail("null accumulate argument (terms, index or acc)");
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return fail("accumulate too large");
    StreamGuard guard(stream);
    hipLaunchKernelGGL(fixed_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, terms, index, n,
                       reinterpret_cast<const int32_t*>(scale_rec), acc);
    return check_launch("fixed_accumulate_kernel");
}

extern "C" int sphrt_fixed_exponent_host(double bound, int32_t* E, int32_t* flags) {
    if (!E || !flags) return fail("null exponent output");
    if (bound < 0.0) return fail("negative bound");
    const FixedScale s = fixed_exponent(bound);
    *E = s.E;
    *flags = s.flags;
    return 0;
}

extern "C" void sphrt_fixed_quantise_host(double term, int32_t E, int64_t lo_hi[2]) {
    fixed_quantise(term, kFixedBits - E, lo_hi[0], lo_hi[1]);
}

extern "C" double sphrt_fixed_value_host(int64_t lo, int64_t hi, int32_t E, int32_t flags) {
    return fixed_value(lo, hi, FixedScale{E, flags});
}
