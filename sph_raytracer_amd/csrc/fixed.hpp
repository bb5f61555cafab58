// fixed.hpp — the fixed-point accumulator of the deterministic matrix-free adjoint, host and
// device (the host mirrors of sphrt.h, sphrt_fixed_*_host, are these functions).
//
// Every term of a sum is quantised onto one power-of-two grid and added as an integer, so the
// sum does not depend on the order of the adds: not on the ray order, the workgroup schedule or
// the way a batch is split over calls.
//
//   exponent   a bound B >= |term| of every term, finite and > 0; frexp(B) = f * 2^E with f in
//              [0.5, 1).  The quantum is q = 2^(E - 61): B itself is a rounded product, so one
//              bit of margin is left below int64's 63 (|k| <= 2^61, a term an ulp above B fits).
//   quantise   k = llrint(ldexp(term, 61 - E)), round half to even.  ldexp, not a product with
//              2^(61 - E), which need not be representable.  (Terms above the bound:
//              fixed_quantise below.)
//   split      carry-save: a voxel owns two adjacent int64 {lo, hi} (16 bytes, one line);
//              lo += k & 0xffffffff, hi += k >> 32 (arithmetic), the voxel's integer is
//              V = hi * 2^32 + lo.  Both are plain integer sums (no carry detection), so
//              accumulators filled under one record can be summed elementwise.
//              Capacity: fewer than 2^31 adds per voxel over an accumulator's lifetime
//              (lo < 2^31 * 2^32 = 2^63; |hi| < 2^31 * 2^29); the trace entries refuse batches
//              of n_rays * max(n_chan, 1) >= 2^29.
//   value      ldexp(D, E - 61) with D = V converted to double correctly rounded, ties to even
//              (Python's float(int)): the up-to-96-bit magnitude normalised to its top 64 bits,
//              a sticky bit in bit 0, then the hardware u64 -> f64 conversion (no __int128).
//   record     16 bytes in device memory, {int32 E, int32 flags, 8 bytes pad}.  flags bit 0: the
//              bound was zero (nothing is added, every value is +0.0); bit 1: the bound was not
//              finite (nothing is added, every value is NaN — the whole result, where the
//              float64-atomic path poisons only the voxels it touches: no host sync finds out).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace sphrt {

constexpr int kFixedBits = 61;          // the largest term's magnitude, in quanta: <= 2^61
constexpr int32_t kFixedZero = 1;       // flags: the bound was zero
constexpr int32_t kFixedNonFinite = 2;  // flags: the bound was inf or NaN

struct FixedScale {     // the record's first 8 bytes
    int32_t E, flags;
};

// The record of a bound B (>= 0, or not finite).
__host__ __device__ inline FixedScale fixed_exponent(double B) {
    FixedScale s{0, 0};
    if (!(fabs(B) <= 1.7976931348623157e308)) {     // inf, NaN
        s.flags = kFixedNonFinite;
    } else if (B == 0.0) {
        s.flags = kFixedZero;
    } else {
        int e;
        (void)frexp(B, &e);
        s.E = e;
    }
    return s;
}

// term in quanta of 2^(E - 61), shift = 61 - E, split: k = rint(ldexp(term, shift)) (half to
// even), lo = k & 0xffffffff, hi = k >> 32 (arithmetic: floor(k / 2^32)).  The split is done on
// the integer-valued double (every step exact), which for |k| <= 2^61 is bit for bit
// llrint + mask + shift and also holds beyond int64: a term above the bound — the trace's head
// segment, which runs back from a start inside the grid to the farthest crossing behind it, can
// be many diameters long — is still added exactly, up to 2^32 times the bound (|k| < 2^93); it
// takes that many times more of hi's capacity (the sum of |hi| must stay below 2^63).
__host__ __device__ inline void fixed_quantise(double term, int shift, int64_t& lo, int64_t& hi) {
    const double k = rint(ldexp(term, shift));
    const double h = floor(ldexp(k, -32));
    hi = (int64_t)h;
    lo = (int64_t)(k - h * 4294967296.0);
}

// acc element idx += term, on the device: the term in quanta of 2^-shift, split, as two 64-bit
// integer atomics without return on the element's {lo, hi} pair (the trace's *_FIXED adds and
// sphrt_fixed_accumulate_f64).
__device__ __forceinline__ void fixed_accumulate(int64_t* acc, int64_t idx, double term, int shift) {
    int64_t lo, hi;
    fixed_quantise(term, shift, lo, hi);
    unsigned long long* p = reinterpret_cast<unsigned long long*>(acc) + 2 * idx;
    atomicAdd(p, (unsigned long long)lo);
    atomicAdd(p + 1, (unsigned long long)hi);
}

__host__ __device__ inline int fixed_clz64(uint64_t x) {   // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// V = hi * 2^32 + lo as a double, correctly rounded (ties to even), times 2^(E - 61).
__host__ __device__ inline double fixed_value(int64_t lo, int64_t hi, FixedScale s) {
    if (s.flags & kFixedNonFinite) return NAN;
    if (s.flags & kFixedZero) return 0.0;
    // the 128-bit two's complement V = (vh, vl)
    const uint64_t a = (uint64_t)hi << 32;
    uint64_t vl = a + (uint64_t)lo;
    uint64_t vh = (uint64_t)(hi >> 32) + (uint64_t)(lo >> 63) + (vl < a ? 1u : 0u);
    const bool negative = (int64_t)vh < 0;
    if (negative) {
        vl = ~vl + 1;
        vh = ~vh + (vl == 0 ? 1u : 0u);
    }
    double d;
    if (vh == 0) {
        d = (double)vl;
    } else {
        // the top 64 bits of the magnitude, what is shifted out OR-ed into bit 0: the bit the
        // conversion rounds at is bit 11 of 64, so a sticky bit 0 decides ties as the lost bits would
        const int sh = 64 - fixed_clz64(vh);      // 1 .. 64
        const uint64_t top = sh == 64 ? vh : (vh << (64 - sh)) | (vl >> sh);
        const uint64_t lost = sh == 64 ? vl : vl << (64 - sh);
        d = ldexp((double)(top | (lost != 0 ? 1u : 0u)), sh);
    }
    return ldexp(negative ? -d : d, s.E - kFixedBits);
}

}  // namespace sphrt
