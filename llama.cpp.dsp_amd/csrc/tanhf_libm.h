// tanhf_libm.h -- the host C library's tanhf restated operation for operation, for the soft-cap of the CPU-exact attention kernels: the reference CPU
// backend computes `softcap * tanhf(s)` with the C library (ggml-cpu/ops.cpp:6803), and the device library's tanhf is not that function bit for bit.
// This is the classic fdlibm single-precision form (s_tanhf.c over s_expm1f.c, as the GNU C library ships it for x86-64 up to 2.40: scalar, no fused
// multiply-add): every product, sum and quotient below is ONE rounded f32 operation, in the order written.  Nothing may be contracted: the pragma holds
// that under every -ffp-contract mode that honours pragmas (the library is built with `off`; `fast` on a host compiler would ignore it).  (What expf_libm of mi355q_common.h is to expf.)  Plain C++: it compiles for the host too, where a
// stand-alone program can hold it against the C library.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TANHF_LIBM_FN __host__ __device__ inline
#else
#define TANHF_LIBM_FN inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define TANHF_LIBM_DIV(a, b) __fdiv_rn((a), (b))      // the correctly rounded quotient whatever the division flags say
#else
#define TANHF_LIBM_DIV(a, b) ((a) / (b))
#endif

namespace mi355q {

TANHF_LIBM_FN uint32_t tl_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
TANHF_LIBM_FN float tl_float(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

// expm1f (s_expm1f.c) for the arguments tanhf passes: 2 |x| in [2, 44) and -2 |x| in (-2, 0); finite, no overflow
TANHF_LIBM_FN float expm1f_libm(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float ln2_hi = 6.9313812256e-01f, ln2_lo = 9.0580006145e-06f, invln2 = 1.4426950216e+00f;     // 0x3f317180, 0x3717f7d1, 0x3fb8aa3b
    const float Q1 = -3.3333335072e-02f, Q2 = 1.5873016091e-03f, Q3 = -7.9365076090e-05f, Q4 = 4.0082177293e-06f, Q5 = -2.0109921195e-07f;
    float y, hi, lo, c = 0.0f, t, e, hxs, hfx, r1;
    int32_t k;
    uint32_t hx = tl_bits(x);
    const bool neg = (hx & 0x80000000u) != 0;
    hx &= 0x7fffffffu;
    if (hx >= 0x4195b844u && neg) return 1.0e-30f - 1.0f;            // x < -27 ln2 (not reached from tanhf)
    if (hx > 0x3eb17218u) {                                          // |x| > 0.5 ln2: argument reduction
        if (hx < 0x3F851592u) {                                      // and |x| < 1.5 ln2
            if (!neg) { hi = x - ln2_hi; lo = ln2_lo; k = 1; }
            else      { hi = x + ln2_hi; lo = -ln2_lo; k = -1; }
        } else {
            k = (int32_t) (invln2 * x + (neg ? -0.5f : 0.5f));
            t = (float) k;
            hi = x - t * ln2_hi;                                     // (t * ln2_hi is exact here)
            lo = t * ln2_lo;
        }
        x = hi - lo;
        c = (hi - x) - lo;
    } else if (hx < 0x33000000u) {                                   // |x| < 2^-25: x
        return x;
    } else k = 0;
    hfx = 0.5f * x;
    hxs = x * hfx;
    r1 = 1.0f + hxs * (Q1 + hxs * (Q2 + hxs * (Q3 + hxs * (Q4 + hxs * Q5))));
    t = 3.0f - r1 * hfx;
    e = hxs * TANHF_LIBM_DIV(r1 - t, 6.0f - x * t);
    if (k == 0) return x - (x * e - hxs);
    e = (x * (e - c) - c);
    e -= hxs;
    if (k == -1) return 0.5f * (x - e) - 0.5f;
    if (k == 1) {
        if (x < -0.25f) return -2.0f * (e - (x + 0.5f));
        return 1.0f + 2.0f * (x - e);
    }
    if (k <= -2 || k > 56) {                                         // suffice to return exp(x) - 1
        y = 1.0f - (e - x);
        y = tl_float(tl_bits(y) + ((uint32_t) k << 23));
        return y - 1.0f;
    }
    if (k < 23) {
        t = tl_float(0x3f800000u - (0x1000000u >> k));               // 1 - 2^-k
        y = t - (e - x);
        y = tl_float(tl_bits(y) + ((uint32_t) k << 23));
    } else {
        t = tl_float((uint32_t) (0x7f - k) << 23);                   // 2^-k
        y = x - (e + t);
        y += 1.0f;
        y = tl_float(tl_bits(y) + ((uint32_t) k << 23));
    }
    return y;
}

TANHF_LIBM_FN float tanhf_libm(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float t, z;
    const uint32_t jx = tl_bits(x), ix = jx & 0x7fffffffu;
    const float ax = tl_float(ix);
    if (ix >= 0x7f800000u) {                                         // tanh(+-inf) = +-1, tanh(NaN) = NaN
        if ((jx & 0x80000000u) == 0) return TANHF_LIBM_DIV(1.0f, x) + 1.0f;
        return TANHF_LIBM_DIV(1.0f, x) - 1.0f;
    }
    if (ix < 0x41b00000u) {                                          // |x| < 22
        if (ix == 0) return x;
        if (ix < 0x24000000u) return x * (1.0f + x);                 // |x| < 2^-55
        if (ix >= 0x3f800000u) {                                     // |x| >= 1
            t = expm1f_libm(2.0f * ax);
            z = 1.0f - TANHF_LIBM_DIV(2.0f, t + 2.0f);
        } else {
            t = expm1f_libm(-2.0f * ax);
            z = TANHF_LIBM_DIV(-t, t + 2.0f);
        }
    } else z = 1.0f - 1.0e-30f;                                      // |x| >= 22: 1 (raised inexact)
    return (jx & 0x80000000u) == 0 ? z : -z;
}

} // namespace mi355q
