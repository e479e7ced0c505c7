// fa_quant.cuh -- the per-position arithmetic of FLASH_ATTN_EXT over a quantized KV cache (Q8_0, Q4_0, Q4_1, Q5_0, Q5_1, IQ4_NL), shared by the
// residency op (ops_glue.hip k_flash_attn_ext_q80, k_mul_mat_kvq, k_cpy_f32_kvq) and the decode plan's attention stage (plan.hip
// plan_attn_q80), so that the two give the same bits by construction (DESIGN.md sections 5.6, 5.7e).  The CPU's order (ggml-cpu/ops.cpp:6686-6905):
//   cache stores   f32 -> block (the type's from_float = quantize_row_<type>_ref), what CPY f32 -> type writes
//   q              quantized to the K type's vec_dot_type by the SIMD quantizer (round half to even): Q8_0; Q8_1 (+ s = f16(d * sum q)) for Q4_1 / Q5_1
//   scores         ggml_vec_dot_<type>_q8_0 / _q8_1 in their AVX2 order
//   softmax        walked in position order with a running maximum (expf_libm: the host library's expf)
//   V . P          V dequantized (dequantize_row_<type>) into an F32 accumulator: ggml_vec_scale_f32 when the maximum grows, ggml_vec_mad_f32 per position
// Cache blocks are 2-byte aligned (34 / 18 / 20 / 22 / 24 bytes): they are read and written as halves of words.
//   Q8_0 34: f16 d, 32 int8          Q4_0 18: f16 d, 16 B nibbles        Q4_1 20: f16 d, f16 m, 16 B nibbles
//   Q5_0 22: f16 d, 4 B qh, nibbles  Q5_1 24: f16 d, f16 m, 4 B qh, nibbles     IQ4_NL 18: f16 d, 16 B code-book indices (kvalues_iq4nl)
// (nibbles: low = elements 0..15, high = 16..31; qh bit j = the fifth bit of element j)
#pragma once
#include "mi355q_common.h"
#include "act_quant.cuh"

namespace mi355q {

#ifdef __HIPCC__

template <int KVT> __host__ __device__ constexpr int kv_block_bytes() {
    return KVT == MI355Q_TYPE_Q8_0 ? 34 : KVT == MI355Q_TYPE_Q4_1 ? 20 : KVT == MI355Q_TYPE_Q5_0 ? 22 : KVT == MI355Q_TYPE_Q5_1 ? 24 : 18;
}
template <int KVT> __host__ __device__ constexpr bool kv_has_min() { return KVT == MI355Q_TYPE_Q4_1 || KVT == MI355Q_TYPE_Q5_1; }     // f16 m after d; q is quantized to Q8_1
template <int KVT> __host__ __device__ constexpr bool kv_has_qh()  { return KVT == MI355Q_TYPE_Q5_0 || KVT == MI355Q_TYPE_Q5_1; }     // 4 bytes of fifth bits before the nibbles
template <int KVT> __host__ __device__ constexpr int  kv_qs_off()  { return 2 + (kv_has_min<KVT>() ? 2 : 0) + (kv_has_qh<KVT>() ? 4 : 0); }
// bytes per block by run-time type (0: not a cache block type)
__host__ __device__ inline int kv_block_bytes_rt(int t) {
    return t == MI355Q_TYPE_Q8_0 ? 34 : t == MI355Q_TYPE_Q4_0 ? 18 : t == MI355Q_TYPE_Q4_1 ? 20 : t == MI355Q_TYPE_Q5_0 ? 22 : t == MI355Q_TYPE_Q5_1 ? 24 : t == MI355Q_TYPE_IQ4_NL ? 18 : 0;
}

__device__ __forceinline__ uint32_t ld_w16(const char * p) { return (uint32_t) *(const uint16_t *) p | ((uint32_t) *(const uint16_t *) (p + 2) << 16); }     // a word at a 2-byte aligned address
// four fifth bits (bits 0..3 of b) -> bit 4 of the four bytes of a word (bit i lands on 8 i: the partial products of 1 + 2^7 + 2^14 + 2^21 do not meet)
__device__ __forceinline__ uint32_t kv_spread4(uint32_t b) { return (((b & 0xFu) * 0x00204081u) & 0x01010101u) << 4; }

// best_index_int8 over kvalues_iq4nl (ggml-quants.c:4562-4571): the nearer neighbour, the upper one on a tie, the two distances in f32
__device__ __forceinline__ int iq4nl_best_index(float x) {
    if (x <= -127.0f) return 0;
    if (x >= 113.0f) return 15;
    int ml = 0;
    constexpr float val[16] = { -127.f, -104.f, -83.f, -65.f, -49.f, -35.f, -22.f, -10.f, 1.f, 13.f, 25.f, 38.f, 53.f, 69.f, 89.f, 113.f };
#pragma unroll
    for (int i = 1; i < 15; ++i) ml += !(x < val[i]) ? 1 : 0;                    // the binary search's ml: the last entry <= x
    float below = val[0], above = val[1];
#pragma unroll
    for (int i = 1; i < 15; ++i) if (ml == i) { below = val[i]; above = val[i + 1]; }
    return __fsub_rn(x, below) < __fsub_rn(above, x) ? ml : ml + 1;
}

// ---- f32 -> one cache block: eight lanes own a block, lane l (= lane & 7) the elements 4l .. 4l+3 (every lane of the wave must take part: the
// group reductions).  w: Q8_0 -- the four int8 quants of the lane; the nibble types -- lanes 0..3: the four nibble bytes j = 4l .. 4l+3
// (q[j] | q[j + 16] << 4).  d (and m, qh where the type has them) are valid in every lane of the group.
//   Q8_0   quantize_row_q8_0_ref (round half away from zero)
//   Q4_0   quantize_row_q4_0_ref (ggml-quants.c:31-66): max = the FIRST element of largest magnitude, signed; d = max / -8; q = min(15, (int8) (x / d + 8.5))
//   Q4_1   quantize_row_q4_1_ref (:68-103): d = (max - min) / 15, m = min, q = min(15, (int8) ((x - min) / d + 0.5))
//   Q5_0   quantize_row_q5_0_ref (:105-147): as Q4_0 with -16, 16.5 and 31; the fifth bits go to qh
//   Q5_1   quantize_row_q5_1_ref (:149-191): d = (max - min) / 31, q = (uint8) ((x - min) / d + 0.5)
//   IQ4_NL quantize_row_iq4_nl_ref (:4707 -> quantize_row_iq4_nl_impl :4573, ntry = -1, no weights): d0 = max / -127, one best_index_int8 pass with
//          1 / d0, d = sumqx / sumq2 with w = x^2 -- two sequential f32 sums over the 32 elements, nothing contracted (ggml-quants.c is built as
//          ISO C) --, the indices of that pass are kept.  amax < GROUP_MAX_EPS: d = 0 and zero index bytes (the CPU's bytes are undefined there).
// (1 / d is taken as the CPU takes it: `d ? 1.0f / d : 0.0f`.)
struct KvBlk { uint32_t w; float d; float m; uint32_t qh; };
template <int KVT>
__device__ __forceinline__ void kv_quant_group8(const float4 v, KvBlk & o) {
    o.m = 0.0f; o.qh = 0u;
    if constexpr (KVT == MI355Q_TYPE_Q8_0) {
        int sum;
        q80_group8<false>(v, o.w, o.d, sum);
    } else {
        const int lane = (int) (threadIdx.x & 63);
        const float x[4] = { v.x, v.y, v.z, v.w };
        int qi[4];
        if constexpr (kv_has_min<KVT>()) {
            constexpr float LEVELS = KVT == MI355Q_TYPE_Q4_1 ? 15.0f : 31.0f;
            const float mn = -oct_max(-fminf(fminf(x[0], x[1]), fminf(x[2], x[3]))), mx = oct_max(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
            o.d = __fdiv_rn(__fsub_rn(mx, mn), LEVELS); o.m = mn;
            const float id = o.d != 0.0f ? __fdiv_rn(1.0f, o.d) : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = (int) __fadd_rn(__fmul_rn(__fsub_rn(x[i], mn), id), 0.5f);
                qi[i] = KVT == MI355Q_TYPE_Q4_1 ? min(15, t) : (t & 0xFF);
            }
        } else {
            float amax = 0.0f, mxv = 0.0f;                         // this lane's first element of largest magnitude
#pragma unroll
            for (int i = 0; i < 4; ++i) if (amax < fabsf(x[i])) { amax = fabsf(x[i]); mxv = x[i]; }
            const float gmax = oct_max(amax);                        // the block's largest magnitude; its first holder is the lowest lane that has it
            const unsigned long long holders = __ballot(amax == gmax);
            const int first = __ffs((int) ((holders >> (lane & ~7)) & 0xFFull)) - 1;
            const float bmax = __shfl(mxv, (lane & ~7) + first, 64);
            if constexpr (KVT == MI355Q_TYPE_IQ4_NL) {
                const float id = __fdiv_rn(1.0f, __fdiv_rn(bmax, -127.0f));
                float tx[4], t2[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    qi[i] = iq4nl_best_index(__fmul_rn(id, x[i]));
                    const float q = (float) (int) (int8_t) (iq4_lut4((uint32_t) qi[i]) & 0xFFu);
                    const float wq = __fmul_rn(__fmul_rn(x[i], x[i]), q);
                    tx[i] = __fmul_rn(wq, x[i]); t2[i] = __fmul_rn(wq, q);
                }
                float sumqx = 0.0f, sumq2 = 0.0f;                   // element order: lane 0's four, then lane 1's, ...
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if ((lane & 7) == k) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) { sumqx = __fadd_rn(sumqx, tx[i]); sumq2 = __fadd_rn(sumq2, t2[i]); }
                    }
                    sumqx = __shfl(sumqx, (lane & ~7) + k, 64); sumq2 = __shfl(sumq2, (lane & ~7) + k, 64);
                }
                o.d = __fdiv_rn(sumqx, sumq2);
                if (gmax < 1e-15f) {                               // GROUP_MAX_EPS (uniform over the group)
                    o.d = 0.0f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) qi[i] = 0;
                }
            } else {
                constexpr float HALF_RANGE = KVT == MI355Q_TYPE_Q4_0 ? 8.0f : 16.0f;
                constexpr int QMAX = KVT == MI355Q_TYPE_Q4_0 ? 15 : 31;
                o.d = __fdiv_rn(bmax, -HALF_RANGE);
                const float id = o.d != 0.0f ? __fdiv_rn(1.0f, o.d) : 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) qi[i] = min(QMAX, (int) (int8_t) __fadd_rn(__fmul_rn(x[i], id), HALF_RANGE + 0.5f));
            }
        }
        uint32_t nib = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) nib |= (uint32_t) (qi[i] & 0xFF) << (8 * i);
        if constexpr (kv_has_qh<KVT>()) {                           // bit of element e at bit e: this lane's four at 4 (lane & 7); disjoint, so the sum is the OR
            const uint32_t b4 = ((nib >> 4) & 1u) | ((nib >> 11) & 2u) | ((nib >> 18) & 4u) | ((nib >> 25) & 8u);
            o.qh = (uint32_t) oct_sum((int) (b4 << (4 * (lane & 7))));
        }
        const uint32_t hi = (uint32_t) dpp_i<0x104>((int) nib);  // row_shl:4 -- lanes 0..3 of the group get elements 16..31 from lanes 4..7
        o.w = (nib & 0x0F0F0F0Fu) | ((hi & 0x0F0F0F0Fu) << 4);
    }
}
// store lane l's share of the block at `blk` (the header by lane 0; the nibble types: lanes 0..3 only)
template <int KVT>
__device__ __forceinline__ void kv_store_group8(char * blk, int lane8, const KvBlk & o) {
    if (KVT != MI355Q_TYPE_Q8_0 && lane8 >= 4) return;
    if (lane8 == 0) {
        *(__half *) blk = __float2half_rn(o.d);
        if constexpr (kv_has_min<KVT>()) *(__half *) (blk + 2) = __float2half_rn(o.m);
        if constexpr (kv_has_qh<KVT>()) { *(uint16_t *) (blk + kv_qs_off<KVT>() - 4) = (uint16_t) (o.qh & 0xFFFFu); *(uint16_t *) (blk + kv_qs_off<KVT>() - 2) = (uint16_t) (o.qh >> 16); }
    }
    *(uint16_t *) (blk + kv_qs_off<KVT>() + 4 * lane8) = (uint16_t) (o.w & 0xFFFFu);
    *(uint16_t *) (blk + kv_qs_off<KVT>() + 2 + 4 * lane8) = (uint16_t) (o.w >> 16);
}

// ---- q -> Q8_0 / Q8_1 for the scores: thread i quantizes elements 4i .. 4i+3 of q (zeros beyond DK); whole waves take part.  qq[i] = the packed quants,
// qd[b] = the f16-rounded scale of block b (what the CPU's block_q8_0 holds); SUM (Q8_1, ggml-cpu-quants.c:1053 ff.): qsum[b] = s = f16(d * sum of the
// quants), d not rounded.  The SIMD quantizers round half to even (ggml-cpu-quants.c:842-845, :1172-1175).
template <bool SUM = false>
__device__ __forceinline__ void fa_quantize_q(const float * qp, int i, int64_t DK, uint32_t * qq, float * qd, float * qsum = nullptr) {
    const int e = 4 * i;
    const float4 x = e < DK ? make_float4(qp[e], qp[e + 1], qp[e + 2], qp[e + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t pq; float dq; int sum;
    q80_group8<true>(x, pq, dq, sum);
    if (e < DK) {
        qq[i] = pq;
        if ((i & 7) == 0) {
            qd[i >> 3] = __half2float(__float2half_rn(dq));
            if constexpr (SUM) qsum[i >> 3] = __half2float(__float2half_rn(__fmul_rn(dq, (float) sum)));
        }
    }
}

// ---- one score: the cache row `row` (nblk blocks) against the quantized q, before the scale.  ggml_vec_dot_q8_0_q8_0 (AVX2): per block d = d_k * d_q,
// eight f32 lane sums of four int8 products each fed by fma, then hsum_float_8.  ggml_vec_dot_q4_0_q8_0: bytes_from_nibbles_32 puts the low nibbles at
// elements 0..15 and the high ones at 16..31, minus 8 each; the same lane structure.  _q5_0_q8_0 (:3076-3098): nibble | fifth bit << 4, minus 16.
// _q4_1_q8_1 (:2749-2782) / _q5_1_q8_1 (:3409-3434): unsigned quants, and summs += m_k * s_q in block order (a rounded product, a rounded sum), result
// hsum + summs.  _iq4_nl_q8_0 (:12498-12525): code-book values; blocks in pairs into two accumulators, added, then hsum; an odd last block through the
// scalar tail (:12653-12661): sumf += d * (sum of the 32 products), not contracted.  The integer parts are exact (v_dot4).
template <int KVT>
__device__ __forceinline__ float fa_dot_q80(const char * row, const float * qd, const uint32_t * qq, int nblk, const float * qsum = nullptr) {
    constexpr int BB = kv_block_bytes<KVT>(), QO = kv_qs_off<KVT>();
    float acc[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    if constexpr (KVT == MI355Q_TYPE_IQ4_NL) {
        float acc2[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
        const int npair = nblk & ~1;
        for (int blk = 0; blk < npair; ++blk) {
            const char * kb = row + BB * blk;
            const float dd = __fmul_rn(qd[blk], __half2float(*(const __half *) kb));
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const uint32_t kw = ld_w16(kb + QO + 4 * l);
                const float plo = (float) dot4((int) iq4_lut4(kw & 0x0F0F0F0Fu), (int) qq[8 * blk + l], 0);
                const float phi = (float) dot4((int) iq4_lut4((kw >> 4) & 0x0F0F0F0Fu), (int) qq[8 * blk + 4 + l], 0);
                if (blk & 1) { acc2[l] = __builtin_fmaf(dd, plo, acc2[l]); acc2[l + 4] = __builtin_fmaf(dd, phi, acc2[l + 4]); }     // (uniform)
                else         { acc[l]  = __builtin_fmaf(dd, plo, acc[l]);  acc[l + 4]  = __builtin_fmaf(dd, phi, acc[l + 4]); }
            }
        }
#pragma unroll
        for (int l = 0; l < 8; ++l) acc[l] = __fadd_rn(acc[l], acc2[l]);
    } else {
        for (int blk = 0; blk < nblk; ++blk) {
            const char * kb = row + BB * blk;
            const float dd = __fmul_rn(__half2float(*(const __half *) kb), qd[blk]);
            if constexpr (KVT == MI355Q_TYPE_Q8_0) {
#pragma unroll
                for (int l = 0; l < 8; ++l) {
                    const uint32_t kw = (uint32_t) *(const uint16_t *) (kb + 2 + 4 * l) | ((uint32_t) *(const uint16_t *) (kb + 4 + 4 * l) << 16);
                    acc[l] = __builtin_fmaf(dd, (float) dot4((int) kw, (int) qq[8 * blk + l], 0), acc[l]);
                }
            } else if constexpr (KVT == MI355Q_TYPE_Q4_0) {
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const uint32_t kw = (uint32_t) *(const uint16_t *) (kb + 2 + 4 * l) | ((uint32_t) *(const uint16_t *) (kb + 4 + 4 * l) << 16);
                    const int qlo = (int) qq[8 * blk + l], qhi = (int) qq[8 * blk + 4 + l];
                    acc[l]     = __builtin_fmaf(dd, (float) (dot4((int) (kw & 0x0F0F0F0Fu), qlo, 0) - 8 * dot4(0x01010101, qlo, 0)), acc[l]);
                    acc[l + 4] = __builtin_fmaf(dd, (float) (dot4((int) ((kw >> 4) & 0x0F0F0F0Fu), qhi, 0) - 8 * dot4(0x01010101, qhi, 0)), acc[l + 4]);
                }
            } else {                                                           // Q4_1, Q5_0, Q5_1
                uint32_t qh = 0;
                if constexpr (kv_has_qh<KVT>()) qh = ld_w16(kb + QO - 4);
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const uint32_t kw = ld_w16(kb + QO + 4 * l);
                    const int qlo = (int) qq[8 * blk + l], qhi = (int) qq[8 * blk + 4 + l];
                    uint32_t xlo = kw & 0x0F0F0F0Fu, xhi = (kw >> 4) & 0x0F0F0F0Fu;
                    if constexpr (kv_has_qh<KVT>()) { xlo |= kv_spread4(qh >> (4 * l)); xhi |= kv_spread4(qh >> (16 + 4 * l)); }
                    int plo = dot4((int) xlo, qlo, 0), phi = dot4((int) xhi, qhi, 0);
                    if constexpr (KVT == MI355Q_TYPE_Q5_0) { plo -= 16 * dot4(0x01010101, qlo, 0); phi -= 16 * dot4(0x01010101, qhi, 0); }
                    acc[l]     = __builtin_fmaf(dd, (float) plo, acc[l]);
                    acc[l + 4] = __builtin_fmaf(dd, (float) phi, acc[l + 4]);
                }
            }
        }
    }
    const float t0 = __fadd_rn(acc[0], acc[4]), t1 = __fadd_rn(acc[1], acc[5]), t2 = __fadd_rn(acc[2], acc[6]), t3 = __fadd_rn(acc[3], acc[7]);
    float sum = __fadd_rn(__fadd_rn(t0, t2), __fadd_rn(t1, t3));      // hsum_float_8
    if constexpr (kv_has_min<KVT>()) {
        float summs = 0.0f;
        for (int blk = 0; blk < nblk; ++blk) summs = __fadd_rn(summs, __fmul_rn(__half2float(*(const __half *) (row + BB * blk + 2)), qsum[blk]));
        sum = __fadd_rn(sum, summs);
    }
    if constexpr (KVT == MI355Q_TYPE_IQ4_NL) {
        if (nblk & 1) {                                                        // (uniform)
            const int blk = nblk - 1;
            const char * kb = row + BB * blk;
            const float dd = __fmul_rn(qd[blk], __half2float(*(const __half *) kb));
            int t = 0;
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const uint32_t kw = ld_w16(kb + QO + 4 * l);
                t = dot4((int) iq4_lut4(kw & 0x0F0F0F0Fu), (int) qq[8 * blk + l], t);
                t = dot4((int) iq4_lut4((kw >> 4) & 0x0F0F0F0Fu), (int) qq[8 * blk + 4 + l], t);
            }
            sum = __fadd_rn(sum, __fmul_rn(dd, (float) t));
        }
    }
    return sum;
}

// ---- one element of a cache block as dequantize_row_<type> gives it (ggml-quants.c:255-345, :2436-2452): q * d, (nibble - 8) * d, nibble * d + m
// (a rounded product, a rounded sum), ((nibble | bit << 4) - 16) * d, (nibble | bit << 4) * d + m, d * kvalues_iq4nl[nibble].  e = 0..31.
template <int KVT>
__device__ __forceinline__ float kv_dequant_elem(const char * blk, int e) {
    const float d = __half2float(*(const __half *) blk);
    if constexpr (KVT == MI355Q_TYPE_Q8_0) return __fmul_rn((float) (int) *(const int8_t *) (blk + 2 + e), d);
    else {
        const int byte = (int) *(const uint8_t *) (blk + kv_qs_off<KVT>() + (e & 15));
        int qv = (e < 16 ? byte : byte >> 4) & 15;
        if constexpr (kv_has_qh<KVT>()) qv |= (((int) *(const uint16_t *) (blk + kv_qs_off<KVT>() - 4 + 2 * (e >> 4)) >> (e & 15)) & 1) << 4;
        if constexpr (KVT == MI355Q_TYPE_Q4_0) qv -= 8;
        if constexpr (KVT == MI355Q_TYPE_Q5_0) qv -= 16;
        if constexpr (KVT == MI355Q_TYPE_IQ4_NL) qv = (int) (int8_t) (iq4_lut4((uint32_t) qv) & 0xFFu);
        const float p = __fmul_rn((float) qv, d);
        if constexpr (kv_has_min<KVT>()) return __fadd_rn(p, __half2float(*(const __half *) (blk + 2)));
        else return p;
    }
}

// ---- the online softmax in position order, by ONE wave (all 64 lanes): scores s[0, n) (-inf = skipped) -> s[j] = the weight vs of position j,
// msv[j] = the accumulator's rescale factor ms (a new maximum: ms = expf(Mprev - s), vs = 1; otherwise ms = 1, vs = expf(s - Mprev); skipped:
// ms = 1, vs = 0).  Returns the final maximum (uniform; -inf when every position is skipped).  tab: PLAN_EXP2F_T[lane & 31].
__device__ __forceinline__ float fa_seq_weights(float * s, float * msv, int64_t n, int lane, unsigned long long tab, float carry0 = -INFINITY) {
    float carry = carry0;                                                       // (the maximum a walk over earlier positions ended with: the decode plan's chained splits)
    for (int64_t j0 = 0; j0 < n; j0 += 64) {
        const int64_t j = j0 + lane;
        const float sj = j < n ? s[j] : -INFINITY;
        float x = sj;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const float o = __shfl_up(x, off, 64); if (lane >= off) x = fmaxf(x, o); }     // inclusive prefix maximum
        float prev = __shfl_up(x, 1, 64);
        prev = fmaxf(lane == 0 ? -INFINITY : prev, carry);
        carry = fmaxf(carry, __shfl(x, 63, 64));
        const bool live = sj != -INFINITY, newmax = live && sj > prev;
        const float e = expf_libm(newmax ? __fsub_rn(prev, sj) : live ? __fsub_rn(sj, prev) : 0.0f, tab);
        if (j < n) { s[j] = newmax ? 1.0f : live ? e : 0.0f; msv[j] = newmax ? e : 1.0f; }
    }
    return carry;
}

// ---- V . P for output element e: vb = the cache block of e at position 0, nb_pos = bytes between positions.  acc = the unnormalized F32 accumulator,
// S = the CPU's running sum (S * ms + vs); skipped positions are never read.
template <int KVT>
__device__ __forceinline__ void fa_pv_q80(const char * vb, int64_t nb_pos, int e, const float * ws, const float * msv, int64_t n, float & acc_out, float & S_out) {
    float acc = 0.0f, S = 0.0f;
#pragma unroll 4
    for (int64_t j = 0; j < n; ++j) {
        const float vs = ws[j], ms = msv[j];
        if (vs != 0.0f || ms != 1.0f) {                                       // (uniform)
            const char * blk = vb + j * nb_pos;
            const float vv = kv_dequant_elem<KVT>(blk, e);                    // dequantize_row_<type>
            if (ms != 1.0f) acc = __fmul_rn(acc, ms);                         // ggml_vec_scale_f32
            acc = __builtin_fmaf(vv, vs, acc);                                // ggml_vec_mad_f32
            S = __fadd_rn(__fmul_rn(S, ms), vs);
        }
    }
    acc_out = acc; S_out = S;
}

#endif // __HIPCC__

} // namespace mi355q
