// fa_quant.cuh -- the per-position arithmetic of FLASH_ATTN_EXT over a Q8_0 / Q4_0 KV cache, shared by the residency op (ops_glue.hip
// k_flash_attn_ext_q80, k_cpy_f32_q8_0 / k_cpy_f32_q4_0) and the decode plan's attention stage (plan.hip plan_attn_q80), so that the two give the
// same bits by construction.  The CPU's order (ggml-cpu/ops.cpp:6686-6905):
//   cache stores   f32 -> block_q8_0 (quantize_row_q8_0_ref) / block_q4_0 (quantize_row_q4_0_ref), what CPY f32 -> q8_0 / q4_0 writes
//   q              quantized to Q8_0 by the SIMD quantizer (round half to even): the vec_dot_type of a Q8_0 / Q4_0 K
//   scores         ggml_vec_dot_q8_0_q8_0 / ggml_vec_dot_q4_0_q8_0 in their AVX2 order
//   softmax        walked in position order with a running maximum (expf_libm: the host library's expf)
//   V . P          V dequantized (q * d) into an F32 accumulator: ggml_vec_scale_f32 when the maximum grows, ggml_vec_mad_f32 per position
// Cache blocks are 2-byte aligned (34 / 18 bytes): they are read and written as halves of words.
#pragma once
#include "mi355q_common.h"
#include "act_quant.cuh"

namespace mi355q {

#ifdef __HIPCC__

template <int KVT> __host__ __device__ constexpr int kv_block_bytes() { return KVT == MI355Q_TYPE_Q8_0 ? 34 : 18; }

// ---- f32 -> one cache block: eight lanes own a block, lane l (= lane & 7) the elements 4l .. 4l+3 (every lane of the wave must take part: the
// group reductions).  w: Q8_0 -- the four int8 quants of the lane; Q4_0 -- lanes 0..3: the four nibble bytes j = 4l .. 4l+3 (q[j] | q[j + 16] << 4).
// Q8_0: quantize_row_q8_0_ref (round half away from zero).  Q4_0: quantize_row_q4_0_ref (ggml-quants.c:31-66) -- max = the FIRST element of largest
// magnitude, signed; d = max / -8; q = min(15, (int8) (x / d + 8.5)).
template <int KVT>
__device__ __forceinline__ void kv_quant_group8(const float4 v, uint32_t & w, float & d) {
    if constexpr (KVT == MI355Q_TYPE_Q8_0) {
        int sum;
        q80_group8<false>(v, w, d, sum);
    } else {
        const int lane = (int) (threadIdx.x & 63);
        const float x[4] = { v.x, v.y, v.z, v.w };
        float amax = 0.0f, mx = 0.0f;                            // this lane's first element of largest magnitude
#pragma unroll
        for (int i = 0; i < 4; ++i) if (amax < fabsf(x[i])) { amax = fabsf(x[i]); mx = x[i]; }
        const float gmax = oct_max(amax);                         // the block's largest magnitude; its first holder is the lowest lane that has it
        const unsigned long long holders = __ballot(amax == gmax);
        const int first = __ffs((int) ((holders >> (lane & ~7)) & 0xFFull)) - 1;
        const float bmax = __shfl(mx, (lane & ~7) + first, 64);
        d = __fdiv_rn(bmax, -8.0f);
        const float id = d != 0.0f ? __fdiv_rn(1.0f, d) : 0.0f;
        uint32_t nib = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int qi = min(15, (int) (int8_t) __fadd_rn(__fmul_rn(x[i], id), 8.5f)); nib |= (uint32_t) (qi & 0xFF) << (8 * i); }
        const uint32_t hi = (uint32_t) dpp_i<0x104>((int) nib);  // row_shl:4 -- lanes 0..3 of the group get elements 16..31 from lanes 4..7
        w = (nib & 0x0F0F0F0Fu) | ((hi & 0x0F0F0F0Fu) << 4);
    }
}
// store lane l's share of the block at `blk` (d by lane 0; Q4_0: lanes 0..3 only)
template <int KVT>
__device__ __forceinline__ void kv_store_group8(char * blk, int lane8, uint32_t w, float d) {
    if (KVT == MI355Q_TYPE_Q4_0 && lane8 >= 4) return;
    if (lane8 == 0) *(__half *) blk = __float2half_rn(d);
    *(uint16_t *) (blk + 2 + 4 * lane8) = (uint16_t) (w & 0xFFFFu);
    *(uint16_t *) (blk + 4 + 4 * lane8) = (uint16_t) (w >> 16);
}

// ---- q -> Q8_0 for the scores: thread i quantizes elements 4i .. 4i+3 of q (zeros beyond DK); whole waves take part.  qq[i] = the packed quants,
// qd[b] = the f16-rounded scale of block b (what the CPU's block_q8_0 holds).  The SIMD quantize_row_q8_0 rounds half to even (ggml-cpu-quants.c:842-845).
__device__ __forceinline__ void fa_quantize_q(const float * qp, int i, int64_t DK, uint32_t * qq, float * qd) {
    const int e = 4 * i;
    const float4 x = e < DK ? make_float4(qp[e], qp[e + 1], qp[e + 2], qp[e + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t pq; float dq; int sum;
    q80_group8<true>(x, pq, dq, sum);
    if (e < DK) { qq[i] = pq; if ((i & 7) == 0) qd[i >> 3] = __half2float(__float2half_rn(dq)); }
}

// ---- one score: the cache row `row` (nblk blocks) against the quantized q, before the scale.  ggml_vec_dot_q8_0_q8_0 (AVX2): per block d = d_k * d_q,
// eight f32 lane sums of four int8 products each fed by fma, then hsum_float_8.  ggml_vec_dot_q4_0_q8_0: bytes_from_nibbles_32 puts the low nibbles at
// elements 0..15 and the high ones at 16..31, minus 8 each; the same lane structure.
template <int KVT>
__device__ __forceinline__ float fa_dot_q80(const char * row, const float * qd, const uint32_t * qq, int nblk) {
    constexpr int BB = kv_block_bytes<KVT>();
    float acc[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    for (int blk = 0; blk < nblk; ++blk) {
        const char * kb = row + BB * blk;
        const float dd = __fmul_rn(__half2float(*(const __half *) kb), qd[blk]);
        if constexpr (KVT == MI355Q_TYPE_Q8_0) {
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                const uint32_t kw = (uint32_t) *(const uint16_t *) (kb + 2 + 4 * l) | ((uint32_t) *(const uint16_t *) (kb + 4 + 4 * l) << 16);
                acc[l] = __builtin_fmaf(dd, (float) dot4((int) kw, (int) qq[8 * blk + l], 0), acc[l]);
            }
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const uint32_t kw = (uint32_t) *(const uint16_t *) (kb + 2 + 4 * l) | ((uint32_t) *(const uint16_t *) (kb + 4 + 4 * l) << 16);
                const int qlo = (int) qq[8 * blk + l], qhi = (int) qq[8 * blk + 4 + l];
                acc[l]     = __builtin_fmaf(dd, (float) (dot4((int) (kw & 0x0F0F0F0Fu), qlo, 0) - 8 * dot4(0x01010101, qlo, 0)), acc[l]);
                acc[l + 4] = __builtin_fmaf(dd, (float) (dot4((int) ((kw >> 4) & 0x0F0F0F0Fu), qhi, 0) - 8 * dot4(0x01010101, qhi, 0)), acc[l + 4]);
            }
        }
    }
    const float t0 = __fadd_rn(acc[0], acc[4]), t1 = __fadd_rn(acc[1], acc[5]), t2 = __fadd_rn(acc[2], acc[6]), t3 = __fadd_rn(acc[3], acc[7]);
    return __fadd_rn(__fadd_rn(t0, t2), __fadd_rn(t1, t3));      // hsum_float_8
}

// ---- the online softmax in position order, by ONE wave (all 64 lanes): scores s[0, n) (-inf = skipped) -> s[j] = the weight vs of position j,
// msv[j] = the accumulator's rescale factor ms (a new maximum: ms = expf(Mprev - s), vs = 1; otherwise ms = 1, vs = expf(s - Mprev); skipped:
// ms = 1, vs = 0).  Returns the final maximum (uniform; -inf when every position is skipped).  tab: PLAN_EXP2F_T[lane & 31].
__device__ __forceinline__ float fa_seq_weights(float * s, float * msv, int64_t n, int lane, unsigned long long tab) {
    float carry = -INFINITY;
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
            int qv;
            if constexpr (KVT == MI355Q_TYPE_Q8_0) qv = (int) *(const int8_t *) (blk + 2 + e);
            else { const int byte = (int) *(const uint8_t *) (blk + 2 + (e & 15)); qv = ((e < 16 ? byte : byte >> 4) & 15) - 8; }
            const float vv = __fmul_rn((float) qv, __half2float(*(const __half *) blk));     // dequantize_row_q8_0 / _q4_0
            if (ms != 1.0f) acc = __fmul_rn(acc, ms);                         // ggml_vec_scale_f32
            acc = __builtin_fmaf(vv, vs, acc);                                // ggml_vec_mad_f32
            S = __fadd_rn(__fmul_rn(S, ms), vs);
        }
    }
    acc_out = acc; S_out = S;
}

#endif // __HIPCC__

} // namespace mi355q
