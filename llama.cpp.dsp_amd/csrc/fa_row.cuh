// fa_row.cuh -- what the one-workgroup-per-row FLASH_ATTN_EXT kernels share across translation units (ops_glue.hip: k_flash_attn_ext, k_flash_attn_ext_q80;
// fattn_mix.hip: k_flash_attn_ext_mix): the device copy of a tensor descriptor, the launch shape, and the f16 side of the CPU's arithmetic -- the score in
// ggml_vec_dot_f16's AVX2 order and the F16-accumulator walk over V (ggml-cpu/ops.cpp:6810-6890).  The block types' side lives in fa_quant.cuh.
#pragma once
#include "mi355q_common.h"
#include "fa_quant.cuh"

namespace mi355q {

struct TensorD { char * data; int type; int64_t ne[4]; int64_t nb[4]; };     // device copy of mi355q_tensor (type: 0 f32, 1 f16, 30 bf16)

static inline TensorD to_d(const mi355q_tensor * t) {
    TensorD d; d.data = (char *) t->data; d.type = t->type;
    for (int i = 0; i < 4; ++i) { d.ne[i] = t->ne[i]; d.nb[i] = t->nb[i]; }
    return d;
}

constexpr int FA_THREADS = 1024, FA_WAVES = FA_THREADS / 64;      // 16 waves: a decode step has only n_head workgroups, each must hide its own latency

#ifdef __HIPCC__

// ---- one f16 score by ONE wave, before the scale: kr[u] / qh[u] = element lane + 64 u of the K row / of q rounded to f16 (zero past DK), nblk = DK / 32.
// ggml_vec_dot_f16's order (vec.cpp:128-168, AVX2 form; see plan.hip plan_attn_lds step 2): element e = lane + 64 u feeds accumulator
// (jj, l) = ((e % 32) / 8, e % 8) of block e / 32 -- lanes L and L ^ 32 own the even and the odd blocks of one accumulator, whose chain
// therefore passes between the two halves of the wave; then the tree (a0 + a2) + (a1 + a3), s[l] + s[l + 4], (t0 + t1) + (t2 + t3).  The result is lane 0's.
__device__ __forceinline__ float fa_dot_f16_seq(const float (&kr)[4], const float (&qh)[4], int nblk, int lane) {
    const int half = lane >> 5;
    float acc = 0.0f;
#pragma unroll
    for (int blk = 0; blk < 8; ++blk) {                       // (head sizes up to 256: 8 blocks; constant register indices)
        if (blk < nblk) {
            if (half == (blk & 1)) acc = __builtin_fmaf(kr[blk >> 1], qh[blk >> 1], acc);
            const float other = __shfl_xor(acc, 32, 64);
            if (half != (blk & 1)) acc = other;
        }
    }
    acc = __fadd_rn(acc, __shfl_xor(acc, 16, 64));            // (a0 + a2) in the j = 0 lanes, (a1 + a3) in the j = 1 lanes
    acc = __fadd_rn(acc, __shfl_xor(acc, 8, 64));             // s[l]
    acc = __fadd_rn(acc, __shfl_xor(acc, 4, 64));             // t[i] = s[i] + s[i + 4]
    acc = __fadd_rn(acc, __shfl_xor(acc, 1, 64));             // t0 + t1 | t2 + t3
    acc = __fadd_rn(acc, __shfl_xor(acc, 2, 64));
    return acc;
}

// ---- V . P for one output element of an f16 V with the CPU's F16 accumulator (VKQ16): vb = the element at position 0, nb_pos = bytes between positions,
// ws / msv = fa_seq_weights' weights and rescale factors.  acc is an f16 value at all times; skipped positions are never read.  acc0 / S0: where a walk
// over earlier positions ended (the decode plan's chained splits, plan.hip plan_attn_mix step 3b); 0 for a walk from the start.
__device__ __forceinline__ void fa_pv_f16_seq(const char * vb, int64_t nb_pos, const float * ws, const float * msv, int64_t n, float & acc_out, float & S_out,
                                              float acc0 = 0.0f, float S0 = 0.0f) {
    float acc = acc0, S = S0;
#pragma unroll 4
    for (int64_t j = 0; j < n; ++j) {
        const float vs = ws[j], ms = msv[j];
        if (vs != 0.0f || ms != 1.0f) {                             // (uniform) masked positions are skipped altogether
            const float vv = __half2float(*(const __half *) (vb + j * nb_pos));
            if (ms != 1.0f) acc = f16_round(__fmul_rn(acc, ms));         // ggml_vec_scale_f16
            acc = f16_round(__builtin_fmaf(vv, vs, acc));                // ggml_vec_mad_f16
            S = __fadd_rn(__fmul_rn(S, ms), vs);
        }
    }
    acc_out = acc; S_out = S;
}

#endif // __HIPCC__

} // namespace mi355q
