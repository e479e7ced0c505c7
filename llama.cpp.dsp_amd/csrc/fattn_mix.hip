// fattn_mix.hip -- k_flash_attn_ext_mix<KT, VT>: FLASH_ATTN_EXT over a KV cache whose K and V have DIFFERENT types (-ctk A -ctv B), each of
// f16, q8_0, q4_0, q4_1, q5_0, q5_1, iq4_nl.  One workgroup per (query row, head, batch) with the CPU's arithmetic, which is separable
// (ggml-cpu/ops.cpp:6767-6770, :6793, :6841, :6870): the scores follow the K type alone, the accumulator follows the V type alone.
//   K a block type   q quantized to the type's vec_dot_type (Q8_0; Q8_1 for Q4_1 / Q5_1), a thread per position, the type's vec_dot: fa_quantize_q,
//                    fa_dot_q80<KT> (fa_quant.cuh) -- the K phase of k_flash_attn_ext_q80
//   K f16            q rounded to f16, a wave per position, ggml_vec_dot_f16's AVX2 order: fa_dot_f16_seq (fa_row.cuh) -- the seq form of k_flash_attn_ext
//   then             s * scale (one rounding), the soft-cap with the host C library's tanhf restated (tanhf_libm.h: the device library's differs in the last
//                    bits, which the same-type kernels accept), + slope * mask; a masked position is skipped whatever its cache row holds
//   softmax          fa_seq_weights: the online softmax walked in position order
//   V a block type   dequantize_row_<type> into the F32 accumulator: fa_pv_q80<VT>
//   V f16            the F16 accumulator (ggml_vec_scale_f16 / ggml_vec_mad_f16): fa_pv_f16_seq
// A translation unit of its own for the build's sake: 42 instantiations.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <array>
#include <utility>

#include "fa_row.cuh"
#include "tanhf_libm.h"

namespace mi355q {

template <int KT, int VT>                                                   // 1 (f16) or a block type of fa_quant.cuh; KT != VT
__global__ void __launch_bounds__(FA_THREADS) k_flash_attn_ext_mix(const TensorD q, const TensorD k, const TensorD v, const TensorD m, int has_mask, const TensorD d,
                                                                   float scale, float max_bias, float softcap, float m0, float m1, uint32_t n_head_log2) {
    extern __shared__ __attribute__((aligned(16))) float fx_s[];             // [n_kv] scores -> weights | [n_kv] rescale factors | a block K: q as [DK / 32] block scales, [DK / 4] packed quants, [DK / 32] block sums
    constexpr bool KB = KT != 1, VB = VT != 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int64_t DK = k.ne[0], DV = v.ne[0], n_kv = k.ne[1];
    const int64_t hk = h / (q.ne[2] / k.ne[2]), hv = h / (q.ne[2] / v.ne[2]), bk = b / (q.ne[3] / k.ne[3]), bv = b / (q.ne[3] / v.ne[3]);
    float * msv = fx_s + n_kv;
    const float * qp = (const float *) (q.data + t * q.nb[1] + h * q.nb[2] + b * q.nb[3]);
    const float slope = max_bias > 0.0f ? ((uint32_t) h < n_head_log2 ? powf(m0, (float) (h + 1)) : powf(m1, (float) (2 * (h - n_head_log2) + 1))) : 1.0f;
    const __half * mp = has_mask ? (const __half *) (m.data + t * m.nb[1]) : nullptr;
    const char * kbase = k.data + hk * k.nb[2] + bk * k.nb[3];
    const int nblk = (int) (DK >> 5);
    // ---- scores
    if constexpr (KB) {
        float * qd = msv + n_kv;
        uint32_t * qq = (uint32_t *) (qd + (DK >> 5));
        float * qsum = (float *) (qq + (DK >> 2));
        if (tid < ((DK / 4 + 63) & ~63)) fa_quantize_q<kv_has_min<KT>()>(qp, tid, DK, qq, qd, qsum);     // (whole waves take part: the 8-lane reductions)
        __syncthreads();
        for (int64_t j = tid; j < n_kv; j += FA_THREADS) {                    // one position per thread
            const float mv = mp ? __fmul_rn(slope, __half2float(mp[j])) : 0.0f;
            float s = -INFINITY;
            if (mv != -INFINITY) {                                            // (a masked position is skipped by the CPU whatever its cache row holds)
                s = fa_dot_q80<KT>(kbase + j * k.nb[1], qd, qq, nblk, qsum);
                s = __fmul_rn(s, scale);
                if (softcap != 0.0f) s = __fmul_rn(softcap, tanhf_libm(s));      // the host C library's tanhf (tanhf_libm.h)
                s = __fadd_rn(s, mv);
            }
            fx_s[j] = s;
        }
    } else {
        float qh[4];                                                          // head sizes up to 256: 4 elements per lane
#pragma unroll
        for (int u = 0; u < 4; ++u) qh[u] = lane + 64 * u < DK ? __half2float(__float2half_rn(qp[lane + 64 * u])) : 0.0f;
        constexpr int JB = 8;                                                 // rows per trip: their loads are in flight together
        for (int64_t j0 = wave; j0 < n_kv; j0 += FA_WAVES * JB) {             // one position per wave
            float kr[JB][4];
#pragma unroll
            for (int c = 0; c < JB; ++c) {
                const int64_t j = j0 + FA_WAVES * c < n_kv ? j0 + FA_WAVES * c : j0;
                const __half * kp = (const __half *) (kbase + j * k.nb[1]);
#pragma unroll
                for (int u = 0; u < 4; ++u) kr[c][u] = lane + 64 * u < DK ? __half2float(kp[lane + 64 * u]) : 0.0f;
            }
#pragma unroll
            for (int c = 0; c < JB; ++c) {
                const int64_t j = j0 + FA_WAVES * c;
                float s = fa_dot_f16_seq(kr[c], qh, nblk, lane);
                if (lane == 0 && j < n_kv) {
                    s = __fmul_rn(s, scale);
                    if (softcap != 0.0f) s = __fmul_rn(softcap, tanhf_libm(s));      // the host C library's tanhf (tanhf_libm.h)
                    if (mp) {
                        const float mv = __fmul_rn(slope, __half2float(mp[j]));
                        s = mv == -INFINITY ? -INFINITY : __fadd_rn(s, mv);     // (a masked position: its row's bits, NaN included, go nowhere)
                    }
                    fx_s[j] = s;
                }
            }
        }
    }
    __syncthreads();
    // ---- online softmax in order: rescale factor and weight per position
    if (wave == 0) fa_seq_weights(fx_s, msv, n_kv, lane, PLAN_EXP2F_T[lane & 31]);
    __syncthreads();
    // ---- V . P, a thread per output dim: the F32 accumulator over a block V, the F16 accumulator over an f16 V
    if (tid < DV) {
        const char * vbase = v.data + hv * v.nb[2] + bv * v.nb[3];
        float acc, S;
        if constexpr (VB) fa_pv_q80<VT>(vbase + kv_block_bytes<VT>() * (tid >> 5), v.nb[1], tid & 31, fx_s, msv, n_kv, acc, S);
        else fa_pv_f16_seq(vbase + 2 * (int64_t) tid, v.nb[1], fx_s, msv, n_kv, acc, S);
        *(float *) (d.data + tid * d.nb[0] + h * d.nb[1] + t * d.nb[2] + b * d.nb[3]) = __fmul_rn(acc, __fdiv_rn(1.0f, S));
    }
}

// ---- the 7 x 7 table of instantiations (the diagonal is empty: same-type caches have kernels of their own)
constexpr int FA_MIX_TYPES[7] = { 1, MI355Q_TYPE_Q8_0, MI355Q_TYPE_Q4_0, MI355Q_TYPE_Q4_1, MI355Q_TYPE_Q5_0, MI355Q_TYPE_Q5_1, MI355Q_TYPE_IQ4_NL };
static int fa_mix_index(int type) {
    for (int i = 0; i < 7; ++i) if (FA_MIX_TYPES[i] == type) return i;
    return -1;
}
template <size_t I>
static const void * fa_mix_entry() {
    constexpr int kt = FA_MIX_TYPES[I / 7], vt = FA_MIX_TYPES[I % 7];
    if constexpr (kt == vt) return nullptr;
    else return (const void *) k_flash_attn_ext_mix<kt, vt>;
}
template <size_t... I>
static std::array<const void *, 49> fa_mix_table(std::index_sequence<I...>) { return { fa_mix_entry<I>()... }; }

// The launcher ops_glue.hip calls once mi355q_op_flash_attn_ext_path2 has answered MI355Q_FA_PATH_KV_ROW for a mixed pair: types, shapes, alignment and
// n_kv <= 8192 are checked there.  scale is the one applied to the raw dot product (already divided by the soft-cap).
__attribute__((visibility("hidden")))
int fattn_mix_launch(const mi355q_tensor * q, const mi355q_tensor * k, const mi355q_tensor * v, const mi355q_tensor * mask, const mi355q_tensor * dst,
                     float scale, float max_bias, float softcap, float m0, float m1, uint32_t n_head_log2, void * stream) {
    static const std::array<const void *, 49> table = fa_mix_table(std::make_index_sequence<49>());
    const int ki = fa_mix_index(k->type), vi = fa_mix_index(v->type);
    if (ki < 0 || vi < 0 || ki == vi) return MI355Q_ERR_UNSUPPORTED;
    const int64_t DK = k->ne[0], n_kv = k->ne[1];
    const size_t lds = (size_t) (2 * n_kv + (k->type != 1 ? 2 * (DK / 32) + DK / 4 : 0)) * 4;
    if (lds > 150 * 1024) return MI355Q_ERR_UNSUPPORTED;
    static bool attr_set[64] = {};
    if (lds > 48 * 1024) {
        int dev = 0; (void) hipGetDevice(&dev); dev = dev >= 0 && dev < 64 ? dev : 0;
        if (!attr_set[dev]) {
            for (const void * fn : table)
                if (fn && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) != hipSuccess) return MI355Q_ERR_HIP;
            attr_set[dev] = true;
        }
    }
    TensorD qd = to_d(q), kd = to_d(k), vd = to_d(v), md = mask ? to_d(mask) : to_d(q), dd = to_d(dst);
    int has_mask = mask ? 1 : 0;
    void * args[] = { &qd, &kd, &vd, &md, &has_mask, &dd, &scale, &max_bias, &softcap, &m0, &m1, &n_head_log2 };
    const hipError_t e = hipLaunchKernel(table[7 * ki + vi], dim3((unsigned) q->ne[1], (unsigned) q->ne[2], (unsigned) q->ne[3]), dim3(FA_THREADS), args, lds, (hipStream_t) stream);
    return e == hipSuccess && hipGetLastError() == hipSuccess ? MI355Q_OK : MI355Q_ERR_HIP;
}

} // namespace mi355q
