// fattn_mfma.cuh -- k_flash_attn_mfma: FLASH_ATTN_EXT for many query rows in ONE launch on the matrix cores, gfx950 only.
//
//   dst[:, h, t, b] = softmax_j(softcap(scale * k_j . f16(q_t)) + slope_h * mask[t][j]) . v_j        f16 K / V, f32 q, f16 mask or none, f32 dst
//
// One 256-thread workgroup per (64 query rows, head, batch); wave w owns rows 16 w .. 16 w + 15 and keeps their q fragments in registers.  The
// window is walked in tiles of 64 positions: the K and the V tile are copied into LDS as they lie in memory (rows padded against bank conflicts),
//   S^T[j][t] = sum_e K[j][e] q[t][e]        v_mfma_f32_16x16x32_f16, A = K rows from LDS, B = q fragment      (C: lane holds t = lane & 15,
//                                                                                                               j = 16 blk + 4 (lane >> 4) + r)
//   online softmax in f32 per row t (the four lanes lane & 15 == t hold its 64 scores): running maximum, running sum, O rescaled per tile,
//   O^T[e][t] += sum_j V[j][e] P[t][j]       A = V read TRANSPOSED from LDS (ds_read_b64_tr_b16), B = P rounded to f16.
// The sum index of an MFMA may be walked in any order as long as both operands agree: k element i of lane group g is position
// 16 (2 s + (i >> 2)) + 4 g + (i & 3) of the tile, which is where the C layout of S^T left the scores -- P never leaves its registers, and the
// transposed read delivers exactly V[those four positions][e] per lane.  No score scratch, no workspace, no global atomics.
//
// A tile whose mask is -inf for all of the workgroup's query rows is neither loaded nor computed (the causal half of a prompt): a first pass over
// the mask rows leaves one bit per tile in LDS.  Tiles past that bitmap's capacity (FA_MAP_WORDS * 32 tiles) are simply taken as live.
// Inside a live tile a masked position has probability exactly 0 and its score is replaced, not added to: the contract is the one of the other
// matrix-core paths, finite cache rows.  Rows of the tile past n_kv and head elements past DK are zero in LDS, never garbage.
//
// KVT, the cache type -- VVT is V's where it differs from K's, a mixed cache: fattn_mfma_mx[a-d].hip -- (fattn_mfma.hip: f16; fattn_mfma_kva.hip / _kvb.hip: the others, translation units of their own for the build's sake):
//   1 (f16)          the text above.
//   a block type     Q8_0, Q4_0, Q4_1, Q5_0, Q5_1, IQ4_NL: only the staging differs.  Thread (row, seg) owns elements 8 seg .. 8 seg + 7 of block i
//                    of its row: it fetches their raw bytes (8 quant bytes, d, m / one byte of qh where the type has them) packed in four registers
//                    while the loads fly under the current tile's MFMAs and decodes them to f16 on the way into the SAME LDS tile:
//                    element e = __float2half_rn(kv_dequant_elem<KVT>(blk, e)), what k_dequant_cache_f16 writes -- so the output equals the f16
//                    kernel's on the f16 copy of the cache bit for bit.  Blocks are only 2-byte aligned: dword loads where data and nb[1..3] are
//                    multiples of 4 (the alignment of a block part then follows from the block's index), 16-bit loads otherwise; nothing outside
//                    the blocks of rows < n_kv is read.
//   MI355Q_T_BF16    q rounded to bf16 once (RNE, the CPU's rule), K / V tiles copied as they lie (the transposed LDS read does not care about the
//                    type), both products on v_mfma_f32_16x16x32_bf16, P rounded to bf16: no value passes through f16.
#pragma once
#include "mi355q_common.h"
#include "fa_quant.cuh"

#include <math.h>

namespace mi355q {

typedef _Float16 fam_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 fam_h4 __attribute__((ext_vector_type(4)));
typedef float    fam_f4 __attribute__((ext_vector_type(4)));

constexpr int FAM_T = 64;                       // query rows per workgroup and positions per tile
constexpr int FAM_MAP_WORDS = 1024;             // live-tile bitmap: 32768 tiles = 2 Mi positions (beyond: live)

struct FamArgs {
    const char * q, * k, * v, * m; char * d;
    int64_t q_nb[4], k_nb[4], v_nb[4], d_nb[4], m_nb1;
    int64_t N, n_kv;
    int DK, DV, gqa_k, gqa_v, bq_k, bq_v;       // heads of q per head of k / v, batches of q per batch of k / v
    int map_words;
    float scale, softcap, max_bias, m0, m1; uint32_t n_head_log2;
    int k_al4, v_al4;                           // a block cache: data and nb[1..3] are multiples of 4 (dword loads)
};

__host__ __device__ constexpr bool fam_is_blocks(int t) {
    return t == MI355Q_TYPE_Q8_0 || t == MI355Q_TYPE_Q4_0 || t == MI355Q_TYPE_Q4_1 || t == MI355Q_TYPE_Q5_0 || t == MI355Q_TYPE_Q5_1 || t == MI355Q_TYPE_IQ4_NL;
}

__device__ __forceinline__ fam_h4 fam_read_tr(const uint8_t * p) {
    typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    typedef __attribute__((address_space(3))) fp16x4 lds_h4;
    const fp16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4 *) (uintptr_t) p);      // (the LDS offset is the low half of the flat address)
    return __builtin_bit_cast(fam_h4, x);
}

// f32 -> bf16 bits by the CPU's rule (ggml_compute_fp32_to_bf16; ops_glue.hip f32_to_bf16): round to nearest even on the bits, a NaN made quiet
__device__ __forceinline__ _Float16 fam_bf16_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    const uint16_t r = (u & 0x7FFFFFFFu) > 0x7F800000u ? (uint16_t) ((u >> 16) | 0x40u) : (uint16_t) ((u + (0x7FFFu + ((u >> 16) & 1u))) >> 16);
    return __builtin_bit_cast(_Float16, r);
}
template <bool BF>
__device__ __forceinline__ fam_f4 fam_mfma(const fam_h8 x, const fam_h8 y, const fam_f4 c) {       // (BF: the registers hold bf16 bits)
    if constexpr (BF) {
        typedef __bf16 fam_b8 __attribute__((ext_vector_type(8)));
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(fam_b8, x), __builtin_bit_cast(fam_b8, y), c, 0, 0, 0);
    } else return __builtin_amdgcn_mfma_f32_16x16x32_f16(x, y, c, 0, 0, 0);
}

// ---- a block cache: the raw bytes of elements 8 s .. 8 s + 7 of the block at `blk`: r.x, r.y = the 8 quant bytes (the nibble types: the bytes that hold
// them, qs[8 (s & 1) ..]), r.z = d | m << 16, r.w = byte s of qh.  mod4 = the block's address modulo 4, known when al4 (0 or 2: blocks are even-sized).
template <int KVT>
__device__ __forceinline__ void fam_fetch_blk(const char * blk, int s, bool al4, int mod4, uint4 & r) {
    constexpr int QO = kv_qs_off<KVT>();
    const char * p = blk + QO + 8 * (KVT == MI355Q_TYPE_Q8_0 ? s : (s & 1));
    if (al4) {
        if (((mod4 + QO) & 3) == 0) { r.x = *(const uint32_t *) p; r.y = *(const uint32_t *) (p + 4); }
        else {                                                                // 2 mod 4: a half, a word, a half -- exactly the 8 bytes
            const uint32_t x = *(const uint16_t *) p, y = *(const uint32_t *) (p + 2), z = *(const uint16_t *) (p + 6);
            r.x = x | (y << 16); r.y = (y >> 16) | (z << 16);
        }
    } else { r.x = ld_w16(p); r.y = ld_w16(p + 4); }
    r.z = *(const uint16_t *) blk;
    if constexpr (kv_has_min<KVT>()) r.z |= (uint32_t) *(const uint16_t *) (blk + 2) << 16;
    r.w = 0;
    if constexpr (kv_has_qh<KVT>()) r.w = ((uint32_t) *(const uint16_t *) (blk + QO - 4 + 2 * (s >> 1)) >> (8 * (s & 1))) & 0xFFu;
}
// ... decoded: eight f16, element e = __float2half_rn(kv_dequant_elem<KVT>(blk, 8 s + e)) with the same f32 operations (fa_quant.cuh)
template <int KVT>
__device__ __forceinline__ uint4 fam_decode_blk(const uint4 r, int s) {
    const float d = h2f(r.z & 0xFFFFu);
    uint32_t w[2] = { r.x, r.y };
    if constexpr (KVT != MI355Q_TYPE_Q8_0) {
        if (s >= 2) { w[0] >>= 4; w[1] >>= 4; }                               // elements 16 .. 31: the high nibbles
        w[0] &= 0x0F0F0F0Fu; w[1] &= 0x0F0F0F0Fu;
        if constexpr (kv_has_qh<KVT>()) { w[0] |= kv_spread4(r.w); w[1] |= kv_spread4(r.w >> 4); }
        if constexpr (KVT == MI355Q_TYPE_IQ4_NL) { w[0] = iq4_lut4(w[0]); w[1] = iq4_lut4(w[1]); }
    }
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t byte = (w[e >> 2] >> (8 * (e & 3))) & 0xFFu;
        int qv = (int) byte;
        if constexpr (KVT == MI355Q_TYPE_Q8_0 || KVT == MI355Q_TYPE_IQ4_NL) qv = (int) (int8_t) byte;
        if constexpr (KVT == MI355Q_TYPE_Q4_0) qv -= 8;
        if constexpr (KVT == MI355Q_TYPE_Q5_0) qv -= 16;
        float x = __fmul_rn((float) qv, d);
        if constexpr (kv_has_min<KVT>()) x = __fadd_rn(x, h2f(r.z >> 16));
        const uint32_t hb = __half_as_ushort(__float2half_rn(x));
        o[e >> 1] = (e & 1) ? (o[e >> 1] | (hb << 16)) : hb;
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// DKB / DVB: the head sizes rounded up to 64, 128 or 256 -- they size the register arrays; the true sizes are run-time values
// KVT / VVT: the K and the V cache type (VVT != KVT: a mixed cache, DESIGN.md 5.7g -- the K staging follows KVT, the V staging VVT, nothing else differs)
template <int DKB, int DVB, int KVT = 1, int VVT = KVT>
__global__ void __launch_bounds__(256) k_flash_attn_mfma(const FamArgs a) {
    constexpr bool QK = fam_is_blocks(KVT), QV = fam_is_blocks(VVT), BF = KVT == MI355Q_T_BF16;
    static_assert(KVT == VVT || (KVT != MI355Q_T_BF16 && VVT != MI355Q_T_BF16), "a mixed cache has no bf16 side");
    extern __shared__ __attribute__((aligned(16))) uint8_t fam_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
    const int64_t N = a.N, n_kv = a.n_kv, n0 = (int64_t) blockIdx.x * FAM_T;
    const int h = blockIdx.y, b = blockIdx.z, DK = a.DK, DV = a.DV;
    const int dk32 = (DK + 31) & ~31;                                        // the K tile's row in LDS: whole 32-element MFMA steps, the tail zero
    const int rowK = 2 * dk32 + 16, rowV = 2 * DV + 32;                      // bytes; K read as b128 down 16 rows, V by the transposed b64 read
    uint32_t * live = (uint32_t *) fam_lds;
    uint8_t * Ks = fam_lds + 4 * a.map_words, * Vs = Ks + FAM_T * rowK;
    const int64_t n_tiles = (n_kv + FAM_T - 1) / FAM_T;
    const char * kb = a.k + (h / a.gqa_k) * a.k_nb[2] + (b / a.bq_k) * a.k_nb[3];
    const char * vb = a.v + (h / a.gqa_v) * a.v_nb[2] + (b / a.bq_v) * a.v_nb[3];
    const bool m_vec8 = a.m && ((((uintptr_t) a.m) | (uintptr_t) a.m_nb1) & 7) == 0;

    // ---- which tiles are live: wave w looks at tiles w, w + 4, ..; lane = query row of the workgroup
    if (a.m) {
        for (int i = tid; i < a.map_words; i += 256) live[i] = 0;
        __syncthreads();
        const int64_t lim = n_tiles < (int64_t) a.map_words * 32 ? n_tiles : (int64_t) a.map_words * 32;
        const bool m_vec16 = ((((uintptr_t) a.m) | (uintptr_t) a.m_nb1) & 15) == 0;
        const bool row_ok = n0 + lane < N;
        const char * mr = a.m + (row_ok ? n0 + lane : n0) * a.m_nb1;
        for (int64_t t = wave; t < lim; t += 4) {
            const int64_t j0 = t * FAM_T;
            bool any = false;
            if (row_ok) {
                if (m_vec16 && j0 + FAM_T <= n_kv) {
                    const uint4 * p = (const uint4 *) (mr + 2 * j0);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const uint4 w = p[i];
                        const uint32_t x[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
                        for (int u = 0; u < 4; ++u) any = any || (x[u] & 0xFFFFu) != 0xFC00u || (x[u] >> 16) != 0xFC00u;
                    }
                } else {
                    const int64_t cnt = n_kv - j0 < FAM_T ? n_kv - j0 : FAM_T;
                    const uint16_t * p = (const uint16_t *) (mr + 2 * j0);
                    for (int64_t i = 0; i < cnt; ++i) any = any || p[i] != 0xFC00u;
                }
            }
            if (__ballot(any) != 0ull && lane == 0) atomicOr(&live[t >> 5], 1u << (t & 31));
        }
        __syncthreads();
    }
    auto next_live = [&](int64_t t) -> int64_t {                              // the first live tile >= t (uniform)
        if (!a.m) return t;
        while (t < n_tiles && t < (int64_t) a.map_words * 32 && !((live[t >> 5] >> (t & 31)) & 1u)) ++t;
        return t;
    };

    // ---- this wave's q rows as B fragments: lane holds row c16, elements 32 kk + 8 g .. + 7, rounded to f16 once
    const int64_t tq = n0 + 16 * wave + c16, tq_c = tq < N ? tq : N - 1;      // (rows past N repeat the last row and are not stored)
    fam_h8 qf[DKB / 32];
    {
        const char * qp = a.q + tq_c * a.q_nb[1] + h * a.q_nb[2] + b * a.q_nb[3];
#pragma unroll
        for (int kk = 0; kk < DKB / 32; ++kk) {
            const int e = 32 * kk + 8 * g;
            float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
            if (e < DK) { f0 = *(const float4 *) (qp + 4 * e); f1 = *(const float4 *) (qp + 4 * e + 16); }
            if constexpr (BF) qf[kk] = (fam_h8) { fam_bf16_bits(f0.x), fam_bf16_bits(f0.y), fam_bf16_bits(f0.z), fam_bf16_bits(f0.w), fam_bf16_bits(f1.x), fam_bf16_bits(f1.y), fam_bf16_bits(f1.z), fam_bf16_bits(f1.w) };
            else qf[kk] = (fam_h8) { (_Float16) f0.x, (_Float16) f0.y, (_Float16) f0.z, (_Float16) f0.w, (_Float16) f1.x, (_Float16) f1.y, (_Float16) f1.z, (_Float16) f1.w };
        }
    }
    const float slope = a.max_bias > 0.0f ? ((uint32_t) h < a.n_head_log2 ? powf(a.m0, (float) (h + 1)) : powf(a.m1, (float) (2 * (h - (int) a.n_head_log2) + 1))) : 1.0f;
    const char * mrow = a.m ? a.m + tq_c * a.m_nb1 : nullptr;

    fam_f4 O[DVB / 16];
#pragma unroll
    for (int c = 0; c < DVB / 16; ++c) O[c] = (fam_f4) { 0.f, 0.f, 0.f, 0.f };
    float mx = -INFINITY, sum = 0.0f;                                         // the row's running maximum; THIS LANE's part of its running sum

    // ---- staging: thread -> (tile row tid >> 2, 16-byte chunks (tid & 3) + 4 i of that row); the next tile's loads fly under this tile's MFMAs
    const int srow = tid >> 2, sseg = tid & 3;
    uint4 kr[DKB / 32], vr[DVB / 32];                                         // (a block cache: the raw bytes of fam_fetch_blk, decoded on the way into LDS)
    bool row_ok = false;                                                      // the staged row lies inside the window
    uint2 mr4[4];                                                             // this lane's 16 mask values of the tile: positions 16 blk + 4 g .. + 3
    auto fetch = [&](int64_t t) {
        const int64_t j = t * FAM_T + srow;
        const bool ok = j < n_kv;
        if constexpr (QK || QV) row_ok = ok;
        const char * kp = kb + (ok ? j : 0) * a.k_nb[1], * vp = vb + (ok ? j : 0) * a.v_nb[1];
#pragma unroll
        for (int i = 0; i < DKB / 32; ++i) {
            const int e = 8 * (sseg + 4 * i);
            kr[i] = make_uint4(0, 0, 0, 0);
            if constexpr (QK) { if (ok && 32 * i < DK) fam_fetch_blk<KVT>(kp + kv_block_bytes<KVT>() * i, sseg, a.k_al4 != 0, (kv_block_bytes<KVT>() * i) & 3, kr[i]); }
            else if (ok && e < DK) kr[i] = *(const uint4 *) (kp + 2 * e);
        }
#pragma unroll
        for (int i = 0; i < DVB / 32; ++i) {
            const int e = 8 * (sseg + 4 * i);
            vr[i] = make_uint4(0, 0, 0, 0);
            if constexpr (QV) { if (ok && 32 * i < DV) fam_fetch_blk<VVT>(vp + kv_block_bytes<VVT>() * i, sseg, a.v_al4 != 0, (kv_block_bytes<VVT>() * i) & 3, vr[i]); }
            else if (ok && e < DV) vr[i] = *(const uint4 *) (vp + 2 * e);
        }
        if (mrow) {
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) {
                const int64_t jm = t * FAM_T + 16 * blk + 4 * g;
                if (m_vec8 && jm + 4 <= n_kv) mr4[blk] = *(const uint2 *) (mrow + 2 * jm);
                else {
                    uint32_t x[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[r] = jm + r < n_kv ? *(const uint16_t *) (mrow + 2 * (jm + r)) : 0xFC00u;
                    mr4[blk] = make_uint2(x[0] | (x[1] << 16), x[2] | (x[3] << 16));
                }
            }
        }
    };

    int64_t t = next_live(0);
    if (t < n_tiles) fetch(t);
    while (t < n_tiles) {
        __syncthreads();                                                      // the previous tile's fragments have been read
#pragma unroll
        for (int i = 0; i < DKB / 32; ++i) if (8 * (sseg + 4 * i) < dk32) {
            if constexpr (QK) *(uint4 *) (Ks + srow * rowK + 16 * (sseg + 4 * i)) = row_ok ? fam_decode_blk<KVT>(kr[i], sseg) : make_uint4(0, 0, 0, 0);
            else *(uint4 *) (Ks + srow * rowK + 16 * (sseg + 4 * i)) = kr[i];
        }
#pragma unroll
        for (int i = 0; i < DVB / 32; ++i) if (8 * (sseg + 4 * i) < DV) {
            if constexpr (QV) *(uint4 *) (Vs + srow * rowV + 16 * (sseg + 4 * i)) = row_ok ? fam_decode_blk<VVT>(vr[i], sseg) : make_uint4(0, 0, 0, 0);
            else *(uint4 *) (Vs + srow * rowV + 16 * (sseg + 4 * i)) = vr[i];
        }
        uint2 mk[4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) mk[blk] = mr4[blk];
        const int64_t j0 = t * FAM_T;
        __syncthreads();
        t = next_live(t + 1);
        if (t < n_tiles) fetch(t);

        // ---- S^T = K q: four blocks of 16 positions
        fam_f4 S[4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) S[blk] = (fam_f4) { 0.f, 0.f, 0.f, 0.f };
#pragma unroll
        for (int kk = 0; kk < DKB / 32; ++kk) {
            if (32 * kk < DK) {
#pragma unroll
                for (int blk = 0; blk < 4; ++blk) {
                    const fam_h8 kf = *(const fam_h8 *) (Ks + (16 * blk + c16) * rowK + 2 * (32 * kk + 8 * g));
                    S[blk] = fam_mfma<BF>(kf, qf[kk], S[blk]);
                }
            }
        }
        // ---- scale, soft-cap, mask; the row's new maximum
        float tmax = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            const uint32_t mw[2] = { mk[blk].x, mk[blk].y };
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = S[blk][r] * a.scale;
                if (a.softcap != 0.0f) s = a.softcap * tanhf(s);
                if (mrow) {
                    const uint16_t hb = (uint16_t) (mw[r >> 1] >> (16 * (r & 1)));
                    const float mv = slope * __half2float(__ushort_as_half(hb));
                    s = mv == -INFINITY ? -INFINITY : s + mv;                  // (also the positions past n_kv of the last tile)
                } else if (j0 + 16 * blk + 4 * g + r >= n_kv) s = -INFINITY;
                S[blk][r] = s;
                tmax = fmaxf(tmax, s);
            }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mnew = fmaxf(mx, tmax);
        const float alpha = mnew == -INFINITY ? 1.0f : expf(mx - mnew);       // (mx = -inf: exp(-inf) = 0, O and sum are still 0)
        mx = mnew;
        sum *= alpha;
        fam_h8 pf[2];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = mnew == -INFINITY ? 0.0f : expf(S[blk][r] - mnew);      // a masked position: exp(-inf) = 0 exactly
                sum += p;
                if constexpr (BF) pf[blk >> 1][4 * (blk & 1) + r] = fam_bf16_bits(p);
                else pf[blk >> 1][4 * (blk & 1) + r] = (_Float16) p;
            }
        // ---- O^T = O^T alpha + V^T P
#pragma unroll
        for (int c = 0; c < DVB / 16; ++c) {
            if (16 * c < DV) {
                O[c] *= alpha;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const uint8_t * vp = Vs + (32 * s + 4 * g + (c16 >> 2)) * rowV + 2 * (16 * c + 4 * (c16 & 3));
                    const fam_h4 lo = fam_read_tr(vp), hi = fam_read_tr(vp + 16 * rowV);
                    const fam_h8 vf = { lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3] };
                    O[c] = fam_mfma<BF>(vf, pf[s], O[c]);
                }
            }
        }
    }
    // ---- dst[e][h][t][b] = O^T[e][t] / sum_t; lane holds e = 16 c + 4 g + r
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (tq < N) {
        const float inv = sum > 0.0f ? 1.0f / sum : 0.0f;                     // (a row with every position masked: zeros)
        char * dp = a.d + h * a.d_nb[1] + tq * a.d_nb[2] + b * a.d_nb[3];
#pragma unroll
        for (int c = 0; c < DVB / 16; ++c) {
            if (16 * c < DV) {
#pragma unroll
                for (int r = 0; r < 4; ++r) *(float *) (dp + (int64_t) (16 * c + 4 * g + r) * a.d_nb[0]) = O[c][r] * inv;
            }
        }
    }
}

template <int DKB, int DVB, int KVT, int VVT = KVT>
static hipError_t fam_launch_t(const FamArgs & a, dim3 grid, size_t lds, hipStream_t st) {
    static bool attr_set[64] = {};
    if (lds > 48 * 1024) {
        int dev = 0; (void) hipGetDevice(&dev); dev = dev >= 0 && dev < 64 ? dev : 0;
        if (!attr_set[dev]) {
            const hipError_t e = hipFuncSetAttribute((const void *) k_flash_attn_mfma<DKB, DVB, KVT, VVT>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
            if (e != hipSuccess) return e;
            attr_set[dev] = true;
        }
    }
    hipLaunchKernelGGL((k_flash_attn_mfma<DKB, DVB, KVT, VVT>), grid, dim3(256), lds, st, a);
    return hipGetLastError();
}

// the nine (DKB, DVB) buckets of one cache type
template <int KVT>
static hipError_t fam_launch_buckets(const FamArgs & a, dim3 grid, size_t lds, hipStream_t st) {
    const int kc = a.DK <= 64 ? 0 : a.DK <= 128 ? 1 : 2, vc = a.DV <= 64 ? 0 : a.DV <= 128 ? 1 : 2;
    switch (3 * kc + vc) {
        case 0: return fam_launch_t<64, 64, KVT>(a, grid, lds, st);
        case 1: return fam_launch_t<64, 128, KVT>(a, grid, lds, st);
        case 2: return fam_launch_t<64, 256, KVT>(a, grid, lds, st);
        case 3: return fam_launch_t<128, 64, KVT>(a, grid, lds, st);
        case 4: return fam_launch_t<128, 128, KVT>(a, grid, lds, st);
        case 5: return fam_launch_t<128, 256, KVT>(a, grid, lds, st);
        case 6: return fam_launch_t<256, 64, KVT>(a, grid, lds, st);
        case 7: return fam_launch_t<256, 128, KVT>(a, grid, lds, st);
        default: return fam_launch_t<256, 256, KVT>(a, grid, lds, st);
    }
}
// the other cache types' buckets: fattn_mfma_kva.hip (Q8_0, Q4_0, Q4_1, bf16), fattn_mfma_kvb.hip (Q5_0, Q5_1, IQ4_NL)
__attribute__((visibility("hidden"))) hipError_t fam_launch_kva(int type, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st);
__attribute__((visibility("hidden"))) hipError_t fam_launch_kvb(int type, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st);

// ---- a mixed cache (K type != V type): the pairs with f16 or Q8_0 on at least one side, head sizes of ONE bucket -- 22 pairs, 66 kernels
__host__ __device__ constexpr bool fam_mix_anchor(int t) { return t == 1 || t == MI355Q_TYPE_Q8_0; }
inline bool fam_mix_built(int kt, int vt, int64_t DK, int64_t DV) {
    const auto seven = [](int t) { return t == 1 || fam_is_blocks(t); };
    const auto bucket = [](int64_t d) { return d <= 64 ? 0 : d <= 128 ? 1 : 2; };
    return kt != vt && seven(kt) && seven(vt) && (fam_mix_anchor(kt) || fam_mix_anchor(vt)) && bucket(DK) == bucket(DV);
}
template <int KVT, int VVT>
static hipError_t fam_launch_diag(const FamArgs & a, dim3 grid, size_t lds, hipStream_t st) {
    if (a.DK <= 64)  return fam_launch_t<64, 64, KVT, VVT>(a, grid, lds, st);
    if (a.DK <= 128) return fam_launch_t<128, 128, KVT, VVT>(a, grid, lds, st);
    return fam_launch_t<256, 256, KVT, VVT>(a, grid, lds, st);
}
// all block types on the free side of an anchor: ANCHOR_K ? K = ANCHOR, V = type : K = type, V = ANCHOR; WITH_ANCHORS: the other anchor type too
template <int ANCHOR, bool ANCHOR_K, bool WITH_ANCHORS>
static hipError_t fam_launch_mix_side(int type, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st) {
#define FAM_MIX_CASE(T) case T: if constexpr (ANCHOR_K) return fam_launch_diag<ANCHOR, T>(a, grid, lds, st); else return fam_launch_diag<T, ANCHOR>(a, grid, lds, st);
    if constexpr (WITH_ANCHORS) {
        constexpr int OTHER = ANCHOR == 1 ? MI355Q_TYPE_Q8_0 : 1;
        if (type == OTHER) { if constexpr (ANCHOR_K) return fam_launch_diag<ANCHOR, OTHER>(a, grid, lds, st); else return fam_launch_diag<OTHER, ANCHOR>(a, grid, lds, st); }
    }
    switch (type) {
        FAM_MIX_CASE(MI355Q_TYPE_Q4_0) FAM_MIX_CASE(MI355Q_TYPE_Q4_1) FAM_MIX_CASE(MI355Q_TYPE_Q5_0) FAM_MIX_CASE(MI355Q_TYPE_Q5_1) FAM_MIX_CASE(MI355Q_TYPE_IQ4_NL)
        default: return hipErrorInvalidValue;
    }
#undef FAM_MIX_CASE
}
// fattn_mfma_mxa.hip (K f16), _mxb.hip (K Q8_0), _mxc.hip (V f16, K of the other five), _mxd.hip (V Q8_0, K of the other five)
__attribute__((visibility("hidden"))) hipError_t fam_launch_mxa(int vtype, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st);
__attribute__((visibility("hidden"))) hipError_t fam_launch_mxb(int vtype, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st);
__attribute__((visibility("hidden"))) hipError_t fam_launch_mxc(int ktype, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st);
__attribute__((visibility("hidden"))) hipError_t fam_launch_mxd(int ktype, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st);

} // namespace mi355q
