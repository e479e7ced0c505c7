// gemv_float.hip -- token generation over UNQUANTIZED weights: y[n][m] = W[m][:] . x[n][:], W an f16 or bf16 matrix read once per token, x f32 with
// 1 <= n <= 8 columns, y f32.  The arithmetic is the reference CPU backend's AVX2 build, bit for bit:
//   f16   x rounded to f16 once (round to nearest even); ggml_vec_dot_f16 (ggml-cpu/vec.cpp:128-168): 32-element steps, four accumulators of 8 lanes fed by
//         an f32 fma, GGML_F16_VEC_REDUCE: (a0 + a2) + (a1 + a3) = s[0..7], t[i] = s[i] + s[i + 4], (t0 + t1) + (t2 + t3)          (fa_row.cuh fa_dot_f16_seq)
//   bf16  x rounded by ggml_compute_fp32_to_bf16 (NaN made quiet as (bits >> 16) | 0x40); ggml_vec_dot_bf16's AVX2 branch: multiply THEN add,
//         (c1 + c3) + (c2 + c4), high half + low half, movehl, movehdup = (g0 + g2) + (g1 + g3)                               (ops_glue.hip k_mul_mat_f)
// Element i of a 32-element chunk belongs to accumulator (i % 32) / 8, SIMD lane i % 8, and each (row, accumulator, lane) chain walks the chunks in
// order.  A GPU lane that loads 16 bytes loads 8 elements = one whole accumulator of one chunk: FOUR lanes own a row (quad lane q = accumulator q), each
// carries the 8 chains of its accumulator per column and walks the row's chunks in order in groups of 8 (above two columns: 4) with the next group's loads in flight.  The cross-accumulator
// tree is two DPP quad steps, the 8 -> 1 sum stays inside the lane.  Nothing here reorders an addition of the CPU's.
//
// Rows per wave (4, 8 or 16; 16 = every lane busy): the number of lanes that can carry chains is 4 M whatever the launch shape, so for a short matrix
// the question is only WHERE they sit.  Fewer rows per wave spread the same loads over more CUs (each with its own L1 / texture path); the host picks
// the largest count that still gives every one of the 256 CUs a workgroup (fw_rows_per_wave).  Lanes without a row issue no load and store nothing.
//
// Activations: every workgroup rounds x once into LDS in the weight's type ([n][tile] 16-bit values, <= 32 KiB; a long K or many columns go
// tile by tile, the weight loads stay in flight across the tile barriers), one ds_read_b128 per column and chunk.
#include "mi355q_common.h"

namespace mi355q {

constexpr int FW_THREADS = 256, FW_WAVES = FW_THREADS / 64;
constexpr int FW_D_MAX = 8;                                  // chunks per group and lane: 8 with 1 - 2 columns (two groups: 64 VGPRs), 4 above
constexpr int FW_TILE_ALIGN = 64 * FW_D_MAX;                 // a tile is whole pairs of groups: it starts on buffer `cur`, slot 0
constexpr int FW_LDS_ELEMS = 16384;                          // 32 KiB of 16-bit activations per workgroup
constexpr int FW_CUS = 256;                                  // MI355X

#ifdef __HIPCC__

// ggml_compute_fp32_to_bf16 (ggml-impl.h; ops_glue.hip f32_to_bf16): the integer form is the contract, not v_cvt_pk_bf16_f32
__device__ __forceinline__ uint16_t fw_f32_to_bf16(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t) ((u >> 16) | 0x40u);
    return (uint16_t) ((u + (0x7FFFu + ((u >> 16) & 1u))) >> 16);
}

// the 8 elements of 16 bytes, widened exactly to f32
template <bool BF16>
__device__ __forceinline__ void fw_widen(const uint4 v, float (&f)[8]) {
    const uint32_t d[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (BF16) { f[2 * i] = __uint_as_float(d[i] << 16); f[2 * i + 1] = __uint_as_float(d[i] & 0xFFFF0000u); }
        else                { f[2 * i] = h2f(d[i] & 0xFFFFu);         f[2 * i + 1] = h2f(d[i] >> 16); }
    }
}

// one chunk of one row quarter against every column: wv = the lane's 8 weights, xs = its 8 activations of column 0 in LDS
template <bool BF16, int NCOLS>
__device__ __forceinline__ void fw_step(const uint4 wv, const uint16_t * xs, int tile_k, float (&acc)[NCOLS][8]) {
    float wf[8];
    fw_widen<BF16>(wv, wf);
#pragma unroll
    for (int n = 0; n < NCOLS; ++n) {
        float xf[8];
        fw_widen<BF16>(*(const uint4 *) (xs + n * tile_k), xf);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if constexpr (BF16) acc[n][j] = __fadd_rn(__fmul_rn(wf[j], xf[j]), acc[n][j]);      // _mm256_add_ps(_mm256_mul_ps(x, y), c)
            else                acc[n][j] = __builtin_fmaf(wf[j], xf[j], acc[n][j]);            // _mm256_fmadd_ps(x, y, sum)
        }
    }
}

template <bool BF16, int NCOLS>
__global__ void __launch_bounds__(FW_THREADS) k_gemv_fw(const char * __restrict__ w, int64_t w_stride, const char * __restrict__ x, int64_t x_stride,
                                                        char * __restrict__ y, int64_t y_stride, int64_t M, int K, int rpw, int tile_k) {
    extern __shared__ __attribute__((aligned(16))) uint16_t fw_x[];          // [NCOLS][tile_k]: x in the weight's type
    constexpr int FW_D = NCOLS <= 2 ? FW_D_MAX : FW_D_MAX / 2;                // (8 accumulators per column: the load buffers give way)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane & 3, rl = lane >> 2;                                   // accumulator of the row's chunks, row of the wave
    const int64_t row0 = ((int64_t) blockIdx.x * FW_WAVES + wave) * rpw, row = row0 + rl;
    const bool live = rl < rpw && row < M;
    // The hot loop has no divergent branch (one would cost the loads in flight: every join waits for all of them).  A lane without a row loads what the
    // lane rpw rows below it loads -- the same address in the same instruction, no further line -- or the last row's, and stores nothing.
    const int64_t row_ld = row0 + (rl & (rpw - 1)) < M ? row0 + (rl & (rpw - 1)) : M - 1;
    const char * wp = w + row_ld * w_stride + 16 * q;
    const int nchunks = K >> 5;

    // two groups of FW_D chunks: the next group is requested, then the current one is consumed (FW_D 16-byte loads in flight per lane at all times)
    uint4 cur[FW_D], nxt[FW_D];
#pragma unroll
    for (int u = 0; u < FW_D; ++u) cur[u] = ldg16_nt(wp + 64 * (int64_t) (u < nchunks ? u : nchunks - 1));     // in flight during the activation prologue
    float acc[NCOLS][8];
#pragma unroll
    for (int n = 0; n < NCOLS; ++n)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[n][j] = 0.0f;

    for (int k0 = 0; k0 < K; k0 += tile_k) {
        const int tk = K - k0 < tile_k ? K - k0 : tile_k;
        if (k0) __syncthreads();                                              // everyone has read the previous tile
#pragma unroll
        for (int n = 0; n < NCOLS; ++n) {
            const float * xp = (const float *) (x + n * x_stride) + k0;
            for (int i = tid; i < tk; i += FW_THREADS) {
                const float v = xp[i];
                fw_x[n * tile_k + i] = BF16 ? fw_f32_to_bf16(v) : __half_as_ushort(__float2half_rn(v));
            }
        }
        __syncthreads();
        const int c0 = k0 >> 5, c1 = (k0 + tk) >> 5;                          // (c0 is a multiple of 2 FW_D: cur[u] holds chunk c + u)
        const uint16_t * xs = fw_x + 8 * q;
        int c = c0;
        // request the group after this one into `get`, then consume `use` one chunk at a time (the scheduling barriers: hoisting every LDS read and
        // widening of a group costs the registers)
        auto group = [&](const uint4 (&use)[FW_D], uint4 (&get)[FW_D]) {
#pragma unroll
            for (int u = 0; u < FW_D; ++u) {                                  // (past the row's end: its last chunk again, never consumed)
                const int nx = c + FW_D + u;
                get[u] = ldg16_nt(wp + 64 * (int64_t) (nx < nchunks ? nx : nchunks - 1));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < FW_D; ++u) {
                fw_step<BF16, NCOLS>(use[u], xs + 32 * u, tile_k, acc);
                __builtin_amdgcn_sched_barrier(0);
            }
            c += FW_D; xs += 32 * FW_D;
        };
        while (c + 2 * FW_D <= c1) { group(cur, nxt); group(nxt, cur); }      // the two buffers swap roles: no copy waits for a load
        if (c + FW_D <= c1) {                                                 // (an odd group: in the row's last tile only)
            group(cur, nxt);
#pragma unroll
            for (int u = 0; u < FW_D; ++u) cur[u] = nxt[u];
        }
#pragma unroll
        for (int u = 0; u < FW_D; ++u)                                        // the row's last chunks ((K / 32) % FW_D, in the last tile only): nothing to request
            if (c + u < c1) fw_step<BF16, NCOLS>(cur[u], xs + 32 * u, tile_k, acc);
    }
#pragma unroll
    for (int n = 0; n < NCOLS; ++n) {
        float s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = acc[n][j];
            v = __fadd_rn(v, dpp_f<0x4E>(v));                                 // a0 + a2 (quad lanes 0, 2) | a1 + a3 (quad lanes 1, 3)
            v = __fadd_rn(v, dpp_f<0xB1>(v));                                 // (a0 + a2) + (a1 + a3) in quad lane 0
            s[j] = v;
        }
        float r;
        if constexpr (BF16) {
            const float g0 = __fadd_rn(s[4], s[0]), g1 = __fadd_rn(s[5], s[1]), g2 = __fadd_rn(s[6], s[2]), g3 = __fadd_rn(s[7], s[3]);    // high half + low half
            r = __fadd_rn(__fadd_rn(g0, g2), __fadd_rn(g1, g3));                                                                          // movehl, movehdup
        } else {
            const float t0 = __fadd_rn(s[0], s[4]), t1 = __fadd_rn(s[1], s[5]), t2 = __fadd_rn(s[2], s[6]), t3 = __fadd_rn(s[3], s[7]);
            r = __fadd_rn(__fadd_rn(t0, t1), __fadd_rn(t2, t3));
        }
        if (live && q == 0) *(float *) (y + n * y_stride + 4 * row) = r;
    }
}

#endif // __HIPCC__

// rows per wave of a launch: the flag's, or the largest of 16 / 8 / 4 that leaves no CU without a workgroup
static int fw_rows_per_wave(int64_t m, int flags) {
    switch (flags & MI355Q_FW_ROWS_MASK) {
        case MI355Q_FW_ROWS_4:  return 4;
        case MI355Q_FW_ROWS_8:  return 8;
        case MI355Q_FW_ROWS_16: return 16;
    }
    for (int rpw = 16; rpw > 4; rpw >>= 1) if ((m + FW_WAVES * rpw - 1) / (FW_WAVES * rpw) >= FW_CUS) return rpw;
    return 4;
}
static int fw_tile_k(int64_t k, int64_t n) {
    const int64_t cap = FW_LDS_ELEMS / n / FW_TILE_ALIGN * FW_TILE_ALIGN;
    return (int) (k < cap ? k : cap);
}

} // namespace mi355q

using namespace mi355q;

#define FW_FAIL(code, msg) do { mi355q_set_error(msg); return code; } while (0)

extern "C" {

void mi355q_set_error(const char * msg);          // api.hip

int mi355q_mul_mat_fw_path(int type, const void * w, int64_t w_stride_bytes, const float * x, int64_t x_stride_bytes, float * y, int64_t y_stride_bytes,
                           int64_t m, int64_t n, int64_t k, int flags) {
    if (type != MI355Q_T_F16 && type != MI355Q_T_BF16) FW_FAIL(MI355Q_ERR_UNSUPPORTED, "mul_mat_fw: the weight type must be f16 (1) or bf16 (30)");
    if (flags & ~MI355Q_FW_ROWS_MASK) FW_FAIL(MI355Q_ERR_UNSUPPORTED, "mul_mat_fw: unknown flag");
    if (m < 1 || n < 1 || n > 8) FW_FAIL(MI355Q_ERR_UNSUPPORTED, "mul_mat_fw: 1 <= n <= 8 columns and m >= 1 rows");
    if (k < 32 || k % 32 || k > 0x7FFFFFE0) FW_FAIL(MI355Q_ERR_UNSUPPORTED, "mul_mat_fw: k must be a multiple of 32 (the tail the CPU adds in double stays with op_mul_mat_f)");
    if (!w || !x || !y) FW_FAIL(MI355Q_ERR_UNSUPPORTED, "mul_mat_fw: null pointer");
    if ((((uintptr_t) w | (uintptr_t) w_stride_bytes) & 15) || w_stride_bytes < 2 * k) FW_FAIL(MI355Q_ERR_UNSUPPORTED, "mul_mat_fw: the base and the row pitch of w must be multiples of 16 bytes, pitch >= 2 k");
    if ((((uintptr_t) x | (uintptr_t) x_stride_bytes) & 3) || (n > 1 && x_stride_bytes < 4 * k)) FW_FAIL(MI355Q_ERR_UNSUPPORTED, "mul_mat_fw: x rows must be contiguous f32 at a 4-byte aligned pitch >= 4 k");
    if ((((uintptr_t) y | (uintptr_t) y_stride_bytes) & 3) || y_stride_bytes < 4 * m) FW_FAIL(MI355Q_ERR_UNSUPPORTED, "mul_mat_fw: the pitch of y must be 4-byte aligned and >= 4 m");
    // measured slower than op_mul_mat_f (profiles/fw_stream.md): four or more columns over a SHORT, large matrix -- 4 m lanes carry every chain, and with
    // 8 accumulators per column they are too few to hide both the loads and the arithmetic.  Small matrices stay: there the launch dominates either way.
    if (n >= 4 && m < 8192 && m * k >= ((int64_t) 1 << 24)) FW_FAIL(MI355Q_ERR_UNSUPPORTED, "mul_mat_fw: 4 or more columns over a short matrix (m < 8192, m k >= 2^24) stay with op_mul_mat_f");
    const int rows = FW_WAVES * fw_rows_per_wave(m, flags);
    if ((m + rows - 1) / rows > 0x7FFFFFFF) FW_FAIL(MI355Q_ERR_UNSUPPORTED, "mul_mat_fw: too many rows");
    return MI355Q_FW_PATH_STREAM;
}

int mi355q_mul_mat_fw(int type, const void * w, int64_t w_stride_bytes, const float * x, int64_t x_stride_bytes, float * y, int64_t y_stride_bytes,
                      int64_t m, int64_t n, int64_t k, int flags, void * stream) {
    const int path = mi355q_mul_mat_fw_path(type, w, w_stride_bytes, x, x_stride_bytes, y, y_stride_bytes, m, n, k, flags);     // every check stands there once
    if (path < 0) return path;
    const int rpw = fw_rows_per_wave(m, flags), tile_k = fw_tile_k(k, n);
    const dim3 grid((unsigned) ((m + FW_WAVES * rpw - 1) / (FW_WAVES * rpw)));
    const size_t lds = (size_t) n * tile_k * 2;
#define FW_LAUNCH(B, N) hipLaunchKernelGGL((k_gemv_fw<B, N>), grid, dim3(FW_THREADS), lds, (hipStream_t) stream, (const char *) w, w_stride_bytes, (const char *) x, \
                                           x_stride_bytes, (char *) y, y_stride_bytes, m, (int) k, rpw, tile_k)
#define FW_COLS(B) switch (n) { case 1: FW_LAUNCH(B, 1); break; case 2: FW_LAUNCH(B, 2); break; case 3: FW_LAUNCH(B, 3); break; case 4: FW_LAUNCH(B, 4); break; \
                                case 5: FW_LAUNCH(B, 5); break; case 6: FW_LAUNCH(B, 6); break; case 7: FW_LAUNCH(B, 7); break; default: FW_LAUNCH(B, 8); break; }
    if (type == MI355Q_T_BF16) FW_COLS(true) else FW_COLS(false)
#undef FW_COLS
#undef FW_LAUNCH
    if (hipGetLastError() != hipSuccess) FW_FAIL(MI355Q_ERR_HIP, "mul_mat_fw: kernel launch failed");
    return MI355Q_OK;
}

} // extern "C"
