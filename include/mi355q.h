/* mi355q.h -- C-ABI of libmi355q.so: MI355X (gfx950 / CDNA4) kernels for the quantized
 * dequant + mat-vec / mat-mat multiply that dominates llama.cpp token generation.
 *
 * This is the drop-in boundary for the hot path.  Plain pointers and sizes only; no ggml, torch
 * or HIP types appear in any signature (streams are passed as void* = hipStream_t).
 *
 * What each entry point replaces in the reference (paths relative to /root/reference):
 *
 *   mi355q_mul_mat        GGML_OP_MUL_MAT with quantized src0, f32 src1, f32 dst
 *                           CPU : ggml_compute_forward_mul_mat      ggml/src/ggml-cpu/ggml-cpu.c:1266-1458
 *                           GPU : ggml_cuda_mul_mat -> mul_mat_vec_q / mul_mat_q / dequant+GEMM
 *                                 ggml/src/ggml-cuda/ggml-cuda.cu:1877-1938, mmvq.cu:130-288, mmq.cuh:2595-2674
 *   mi355q_mul_mat_id     GGML_OP_MUL_MAT_ID (MoE expert-indirect matmul)
 *                           CPU : ggml_compute_forward_mul_mat_id   ggml/src/ggml-cpu/ggml-cpu.c:1540-1718
 *                           GPU : ggml_cuda_mul_mat_id              ggml/src/ggml-cuda/ggml-cuda.cu:1994-2130
 *   mi355q_quantize_act   activation quantizer run before every quantized matmul
 *                           CPU : from_float of the vec_dot_type    ggml/src/ggml-cpu/ggml-cpu.c:1328-1363,
 *                                 quantize_row_q8_0/q8_1/q8_K       ggml/src/ggml-quants.c:194-253, 2479-2516
 *                           GPU : quantize_q8_1                     ggml/src/ggml-cuda/quantize.cu:4-38
 *   mi355q_weights_upload / _download
 *                         ggml_backend_buffer_i.set_tensor / get_tensor for quantized weights
 *                           ggml/src/ggml-backend-impl.h:41-66 (CUDA: ggml-cuda.cu:568-600); the device keeps a
 *                           coalescing-friendly per-row plane layout, invisible above this ABI
 *   mi355q_row_size / mi355q_type_supported
 *                         ggml_row_size / ggml_backend_device_i.supports_op
 *                           ggml/src/ggml.c (ggml_row_size), ggml/src/ggml-backend-impl.h:137-185
 *
 * The ggml backend plugin (libggml-mi355.so: ggml_backend_init / ggml_backend_score, the four vtables of
 * ggml/src/ggml-backend-impl.h) is a thin C++ host layer over this ABI; see INTEGRATION.md.
 *
 * Numerics contract: activations are quantized exactly as the reference CPU backend does for the weight
 * type (Q8_0 / Q8_1 for the 32-element formats, Q8_K for K-quants and IQ4_XS), every per-block integer dot
 * product is exact, and only the order of the final f32 additions differs from the CPU.
 *
 * All functions return 0 on success, a negative MI355Q_ERR_* otherwise (never throw, never abort).
 * A missing / non-gfx950 device is an error, not a fallback: there is no CPU path in this library.
 */
#ifndef MI355Q_H
#define MI355Q_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355Q_API_VERSION 3

/* error codes */
#define MI355Q_OK                0
#define MI355Q_ERR_UNSUPPORTED  -1   /* type / shape combination not implemented            */
#define MI355Q_ERR_SHAPE        -2   /* inconsistent sizes, K not a multiple of the block   */
#define MI355Q_ERR_ALIGN        -3   /* pointer / stride alignment contract violated        */
#define MI355Q_ERR_HIP          -4   /* a HIP runtime call failed (see mi355q_last_error)   */
#define MI355Q_ERR_WORKSPACE    -5   /* workspace too small                                 */
#define MI355Q_ERR_NO_DEVICE    -6   /* no usable gfx950 device                             */

/* weight / activation type ids are ggml's enum ggml_type values (ggml/include/ggml.h) */
#define MI355Q_TYPE_F32    0
#define MI355Q_TYPE_Q4_0   2
#define MI355Q_TYPE_Q4_1   3
#define MI355Q_TYPE_Q5_0   6
#define MI355Q_TYPE_Q5_1   7
#define MI355Q_TYPE_Q8_0   8
#define MI355Q_TYPE_Q8_1   9
#define MI355Q_TYPE_Q2_K   10
#define MI355Q_TYPE_Q3_K   11
#define MI355Q_TYPE_Q4_K   12
#define MI355Q_TYPE_Q5_K   13
#define MI355Q_TYPE_Q6_K   14
#define MI355Q_TYPE_Q8_K   15
#define MI355Q_TYPE_IQ2_XXS 16
#define MI355Q_TYPE_IQ2_XS  17
#define MI355Q_TYPE_IQ3_XXS 18
#define MI355Q_TYPE_IQ1_S   19
#define MI355Q_TYPE_IQ4_NL  20
#define MI355Q_TYPE_IQ3_S   21
#define MI355Q_TYPE_IQ2_S   22
#define MI355Q_TYPE_IQ4_XS  23
#define MI355Q_TYPE_IQ1_M   29

/* flags for mi355q_mul_mat* / mi355q_quantize_act */
#define MI355Q_FLAG_ROUND_AWAY   0x0  /* Q8_0/Q8_1 activations: q = roundf(x/d)   (quantize_row_q8_0_ref; default) */
#define MI355Q_FLAG_ROUND_EVEN   0x1  /*                        q = rint(x/d)     (what the AVX2 / NEON CPU paths do) */
#define MI355Q_FLAG_FORCE_GENERIC 0x2 /* canonical rows only: keep them on the per-column tier (k_gemv_generic) for N > 8, off the
                                         batched canonical tier.  Planar rows ignore it: no flag sends them to the generic kernel */
#define MI355Q_FLAG_FORCE_GEMV   0x4  /* use the GEMV tier even for large N                                         */
#define MI355Q_FLAG_FORCE_MMQ    0x8  /* use the tiled MFMA tier even for small N                                   */

/* ---- library / device ------------------------------------------------------------------------ */
int          mi355q_api_version(void);
int          mi355q_device_count(void);                 /* number of visible gfx950 devices (0 if none)   */
int          mi355q_set_device(int device);
int          mi355q_device_info(int device, char *name, size_t name_len, size_t *free_bytes, size_t *total_bytes,
                                int *compute_units);
const char * mi355q_last_error(void);                   /* thread-local description of the last failure   */

/* ---- geometry ------------------------------------------------------------------------------------ */
int     mi355q_type_supported(int type);                /* 1 if `type` is accepted as src0 of mul_mat      */
int64_t mi355q_blck_size(int type);
int64_t mi355q_type_size(int type);
int64_t mi355q_row_size(int type, int64_t k);           /* == ggml_row_size(type, k); device rows use the same size */
int     mi355q_act_type(int type);                      /* activation format paired with `type` (CPU's vec_dot_type) */
int     mi355q_weights_are_planar(int type, int64_t k); /* 1 if device rows of (type,k) use the plane layout */

/* ---- thin device-memory helpers (so hosts without a HIP binding can drive the library) ----------- */
int mi355q_malloc(void **dev_ptr, size_t bytes);
int mi355q_free(void *dev_ptr);
int mi355q_memset(void *dev_ptr, int value, size_t bytes, void *stream);
int mi355q_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, void *stream);   /* stream NULL: synchronous */
int mi355q_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, void *stream);
int mi355q_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes, void *stream);
/* pinned (page-locked) host memory: staging for asynchronous set/get_tensor, ggml's host buffer type (ggml-backend-impl.h:137-185 get_host_buffer_type) */
int mi355q_host_malloc(void **host_ptr, size_t bytes);
int mi355q_host_free(void *host_ptr);
/* copy between two devices of this process (hipMemcpyPeerAsync: xGMI where the devices are linked), ordered on `stream` of the CURRENT device */
int mi355q_memcpy_peer(void *dst, int dst_device, const void *src, int src_device, size_t bytes, void *stream);
/* events (ggml_backend_event_*: ggml-backend-impl.h:87-124 event_record / event_wait, :137-185 event_new / event_free / event_synchronize) */
int mi355q_event_create(void **event);
int mi355q_event_destroy(void *event);
int mi355q_event_record(void *event, void *stream);
int mi355q_event_wait(void *stream, void *event);           /* makes `stream` (of any device) wait for the event */
int mi355q_event_synchronize(void *event);
int mi355q_stream_create(void **stream);
int mi355q_stream_destroy(void *stream);
int mi355q_stream_synchronize(void *stream);
int mi355q_device_synchronize(void);

/* ---- weights: canonical ggml rows <-> device rows -------------------------------------------------
 * `nrows` whole rows of `k` elements each.  Device rows have the same byte size and row stride as
 * canonical rows (so row-granular views and MoE expert offsets stay valid); only the order of bytes
 * INSIDE a row changes when mi355q_weights_are_planar(type,k).  dst/src device pointers must be
 * 16-byte aligned.  `stream` may be NULL (default stream); the call returns after the copy is complete. */
int mi355q_weights_upload(int type, void *dst_dev, const void *src_host, int64_t nrows, int64_t k, void *stream);
int mi355q_weights_download(int type, void *dst_host, const void *src_dev, int64_t nrows, int64_t k, void *stream);
/* device-to-device variants (canonical bytes already on the device <-> device rows) */
int mi355q_weights_pack_d2d(int type, void *dst_dev, const void *src_canonical_dev, int64_t nrows, int64_t k, void *stream);
int mi355q_weights_unpack_d2d(int type, void *dst_canonical_dev, const void *src_dev, int64_t nrows, int64_t k, void *stream);

/* ---- activation quantizer --------------------------------------------------------------------------
 * x: f32 device, `n` rows of `k` elements, row stride x_stride_bytes (multiple of 4).
 * out: device, n * mi355q_row_size(act_type,k) bytes, CANONICAL ggml block structs
 *      (block_q8_0 / block_q8_1 / block_q8_K, ggml-common.h:209-227, 329-334), bit-identical to the CPU. */
int mi355q_quantize_act(int act_type, const float *x, int64_t x_stride_bytes, void *out,
                        int64_t n, int64_t k, int flags, void *stream);

/* ---- MUL_MAT -----------------------------------------------------------------------------------------
 * y[n][m] = sum_k W[m][k] * x[n][k]       W: `m` device rows of type `type` (uploaded with
 * mi355q_weights_upload), row stride w_stride_bytes (>= row_size, multiple of 16);
 * x: f32 [n rows of k], row stride x_stride_bytes;  y: f32 [n rows of m], row stride y_stride_bytes.
 * workspace: device scratch of at least mi355q_mul_mat_workspace(type,m,n,k) bytes (may be NULL if 0). */
size_t mi355q_mul_mat_workspace(int type, int64_t m, int64_t n, int64_t k);
int    mi355q_mul_mat(int type, const void *w, int64_t w_stride_bytes,
                      const float *x, int64_t x_stride_bytes,
                      float *y, int64_t y_stride_bytes,
                      int64_t m, int64_t n, int64_t k,
                      void *workspace, size_t workspace_bytes, int flags, void *stream);

/* Several weight matrices against the SAME activations in one launch (wq/wk/wv, ffn_gate/ffn_up):
 * y_i[n][m_i] = W_i . x.  All W_i share type-independent k and n; types may differ per matrix.  */
typedef struct mi355q_mat {
    int         type;
    const void *w;
    int64_t     w_stride;   /* bytes between weight rows (>= row_size, multiple of 16 for planar rows) */
    float      *y;
    int64_t     y_stride;   /* bytes between output rows (one per activation row)                      */
    int64_t     m;
} mi355q_mat;
int    mi355q_mul_mat_multi(const mi355q_mat *mats, int n_mats,
                            const float *x, int64_t x_stride_bytes, int64_t n, int64_t k,
                            void *workspace, size_t workspace_bytes, int flags, void *stream);

/* ---- MUL_MAT_ID ---------------------------------------------------------------------------------------
 * y[t][u][:] = W[ids[t][u]] . x[t][u % x_ne1][:]
 * w: n_expert consecutive matrices of m device rows each (expert stride = expert_stride_bytes);
 * x: f32 [n_tok][x_ne1][k] contiguous rows with strides x_stride1_bytes (slot) and x_stride2_bytes (token);
 * ids: i32 device [n_tok][n_used] with row stride ids_stride_bytes;  y: f32 [n_tok][n_used][m] contiguous.
 * The expert ids are read ON THE DEVICE at every size (no host round trip: the call stays capturable).  Up to 16 (token, slot) pairs every
 * pair is one GEMV column; from 17 pairs on (prefill) the pairs are counting-sorted by expert on the device into tile-aligned segments,
 * gathered, multiplied by ONE launch of the matrix-core tier over all experts and scattered back (the reference groups on the host behind a
 * stream synchronize, ggml-cuda.cu:2008-2011); size the workspace with mi355q_mul_mat_id_workspace.  A pair whose expert id is out of range
 * [0, n_expert) -- the reference asserts on it -- gets an output row of NaN on every path. */
size_t mi355q_mul_mat_id_workspace(int type, int64_t m, int64_t k, int64_t n_used, int64_t n_tok, int64_t x_ne1, int64_t n_expert);
int    mi355q_mul_mat_id(int type, const void *w, int64_t w_stride_bytes, int64_t expert_stride_bytes, int64_t n_expert,
                         const float *x, int64_t x_ne1, int64_t x_stride1_bytes, int64_t x_stride2_bytes,
                         const int32_t *ids, int64_t ids_stride_bytes,
                         float *y, int64_t m, int64_t k, int64_t n_used, int64_t n_tok,
                         void *workspace, size_t workspace_bytes, int flags, void *stream);

/* ---- decode plan: the token's dependent chain as ONE persistent launch ----------------------------------------------
 * Replaces the reference's per-node launches + CUDA-graph replay of the token-generation graph
 * (ggml-cuda.cu:2470-2781, evaluate_and_capture_cuda_graph / ggml_backend_cuda_graph_compute): the N = 1 nodes of a
 * decode step -- the quantized MUL_MATs AND the glue between them -- run as an ordered list of STAGES inside one
 * cooperative launch of one workgroup per CU.
 *
 * GEMV stage: 1..4 weight matrices (planar device rows, types may differ) against one activation vector x[k];
 *   y_i[m_i] = W_i . x exactly as mi355q_mul_mat computes it (bit-identical for the same x).  x is formed in the
 *   stage's prologue from f32 vectors of k elements (every workgroup does it for itself, into LDS):
 *     MI355Q_X_PLAIN      x = x0
 *     MI355Q_X_NORM       t = x0 (+ x1);  [sum_out = t;]  x = rms_norm(t, eps) (* norm_w)     ADD -> RMS_NORM -> MUL of build_norm
 *     MI355Q_X_UNARY_MUL  x = unary(x0) * x1      (x_unary: MI355Q_UNARY_SILU / _RELU / _SIGMOID)   build_ffn LLM_FFN_SILU + LLM_FFN_PAR
 *   with the f32 operations of the CPU ops (same expressions as mi355q_op_add_rms_norm_mul / mi355q_op_unary_mul).
 * ATTN stage: rope of q and k, the K / V cache stores of this token and causal attention of ONE token over an f16 KV cache
 *   (ROPE, CPY, MUL_MAT(k,q), SOFT_MAX, MUL_MAT(v,kq) / FLASH_ATTN_EXT of build_attn_mha, src/llama-graph.cpp:1140-1260): see mi355q_attn.
 *
 * Dependencies are DATA-DRIVEN: an operand (x0, x1, q, k, v) whose address range lies inside an output (mats[i].y, sum_out,
 * attn.out) of an EARLIER stage of the plan is a value produced during the run: the producers publish every element as an
 * 8-byte {value, tag} granule in a plan-private buffer and the consumers poll the granules they need -- there is no grid-wide
 * barrier and no flag.  Any other operand must be complete before the launch.  Weights stream across stage boundaries.
 * Plain f32 copies of the outputs are stored at mats[i].y / sum_out / attn.out unless MI355Q_STAGE_NO_PLAIN is set (set it for
 * intermediates nobody outside the plan reads: a caller whose allocator reuses their memory must).
 * Only weight types with a planar layout at this k (mi355q_weights_are_planar) are accepted.
 * run(): asynchronous on `stream`.  status(): synchronizes; 1 = a poll timed out (plan unusable).                         */
#define MI355Q_STAGE_DEPENDS  0x1    /* (API version 1; accepted and ignored: dependencies follow from the operand addresses) */
#define MI355Q_STAGE_NO_PLAIN 0x2    /* do not store plain f32 copies of this stage's outputs                               */
/* ATTN stages over a QUANTIZED KV cache (-ctk T -ctv T, T = q8_0 / q4_0 / q4_1 / q5_0 / q5_1 / iq4_nl): both the K and the V cache hold blocks of
 * that type (no bit: f16; at most one bit).  Block b (32 elements) of kv head g's row at position j is at  cache + j*nb_pos + g*nb_head + b*BB,
 * BB = 34 (q8_0), 18 (q4_0), 20 (q4_1), 22 (q5_0), 24 (q5_1), 18 (iq4_nl); addresses and strides must be even.  Only the flash layout (V rows per
 * position, v_nb_dim = BB) is taken, with head_dim % 32 == 0.  This token's K and V rows are quantized as mi355q_op_cpy (f32 -> T) quantizes
 * them and stored as contiguous rows at *k_dst / *v_dst (v_dst_nb is ignored); the scores and P.V read them back as blocks, as the CPU does.
 * One split per head: the output is mi355q_op_flash_attn_ext's on the same cache, bit for bit; several (windows above 256 positions) merge
 * per-split F32 accumulators.  plan_create refuses a window whose per-split K / V blocks do not fit the LDS (the message
 * gives the type's limit) and the ring engine (MI355Q_PLAN_ENGINE=ring).
 * The q4_1 / q5_0 / q5_1 / iq4_nl bits were added without a change of MI355Q_API_VERSION (no function or structure changed): a library older
 * than them does not know the bits and reads such a stage as an f16 cache.  A caller that may meet an older library checks first that
 * mi355q_op_flash_attn_ext accepts k / v of the type (MI355Q_ERR_UNSUPPORTED otherwise), as it does for the ops it dispatches.               */
#define MI355Q_STAGE_KV_Q8_0  0x4
#define MI355Q_STAGE_KV_Q4_0  0x8
#define MI355Q_STAGE_KV_Q4_1   0x10
#define MI355Q_STAGE_KV_Q5_0   0x20
#define MI355Q_STAGE_KV_Q5_1   0x40
#define MI355Q_STAGE_KV_IQ4_NL 0x80
/* ATTN stages over MIXED K / V cache types (-ctk A -ctv B): a MI355Q_STAGE_KVV_* bit names V's type (at most one bit), and
 * the MI355Q_STAGE_KV_* bits above then name K's type alone (no bit: f16).  Without a KVV bit the KV bits keep their meaning: K and V both have
 * that type.  A KVV bit equal to K's type is the same-type stage, with the same bits.  Each side keeps its own layout: a block side as above
 * (cache + j*nb_pos + g*nb_head + b*BB, even addresses and strides, head_dim % 32 == 0, this token's row stored as mi355q_op_cpy f32 -> the
 * side's type stores it), an f16 side as the f16 stage has it (rows per position, v_nb_dim = 2; this token's row rounded to f16, V through
 * v_dst_nb).  Only the flash layout.  The scores follow K's type (q to its vec_dot_type, its vec_dot), the accumulator V's (f16: the F16
 * accumulator; a block type: F32 over its to_float).  One split per head: the output is mi355q_op_flash_attn_ext2's with MI355Q_FA_KV_MIXED on
 * the same cache, bit for bit.  Several splits: a block V merges per-split F32 accumulators as the same-type stages do; an f16 V is not merged --
 * its splits score in parallel and then continue ONE F16-accumulator walk, split after split, which is the single walk bit for bit.  plan_create refuses a window whose
 * per-split rows of both sides do not fit the LDS (the message names the pair and its limit), the transposed V layout, head sizes that are not
 * whole blocks, odd addresses or strides on a block side, and the ring engine (MI355Q_PLAN_ENGINE=ring); there is no bit for bf16.
 * The bits were added without a change of MI355Q_API_VERSION (no function or structure changed): a library older than them does not know
 * them and reads such a stage as a same-type cache of K's type.  A caller that may meet an older library probes once: mi355q_plan_create
 * of an ATTN stage with two KVV bits set fails with MI355Q_ERR_UNSUPPORTED in a library that knows them (nothing is launched) and not in one
 * that does not.                                                                                                                               */
#define MI355Q_STAGE_KVV_F16    0x100
#define MI355Q_STAGE_KVV_Q8_0   0x200
#define MI355Q_STAGE_KVV_Q4_0   0x400
#define MI355Q_STAGE_KVV_Q4_1   0x800
#define MI355Q_STAGE_KVV_Q5_0   0x1000
#define MI355Q_STAGE_KVV_Q5_1   0x2000
#define MI355Q_STAGE_KVV_IQ4_NL 0x4000
#define MI355Q_STAGE_GEMV 0
#define MI355Q_STAGE_ATTN 1
#define MI355Q_X_PLAIN     0
#define MI355Q_X_NORM      1
#define MI355Q_X_UNARY_MUL 2
typedef struct mi355q_rope_params {      /* the op_params of GGML_OP_ROPE (ggml.c ggml_rope_impl) */
    int   n_dims, mode, n_ctx_orig;
    float freq_base, freq_scale, ext_factor, attn_factor, beta_fast, beta_slow;
} mi355q_rope_params;
/* One token's attention.  q [n_head*head_dim], k, v [n_head_kv*head_dim]: f32 outputs of earlier stages (or complete before the launch).
 * Cache element (position j, dim d, kv head g) is an f16 at  k_cache + j*k_nb_pos + g*k_nb_head + 2*d   and
 * v_cache + j*v_nb_pos + d*v_nb_dim + g*v_nb_head  (v_nb_dim == 2: rows per position, the -fa layout; v_nb_pos == 2: the transposed
 * V cache of the non-flash graph).  This token's roped K row (f16, n_head_kv*head_dim contiguous) is stored at *k_dst and element
 * e of its V row at *v_dst + e*v_dst_nb; k_dst / v_dst are DEVICE slots holding the destination pointers, so that the caller moves the
 * store position every token without rebuilding the plan (cf. mi355q_op_cpy_indirect); the token attends to positions [0, n_kv) with
 * the additive mask row `mask` (f32 or f16, n_kv entries, may be NULL = no masking), as soft_max_ext(kq*scale + mask) does; the row
 * being stored is read from the registers, not from the cache.  out [n_head*head_dim] f32.  rope.mode 0 (normal) or 2 (neox).           */
typedef struct mi355q_attn {
    const float   *q, *k, *v;
    const int32_t *pos;              /* device: the token's position (rope angle)                */
    mi355q_rope_params rope;
    const float   *freq_factors;     /* optional rope frequency factors [n_dims/2]               */
    const void    *k_cache, *v_cache;
    int64_t        k_nb_pos, k_nb_head, v_nb_pos, v_nb_dim, v_nb_head;
    void * const  *k_dst, * const *v_dst;
    int64_t        v_dst_nb;
    const void    *mask;
    int            mask_f16;
    int            n_head, n_head_kv, head_dim, n_kv;
    float          scale;
    float         *out;
    const int32_t *n_kv_dev;         /* optional, device: the window length of THIS run (<= n_kv, which then is the maximum the plan is sized for) */
    int64_t        q_id, k_id, v_id, out_id;   /* value ids (see mi355q_stage); 0 = identify by address */
} mi355q_attn;
typedef struct mi355q_stage {
    mi355q_mat   mats[4];    /* GEMV: y_stride is unused (one activation row) */
    int          n_mats;
    int          flags;
    const float *x;          /* GEMV: x0, device, k floats */
    int64_t      k;
    /* --- API version 2 --- */
    int          kind;       /* MI355Q_STAGE_GEMV (0) / MI355Q_STAGE_ATTN */
    int          x_kind;     /* MI355Q_X_* */
    int          x_unary;
    float        eps;
    const float *x1;         /* second operand (X_NORM: optional addend; X_UNARY_MUL: the multiplier) */
    const float *norm_w;     /* X_NORM: optional weight vector [k] (complete before the launch)        */
    float       *sum_out;    /* X_NORM with x1: where t = x0 + x1 is stored (the next residual's operand), optional */
    const mi355q_attn *attn; /* MI355Q_STAGE_ATTN */
    /* VALUE IDS (optional, 0 = unused).  By default an operand is matched to the earlier output whose ADDRESS range contains it.  A caller
     * whose allocator hands the same memory to several intermediates of one graph (ggml_gallocr does: K's projection reuses the dead pre-rope
     * Q's block, V's reuses K's) cannot be matched that way once the plan reorders consumers behind later producers.  Such a caller labels
     * every output with a unique non-zero id (y_id[i] for mats[i].y, sum_id for sum_out, attn->out_id) and every operand with the id of the
     * value it means (x_id, x1_id, attn->q_id / k_id / v_id; 0 = a plain vector complete before the launch): ids then decide, addresses
     * only give the offset of a sub-vector inside the labelled output.  Any non-zero value is an id, negative ones included.  An x_out vector
     * has no id: no operand of a later stage can name it, by id or by address (plan_create refuses both).                                    */
    int64_t      y_id[4], sum_id, x_id, x1_id;
    /* OUTPUT FORM.  MI355Q_Y_ROWS (0): y_i = W_i . x, one vector per matrix.  MI355Q_Y_UNARY_MUL: n_mats == 2, same type and m; the stage
     * publishes ONE vector  y = unary(W_0 . x) * (W_1 . x)  of m elements at mats[0].y (id y_id[0]; mats[1].y is unused): UNARY -> MUL of
     * build_ffn (LLM_FFN_SILU + LLM_FFN_PAR) folded into the producer, so that ffn_down gathers one vector instead of two.  Every workgroup
     * computes matching rows of both matrices; same f32 expressions as mi355q_op_unary_mul.                                                   */
    int          y_kind, y_unary;
    /* --- API version 3 --- */
    float       *x_out;      /* X_NORM / X_UNARY_MUL: optional; the activation vector the prologue forms (rms_norm(.) * w, unary(.) * x1) is ALSO
                              * stored here as plain f32 -- for a caller whose graph hands that vector to somebody besides this stage's matrices
                              * (llama.cpp: result_norm is read back as the embeddings; a LoRA branch multiplies it again).  One workgroup stores it. */
} mi355q_stage;
#define MI355Q_Y_ROWS      0
#define MI355Q_Y_UNARY_MUL 1
typedef struct mi355q_plan mi355q_plan;
int     mi355q_plan_create(mi355q_plan **out, const mi355q_stage *stages, int n_stages, int flags);
int     mi355q_plan_run(mi355q_plan *plan, void *stream);
int     mi355q_plan_status(mi355q_plan *plan);
/* test hook: set the plan's run counter (the source of the granule tags' epoch); a value near the 32-bit wrap exercises the granule reset */
int     mi355q_plan_debug_set_runs(mi355q_plan *plan, unsigned long long runs);
/* diagnostics of an aborted plan: its 32 sync words (0: abort flag; 1..7: kind of the wait that gave up, stage, workgroup, wave, two operands, landed pages) */
int     mi355q_plan_debug_words(mi355q_plan *plan, unsigned *out32);
/* asynchronous form: enqueues a 4-byte device-to-host copy of the plan's abort word into *host_flag (pinned memory recommended) on `stream`;
 * after the stream has been synchronized, *host_flag != 0 means a poll of an earlier run timed out.                                       */
int     mi355q_plan_status_async(mi355q_plan *plan, unsigned *host_flag, void *stream);
int64_t mi355q_plan_weight_bytes(const mi355q_plan *plan);
int     mi355q_plan_launch_stages(const mi355q_plan *plan);
int     mi355q_plan_destroy(mi355q_plan *plan);

/* ---- residency ops: the small f32/f16 graph ops between the quantized matmuls of a decode graph ------
 * Tensors are described the ggml way: ne[] elements per dimension, nb[] strides in BYTES (views, permutes and broadcasts
 * are expressed through them), data = device pointer.  type: MI355Q_T_F32 / MI355Q_T_F16, and MI355Q_T_BF16 (ggml's id 30, a bf16 KV cache)
 * where an op says so; f32 -> bf16 is the CPU's ggml_compute_fp32_to_bf16 (round to nearest even, NaN -> (bits >> 16) | 0x40).  Each function is the device
 * counterpart of one ggml CPU op and follows its arithmetic (cited in csrc/ops_glue.hip):
 *   op_bin_bcast  GGML_OP_ADD/SUB/MUL/DIV   dst = a (op) b, b broadcast over a (ne_a % ne_b == 0), dst has a's shape
 *   op_unary      GGML_OP_UNARY             SILU, RELU, SIGMOID, TANH, NEG, ABS
 *   op_rms_norm   GGML_OP_RMS_NORM          per row: x / sqrt(mean(x^2) + eps), f32, rows contiguous
 *   op_cpy        GGML_OP_CPY/CONT/DUP      logical element order, any strides, among f32 / f16 / bf16
 *   op_soft_max   GGML_OP_SOFT_MAX          softmax(a*scale + slope*mask) per row; mask f32/f16 [ne00, >= ne01] or NULL
 *   op_rope       GGML_OP_ROPE              normal (mode 0) and neox (mode 2) rotary embedding, YaRN parameters, optional
 *                                           frequency factors (src2); pos = i32 device [ne2]
 *   op_mul_mat_f  GGML_OP_MUL_MAT           with an f16, bf16 or f32 src0 (attention KQ / KQV): dst[m,n] = sum_k a[k,m] b[k,n],
 *                                           dims 2/3 of src0 broadcast; an f16 / bf16 src0 rounds src1 to f16 / bf16 as the CPU does
 *                                           src0 may also be a view of a quantized KV cache (MI355Q_TYPE_Q8_0 / _Q4_0 / _Q4_1 / _Q5_0 / _Q5_1 /
 *                                           _IQ4_NL, nb[0] = block bytes, rows of <= 256 elements in whole blocks): src1 rows are
 *                                           quantized to the type's vec_dot_type and each output is the type's vec_dot, as on the CPU
 *   op_get_rows   GGML_OP_GET_ROWS          f32 / f16 / bf16 rows -> f32                                                          */
#define MI355Q_T_F32 0
#define MI355Q_T_F16 1
#define MI355Q_T_BF16 30
typedef struct mi355q_tensor {
    void   *data;
    int     type;
    int64_t ne[4];
    int64_t nb[4];
} mi355q_tensor;
#define MI355Q_OP_ADD 1
#define MI355Q_OP_SUB 2
#define MI355Q_OP_MUL 3
#define MI355Q_OP_DIV 4
#define MI355Q_UNARY_SILU    1
#define MI355Q_UNARY_RELU    2
#define MI355Q_UNARY_SIGMOID 3
#define MI355Q_UNARY_TANH    4
#define MI355Q_UNARY_NEG     5
#define MI355Q_UNARY_ABS     6
int mi355q_op_bin_bcast(int op, const mi355q_tensor *a, const mi355q_tensor *b, const mi355q_tensor *dst, void *stream);
int mi355q_op_unary(int uop, const mi355q_tensor *a, const mi355q_tensor *dst, void *stream);
int mi355q_op_rms_norm(const mi355q_tensor *a, const mi355q_tensor *dst, float eps, void *stream);
/* Fusions around the path (the reference's graph emits them as separate nodes: build_norm = RMS_NORM then MUL,
 * src/llama-graph.cpp; build_ffn LLM_FFN_SILU + LLM_FFN_PAR = UNARY then MUL).  Same f32 operations in the same order as the
 * separate ops, so results are bit-identical to issuing the nodes one by one.
 *   add_rms_norm_mul: x = b ? a + b : a;  if (sum) *sum = x;  dst = rms_norm(x, eps) [* weight[ne0]]     (b, sum, weight may be NULL)
 *   unary_mul:        dst = unary(a) * b          (SiLU / ReLU / sigmoid; contiguous f32 tensors of one shape)                  */
int mi355q_op_add_rms_norm_mul(const mi355q_tensor *a, const mi355q_tensor *b, const mi355q_tensor *sum, const float *weight,
                               const mi355q_tensor *dst, float eps, void *stream);
int mi355q_op_unary_mul(int uop, const mi355q_tensor *a, const mi355q_tensor *b, const mi355q_tensor *dst, void *stream);
/* GGML_OP_FLASH_ATTN_EXT (ggml.c ggml_flash_attn_ext; CPU ggml-cpu/ops.cpp:6690-6905) for an f16 KV cache:
 *   q f32 [DK, N, H, B], k f16 [DK, n_kv, Hk, Bk], v f16 [DV, n_kv, Hv, Bv] (NOT transposed), mask f16 [>= n_kv, >= N] or NULL,
 *   dst f32 [DV, H, N, B];  dst = softmax(softcap(scale k.q) + slope_h mask) v,  head sizes <= 256; n_kv <= 36864 on every path but the fused one.
 * k / v may instead both be bf16 (MI355Q_T_BF16; n_kv <= 8192 on the row kernel -- beyond: MI355Q_FA_KV_DIRECT below): q is rounded to bf16 and the scores are ggml_vec_dot_bf16 as on the CPU; with
 * >= 16 query rows and the workspace the matrix-core path rounds P to bf16.  Mixed k / v types need MI355Q_FA_KV_MIXED (below).
 * k / v may also both hold blocks of one quantized cache type (MI355Q_TYPE_Q8_0, _Q4_0, _Q4_1, _Q5_0, _Q5_1, _IQ4_NL; nb[0] = the block's bytes,
 * head sizes of whole 32-blocks, n_kv <= 8192 -- beyond: MI355Q_FA_KV_DIRECT below): the CPU's arithmetic for that type; with >= 16 query rows and the
 * workspace the cache is decoded once into f16 scratch for the matrix-core path.  mi355q_op_cpy / _indirect store f32 into such a cache
 * (contiguous destination, source rows of whole 32-blocks) with the bytes of the CPU's from_float of the type.
 * workspace (optional, mi355q_op_flash_attn_ext_workspace bytes): with it, a call with few query rows (decode) splits the KV range over
 * several workgroups per row and merges the pieces in a second launch, and a call with >= 16 query rows (prefill) computes scores,
 * softmax and P V on the matrix-core kernels with the scores of the batch in the workspace; without it every row is one workgroup --
 * unless the fused kernel takes the call.
 * The fused kernel (k_flash_attn_mfma) needs no workspace: one launch, scores never leave the registers, any window length.
 * It takes an f16 cache (or the f16 copy of a quantized one) with DK % 16 == 0, DV % 16 == 0 and data / nb[1..3] of q, k, v multiples of 16
 * bytes; any mask row stride.  Which calls go to it is decided by MI355Q_FA_FUSED, read on every call:
 *   0            never: the behaviour of a library without the kernel, MI355Q_ERR_UNSUPPORTED above 36864 positions included;
 *   1            every call it can take with >= 16 query rows, or with n_kv > 36864;
 *   unset, auto  with >= 16 query rows where neither the three-step matrix-core path nor the CPU-exact row kernel (n_kv <= 1024, DK % 32 == 0)
 *                applies (soft-cap, no or too small a workspace, n_kv % 16 != 0, a wide mask stride), or where the three-step path's scores
 *                N * n_kv * H * B * 4 exceed 256 MiB (the Infinity Cache); and every call with n_kv > 36864, decode included.
 * mi355q_op_flash_attn_ext_path answers which kernels a call would take (one of MI355Q_FA_PATH_*, or a negative MI355Q_ERR_* with the message
 * set) from types, shapes, strides and pointer alignment alone: it makes no device call, and mi355q_op_flash_attn_ext decides by calling it.
 * It was added without a change of MI355Q_API_VERSION: a caller that may meet an older library probes the symbol.                         */
#define MI355Q_FA_PATH_ROW_SEQ    0   /* one workgroup per query row, the CPU's sequential F16 accumulation (bit-exact)         */
#define MI355Q_FA_PATH_ROW_F32    1   /* one workgroup per query row, f32 two-pass                                              */
#define MI355Q_FA_PATH_ROW_SPLIT  2   /* few rows: the KV range split over several workgroups per row, merged by a second launch */
#define MI355Q_FA_PATH_KV_ROW     3   /* a quantized or bf16 cache, one workgroup per row with the CPU's arithmetic             */
#define MI355Q_FA_PATH_MFMA3      4   /* K q -> soft_max -> P V on the matrix-core matmul, scores in the workspace              */
#define MI355Q_FA_PATH_FUSED      5   /* k_flash_attn_mfma                                                                      */
#define MI355Q_FA_PATH_FUSED_KV   6   /* k_flash_attn_mfma on the cache's own blocks / bf16 rows, no f16 copy (only from ..._path2) */
int mi355q_op_flash_attn_ext_path(const mi355q_tensor *q, const mi355q_tensor *k, const mi355q_tensor *v, const mi355q_tensor *mask,
                                  const mi355q_tensor *dst, float logit_softcap, int has_workspace, size_t workspace_bytes);
size_t mi355q_op_flash_attn_ext_workspace(int64_t dv, int64_t n_q, int64_t n_head, int64_t n_batch, int64_t n_kv);
int mi355q_op_flash_attn_ext(const mi355q_tensor *q, const mi355q_tensor *k, const mi355q_tensor *v, const mi355q_tensor *mask,
                             const mi355q_tensor *dst, float scale, float max_bias, float logit_softcap,
                             void *workspace, size_t workspace_bytes, void *stream);
/* The same two with flags (added without a change of MI355Q_API_VERSION: probe the symbols); the functions above are these with flags = 0.
 * MI355Q_FA_KV_DIRECT: the fused kernel may read a quantized or bf16 cache's own rows, decoding blocks on the way into LDS (bf16: both
 * products on the bf16 matrix-core instruction, q and P rounded to bf16, nothing passes through f16).  For a block type the output equals,
 * bit for bit, the fused kernel's on the f16 copy of the cache.  "Direct-eligible": k / v of one block type with DK % 32 == 0, DV % 32 == 0
 * and data / nb[1..3] of k and v even -- or both bf16 with DK % 16 == 0, DV % 16 == 0 and data / nb[1..3] multiples of 16 --, and q's data /
 * nb[1..3] multiples of 16.  The flag is ignored under MI355Q_FA_FUSED=0 and for calls that are not direct-eligible.  Unset / auto, a
 * direct-eligible call answers MI355Q_FA_PATH_FUSED_KV (d) with n_kv > 8192, for any number of query rows -- the window the row kernel
 * refuses; a bf16 prompt the three-step path can take goes there only when its scores exceed 256 MiB -- and (e) with >= 16 query rows where
 * it has neither the f16 copy nor the three-step path (soft-cap, no or too small a workspace; bf16 also n_kv % 16 != 0 or a wide mask
 * stride).  MI355Q_FA_FUSED=1: every direct-eligible call with >= 16 rows or n_kv > 8192.  An answer of FUSED_KV does not depend on the
 * workspace: a caller that gets it may pass none.  Rows at positions >= n_kv are never read; a masked position adds nothing as long as its
 * dequantized value is finite in f16 (bf16: finite).                                                                                    */
#define MI355Q_FA_KV_DIRECT       0x1
/* MI355Q_FA_KV_MIXED: k and v may differ in type (-ctk A -ctv B), each of f16, q8_0, q4_0, q4_1, q5_0, q5_1, iq4_nl; a pair with bf16 on one
 * side stays MI355Q_ERR_UNSUPPORTED.  Without the flag every call answers as before: a mixed pair is refused, by the entry points without flags too.  With it,
 * a same-type call answers what it answers without.  A library from before the flag ignores the bit and refuses the pair with MI355Q_ERR_UNSUPPORTED: that is
 * the probe (ask mi355q_op_flash_attn_ext_path2 once; nothing else changed, MI355Q_API_VERSION included).  DK % 32 == 0; DV % 32 == 0 under a block V; data and
 * nb[1..3] of a block side even.  The CPU's arithmetic is separable and so is this one: the scores follow K's type (q to its vec_dot_type, its vec_dot), the
 * accumulator V's (f16: the F16 accumulator; a block type: F32 over its to_float).  The answers for such a pair:
 *   >= 16 rows, no soft-cap, the workspace, DV % 32 == 0, an f16 side 16-byte aligned: each block side is decoded once into f16 scratch (an f16 side is read
 *                as it lies) and the answer is the f16 rule's for that copy (MFMA3, FUSED, or a row kernel);
 *   >= 16 rows otherwise: FUSED_KV where MI355Q_FA_KV_DIRECT is set too, MI355Q_FA_FUSED is not 0, the pair is built (f16 or q8_0 on at least one side,
 *                DK and DV in the same bucket <= 64 / <= 128 / <= 256) and q and an f16 side are 16-byte aligned -- bit for bit the f16 fused kernel on the f16
 *                copies; else KV_ROW up to 8192 positions; else MI355Q_ERR_UNSUPPORTED;
 *   < 16 rows:   KV_ROW up to 8192 positions, with the CPU's bits as for same-type caches; beyond, FUSED_KV under the same conditions, else
 *                MI355Q_ERR_UNSUPPORTED.
 * MI355Q_FA_FUSED=1 forces FUSED_KV where it is available with >= 16 rows or n_kv > 8192; MI355Q_FA_FUSED=0 never reaches the fused kernel.              */
#define MI355Q_FA_KV_MIXED        0x2
int mi355q_op_flash_attn_ext_path2(const mi355q_tensor *q, const mi355q_tensor *k, const mi355q_tensor *v, const mi355q_tensor *mask,
                                   const mi355q_tensor *dst, float logit_softcap, int has_workspace, size_t workspace_bytes, uint32_t flags);
int mi355q_op_flash_attn_ext2(const mi355q_tensor *q, const mi355q_tensor *k, const mi355q_tensor *v, const mi355q_tensor *mask,
                              const mi355q_tensor *dst, float scale, float max_bias, float logit_softcap,
                              void *workspace, size_t workspace_bytes, void *stream, uint32_t flags);
int mi355q_op_cpy(const mi355q_tensor *a, const mi355q_tensor *dst, void *stream);
int mi355q_op_soft_max(const mi355q_tensor *a, const mi355q_tensor *mask, const mi355q_tensor *dst, float scale, float max_bias, void *stream);
int mi355q_op_rope(const mi355q_tensor *a, const int32_t *pos, const float *freq_factors, const mi355q_tensor *dst,
                   const mi355q_rope_params *p, void *stream);
int mi355q_op_mul_mat_f(const mi355q_tensor *a, const mi355q_tensor *b, const mi355q_tensor *dst, void *stream);
/* Token generation over an UNQUANTIZED weight matrix: y[n][m] = w[m][:] . x[n][:], w an f16 (type 1) or bf16 (type 30) matrix of m rows of
 * k elements, x f32 with 1 <= n <= 8 rows, y f32; strides in bytes.  One streaming launch: 16-byte non-temporal loads, x rounded once per workgroup
 * into the weight's type.  The bits are the reference CPU backend's (AVX2 build): x rounded to f16 (nearest even) and ggml_vec_dot_f16, or x rounded by
 * ggml_compute_fp32_to_bf16 and ggml_vec_dot_bf16 -- for bf16 the same bits as mi355q_op_mul_mat_f.  Asynchronous, capturable, no workspace.
 * Scope: k % 32 == 0 (the tail the CPU adds in double stays with mi355q_op_mul_mat_f), w and w_stride_bytes multiples of 16 with w_stride_bytes >= 2 k,
 * x and x_stride_bytes multiples of 4 (x_stride_bytes >= 4 k where n > 1), y and y_stride_bytes multiples of 4 with y_stride_bytes >= 4 m, m >= 1.
 * Also refused, because measured slower than mi355q_op_mul_mat_f (profiles/fw_stream.md): n >= 4 with m < 8192 and m k >= 2^24.
 * Everything else: MI355Q_ERR_UNSUPPORTED, nothing launched.  These are not types of the quantized path: mi355q_type_supported(1 / 30) stays 0.
 * flags: MI355Q_FW_ROWS_* fixes the rows one wave carries (four lanes own a row: 16 fills the wave; fewer spread a short matrix over more CUs);
 * 0 = the library chooses the largest of 16 / 8 / 4 that still gives each of the 256 CUs a workgroup of MI355Q_FW_WAVES waves.  Every form gives the same bits.
 * mi355q_mul_mat_fw_path answers MI355Q_FW_PATH_STREAM or MI355Q_ERR_UNSUPPORTED (the message set) from the numbers alone: no device call, nothing
 * dereferenced; mi355q_mul_mat_fw decides by calling it.  Added without a change of MI355Q_API_VERSION: probe the symbols.                          */
#define MI355Q_FW_PATH_STREAM 0
#define MI355Q_FW_WAVES       4
#define MI355Q_FW_ROWS_AUTO   0x0
#define MI355Q_FW_ROWS_4      0x1
#define MI355Q_FW_ROWS_8      0x2
#define MI355Q_FW_ROWS_16     0x3
#define MI355Q_FW_ROWS_MASK   0x3
int mi355q_mul_mat_fw_path(int type, const void *w, int64_t w_stride_bytes, const float *x, int64_t x_stride_bytes, float *y, int64_t y_stride_bytes,
                           int64_t m, int64_t n, int64_t k, int flags);
int mi355q_mul_mat_fw(int type /* 1 = f16, 30 = bf16 */, const void *w, int64_t w_stride_bytes, const float *x, int64_t x_stride_bytes,
                      float *y, int64_t y_stride_bytes, int64_t m, int64_t n, int64_t k, int flags, void *stream);
/* GGML_OP_GET_ROWS: dst[:, i10, i11, i12] = a[:, ids[i10, i11, i12], i11, i12]; a f32/f16, ids i32 (tensor with type field ignored), dst f32.
 * GGML_OP_SCALE:    dst = a * scale (f32). */
/* op_cpy whose destination base pointer is read ON THE DEVICE from dest_table[index] (dst->data is ignored): lets a captured
 * launch graph be replayed while the KV-cache store position moves every token (cf. ggml-cuda.cu cpy_dest_ptrs). */
int mi355q_op_cpy_indirect(const mi355q_tensor *a, const mi355q_tensor *dst, void *const *dest_table, int index, void *stream);
int mi355q_op_get_rows(const mi355q_tensor *a, const mi355q_tensor *ids, const mi355q_tensor *dst, void *stream);
/* The MoE router ops of build_moe_ffn (src/llama-graph.cpp:824-965): GGML_OP_ARGSORT (ggml_top_k = argsort descending + a view of the first k):
 * dst i32, same shape as a (f32), dst[row][r] = index of the element of rank r of the row (ties keep index order; ggml-cuda/argsort.cu:11, CPU
 * ops.cpp ggml_compute_forward_argsort_f32); GGML_OP_SUM_ROWS: dst[0, i1, i2, i3] = sum_i0 a[i0, i1, i2, i3], accumulated in f64 as the CPU does. */
int mi355q_op_argsort(const mi355q_tensor *a, const mi355q_tensor *dst, int descending, void *stream);
int mi355q_op_sum_rows(const mi355q_tensor *a, const mi355q_tensor *dst, void *stream);
int mi355q_op_scale(const mi355q_tensor *a, const mi355q_tensor *dst, float scale, void *stream);

/* ---- launch graphs: capture everything enqueued on `stream` between begin and end, replay it with one call ---------------
 * (hipStreamBeginCapture / hipStreamEndCapture / hipGraphInstantiate / hipGraphLaunch; the reference's counterpart is the CUDA
 * graph path of ggml-cuda.cu:2470-2781).  No allocation or synchronization may happen between begin and end.             */
typedef struct mi355q_graph mi355q_graph;
int mi355q_graph_capture_begin(void *stream);
int mi355q_graph_capture_end(void *stream, mi355q_graph **out);     /* on failure the stream leaves capture mode, *out = NULL */
int mi355q_graph_launch(mi355q_graph *graph, void *stream);
int mi355q_graph_destroy(mi355q_graph *graph);

#ifdef __cplusplus
}
#endif
#endif /* MI355Q_H */
