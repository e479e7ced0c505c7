// fattn_mfma.hip -- the launcher of k_flash_attn_mfma (fattn_mfma.cuh) and its f16 instantiations.
#include "fattn_mfma.cuh"

namespace mi355q {

// The launcher ops_glue.hip calls once mi355q_op_flash_attn_ext_path2 has answered MI355Q_FA_PATH_FUSED (f16 k / v) or MI355Q_FA_PATH_FUSED_KV (k / v of
// one block type, or bf16, or a mixed pair of fam_mix_built: the kernel reads the cache's own rows): shapes, types and alignment are checked there.
// scale is the one applied to the raw dot product (already divided by the soft-cap).
__attribute__((visibility("hidden")))
bool fattn_mfma_mix_built(int k_type, int v_type, int64_t DK, int64_t DV) { return fam_mix_built(k_type, v_type, DK, DV); }

__attribute__((visibility("hidden")))
int fattn_mfma_launch(const mi355q_tensor * q, const mi355q_tensor * k, const mi355q_tensor * v, const mi355q_tensor * mask, const mi355q_tensor * dst,
                      float scale, float max_bias, float softcap, float m0, float m1, uint32_t n_head_log2, void * stream) {
    FamArgs a;
    a.q = (const char *) q->data; a.k = (const char *) k->data; a.v = (const char *) v->data; a.m = mask ? (const char *) mask->data : nullptr; a.d = (char *) dst->data;
    for (int i = 0; i < 4; ++i) { a.q_nb[i] = q->nb[i]; a.k_nb[i] = k->nb[i]; a.v_nb[i] = v->nb[i]; a.d_nb[i] = dst->nb[i]; }
    a.m_nb1 = mask ? mask->nb[1] : 0;
    a.N = q->ne[1]; a.n_kv = k->ne[1]; a.DK = (int) k->ne[0]; a.DV = (int) v->ne[0];
    a.gqa_k = (int) (q->ne[2] / k->ne[2]); a.gqa_v = (int) (q->ne[2] / v->ne[2]); a.bq_k = (int) (q->ne[3] / k->ne[3]); a.bq_v = (int) (q->ne[3] / v->ne[3]);
    const int64_t n_tiles = (a.n_kv + FAM_T - 1) / FAM_T, words = ((n_tiles + 31) / 32 + 3) & ~(int64_t) 3;      // whole 16 bytes: the tiles behind stay aligned
    a.map_words = mask ? (int) (words < FAM_MAP_WORDS ? words : FAM_MAP_WORDS) : 0;
    a.scale = scale; a.softcap = softcap; a.max_bias = max_bias; a.m0 = m0; a.m1 = m1; a.n_head_log2 = n_head_log2;
    auto al4 = [](const mi355q_tensor * t) { return ((((uintptr_t) t->data) | (uintptr_t) t->nb[1] | (uintptr_t) t->nb[2] | (uintptr_t) t->nb[3]) & 3) == 0 ? 1 : 0; };
    a.k_al4 = al4(k); a.v_al4 = al4(v);
    const int dk32 = (a.DK + 31) & ~31;
    const size_t lds = (size_t) 4 * a.map_words + (size_t) FAM_T * (2 * dk32 + 16) + (size_t) FAM_T * (2 * a.DV + 32);
    const int64_t gx = (a.N + FAM_T - 1) / FAM_T;
    if (gx > 0x7FFFFFFF) return MI355Q_ERR_UNSUPPORTED;
    const dim3 grid((unsigned) gx, (unsigned) q->ne[2], (unsigned) q->ne[3]);
    hipError_t e = hipSuccess;
    hipStream_t st = (hipStream_t) stream;
    if (k->type != v->type) {                                                  // a mixed cache (MI355Q_FA_KV_MIXED): the 22 built pairs, one bucket for both head sizes
        if (!fam_mix_built(k->type, v->type, a.DK, a.DV)) return MI355Q_ERR_UNSUPPORTED;
        if (k->type == 1) e = fam_launch_mxa(v->type, a, grid, lds, st);
        else if (k->type == MI355Q_TYPE_Q8_0) e = fam_launch_mxb(v->type, a, grid, lds, st);
        else if (v->type == 1) e = fam_launch_mxc(k->type, a, grid, lds, st);
        else e = fam_launch_mxd(k->type, a, grid, lds, st);
        return e == hipSuccess ? MI355Q_OK : MI355Q_ERR_HIP;
    }
    switch (k->type) {
        case 1: e = fam_launch_buckets<1>(a, grid, lds, st); break;
        case MI355Q_TYPE_Q8_0: case MI355Q_TYPE_Q4_0: case MI355Q_TYPE_Q4_1: case MI355Q_T_BF16: e = fam_launch_kva(k->type, a, grid, lds, st); break;
        case MI355Q_TYPE_Q5_0: case MI355Q_TYPE_Q5_1: case MI355Q_TYPE_IQ4_NL: e = fam_launch_kvb(k->type, a, grid, lds, st); break;
        default: return MI355Q_ERR_UNSUPPORTED;
    }
    return e == hipSuccess ? MI355Q_OK : MI355Q_ERR_HIP;
}

} // namespace mi355q
