// fattn_mfma_kva.hip -- k_flash_attn_mfma (fattn_mfma.cuh) on a Q8_0, Q4_0, Q4_1 or bf16 cache's own rows: a translation unit of its own for the build's sake.
#include "fattn_mfma.cuh"

namespace mi355q {

hipError_t fam_launch_kva(int type, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st) {
    switch (type) {
        case MI355Q_TYPE_Q8_0: return fam_launch_buckets<MI355Q_TYPE_Q8_0>(a, grid, lds, st);
        case MI355Q_TYPE_Q4_0: return fam_launch_buckets<MI355Q_TYPE_Q4_0>(a, grid, lds, st);
        case MI355Q_TYPE_Q4_1: return fam_launch_buckets<MI355Q_TYPE_Q4_1>(a, grid, lds, st);
        default:               return fam_launch_buckets<MI355Q_T_BF16>(a, grid, lds, st);
    }
}

} // namespace mi355q
