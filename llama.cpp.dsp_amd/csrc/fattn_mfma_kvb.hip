// fattn_mfma_kvb.hip -- k_flash_attn_mfma (fattn_mfma.cuh) on a Q5_0, Q5_1 or IQ4_NL cache's own rows: a translation unit of its own for the build's sake.
#include "fattn_mfma.cuh"

namespace mi355q {

hipError_t fam_launch_kvb(int type, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st) {
    switch (type) {
        case MI355Q_TYPE_Q5_0: return fam_launch_buckets<MI355Q_TYPE_Q5_0>(a, grid, lds, st);
        case MI355Q_TYPE_Q5_1: return fam_launch_buckets<MI355Q_TYPE_Q5_1>(a, grid, lds, st);
        default:               return fam_launch_buckets<MI355Q_TYPE_IQ4_NL>(a, grid, lds, st);
    }
}

} // namespace mi355q
