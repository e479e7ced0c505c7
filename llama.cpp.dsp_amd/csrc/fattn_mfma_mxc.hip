// fattn_mfma_mxc.hip -- k_flash_attn_mfma (fattn_mfma.cuh) on a mixed cache's own rows, an f16 V with a K of Q4_0, Q4_1, Q5_0, Q5_1 or IQ4_NL: a translation unit of its own for the build's sake.
#include "fattn_mfma.cuh"

namespace mi355q {

hipError_t fam_launch_mxc(int ktype, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st) {
    return fam_launch_mix_side<1, false, false>(ktype, a, grid, lds, st);
}

} // namespace mi355q
