// fattn_mfma_mxa.hip -- k_flash_attn_mfma (fattn_mfma.cuh) on a mixed cache's own rows, an f16 K with a V of any block type: a translation unit of its own for the build's sake.
#include "fattn_mfma.cuh"

namespace mi355q {

hipError_t fam_launch_mxa(int vtype, const FamArgs & a, dim3 grid, size_t lds, hipStream_t st) {
    return fam_launch_mix_side<1, true, true>(vtype, a, grid, lds, st);
}

} // namespace mi355q
