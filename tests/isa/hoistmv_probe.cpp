// TEST INFRASTRUCTURE (tests/test_hoistmv_isa.py): the fused stage B of the hoisted matrix-vector product
// (kernels_kshoist.hpp) and the kernel that adds its partial sums, referenced so that their device assembly can be produced
// in seconds and checked for scratch (spills).
#include "kernels.hpp"
namespace fhe {
namespace k {
__device__ const void *hoistmv_probe_kernels[] = {reinterpret_cast<const void *>(&hoist_matvec_kernel),
                                                  reinterpret_cast<const void *>(&mbfv_sum_kernel)};
}  // namespace k
}  // namespace fhe
