// TEST INFRASTRUCTURE (tests/test_hoistkeyed_isa.py): the two stage B kernels of the hoisted calls with one Galois key set
// per client (kernels_kshoistkeyed.hpp) next to their single-client siblings (kernels_kshoist.hpp), referenced so that
// their device assembly can be produced in seconds, checked for scratch (spills) and compared in registers.
#include "kernels.hpp"
namespace fhe {
namespace k {
__device__ const void *hoistkeyed_probe_kernels[] = {reinterpret_cast<const void *>(&hoist_mac_keyed_kernel),
                                                     reinterpret_cast<const void *>(&hoist_matvec_keyed_kernel),
                                                     reinterpret_cast<const void *>(&hoist_mac_kernel),
                                                     reinterpret_cast<const void *>(&hoist_matvec_kernel)};
}  // namespace k
}  // namespace fhe
