// TEST INFRASTRUCTURE (tests/test_keyed_isa.py): the stage-B kernels of the unfused key switch -- the keyed one
// (kernels_kskeyed.hpp) next to the single-key one it restates -- referenced so that their device assembly can be produced
// in seconds and checked for scratch (spills).
#include "kernels.hpp"
namespace fhe {
namespace k {
__device__ const void *keyed_probe_kernels[] = {reinterpret_cast<const void *>(&ks_mac_keyed_kernel),
                                               reinterpret_cast<const void *>(&ks_mac_kernel)};
}  // namespace k
}  // namespace fhe
