// TEST INFRASTRUCTURE (tests/test_noise_isa.py): explicit instantiations of the lift kernels at the moduli counts of the
// stock parameter sets (3, 5, 9), of C2 (4) and of C5's chain (16), with and without the limb output, so that their device assembly can be
// produced in seconds and checked for scratch (spills) and for the kinds of scalar instructions used.
#include "kernels.hpp"
namespace fhe {
namespace k {
#define FHE_PROBE_L(L)                                                                                                  \
    template __global__ void lift_kernel<L, false>(const u64 *, const u64 *, LiftSub, u64 *, uint32_t *, uint32_t,     \
                                                   uint32_t, uint32_t, uint32_t, uint32_t);                           \
    template __global__ void lift_kernel<L, true>(const u64 *, const u64 *, LiftSub, u64 *, uint32_t *, uint32_t,      \
                                                  uint32_t, uint32_t, uint32_t, uint32_t);
FHE_PROBE_L(3)
FHE_PROBE_L(4)
FHE_PROBE_L(5)
FHE_PROBE_L(9)
FHE_PROBE_L(16)
}  // namespace k
}  // namespace fhe
