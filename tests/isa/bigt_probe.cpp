// TEST INFRASTRUCTURE (tests/test_bigt_isa.py): explicit instantiations of the kernels for plaintext moduli above 64
// bits -- the tail at the (P, W_t) of the five parameter sets of tests/bigt_ref.py and the projection at W_t = 2, 3, 4 --
// so that their device assembly can be produced in seconds and checked for scratch (spills).
#include "kernels.hpp"
namespace fhe {
namespace k {
#define FHE_PROBE_TAIL(P, WT)                                                                                          \
    template __global__ void bigt_tail_kernel<P, WT>(const u64 *, const u64 *, BigT<WT>, u64 *, uint32_t, uint32_t, uint32_t);
#define FHE_PROBE_PROJECT(WT)                                                                                          \
    template __global__ void bigt_project_kernel<WT>(const u64 *, u64, u64 *, uint32_t, const DevMod *, const u64x2 *,  \
                                                     BigT<WT>, BigVal<WT>, uint32_t, uint32_t, u64);
FHE_PROBE_TAIL(4, 2)
FHE_PROBE_TAIL(4, 3)
FHE_PROBE_TAIL(3, 2)
FHE_PROBE_TAIL(6, 4)
FHE_PROBE_TAIL(6, 2)
FHE_PROBE_PROJECT(2)
FHE_PROBE_PROJECT(3)
FHE_PROBE_PROJECT(4)
}  // namespace k
}  // namespace fhe
