// TEST INFRASTRUCTURE (tests/test_keyload_isa.py): explicit instantiations of the wire-load kernel at the whole-row tile
// sizes of the stock parameter sets (4096 ... 16384 points), integer (narrow / general passes) and F64, so that their
// device assembly can be produced in seconds and checked for scratch (spills).
#include "kernels.hpp"
namespace fhe {
namespace k {
#define FHE_PROBE_K(LOGM, NRW, HR)                                                                                      \
    template __global__ void ksk_load_kernel<LOGM, NRW, HR>(const uint8_t *, const uint8_t *, u64, uint32_t,            \
                                                            const u64x2 *, KskOutTable, uint32_t, uint32_t, uint32_t,   \
                                                            uint32_t, const DevMod *, const u64x2 *, uint32_t *);
#define FHE_PROBE_LM(LOGM) FHE_PROBE_K(LOGM, true, 0) FHE_PROBE_K(LOGM, false, 0) FHE_PROBE_K(LOGM, false, 3) \
    FHE_PROBE_K(LOGM, false, 4) FHE_PROBE_K(LOGM, false, 5)
FHE_PROBE_LM(12)
FHE_PROBE_LM(13)
FHE_PROBE_LM(14)
}  // namespace k
}  // namespace fhe
