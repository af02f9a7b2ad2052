// TEST INFRASTRUCTURE (tests/test_encrypt_isa.py): explicit instantiations of the encryption kernels at the whole-row
// tile sizes of the stock parameter sets (4096 ... 16384 points), integer (narrow / general passes) and F64, so that their
// device assembly can be produced in seconds and checked for scratch (spills).
#include "kernels.hpp"
namespace fhe {
namespace k {
#define FHE_PROBE_E(LOGM, NRW, HR)                                                                                     \
    template __global__ void small_ntt_kernel<LOGM, NRW, HR>(const int8_t *, u64 *, uint32_t, const DevMod *,           \
                                                             const u64x2 *);                                          \
    template __global__ void encrypt_sk_kernel<LOGM, NRW, HR>(const int8_t *, const u64 *, const u64 *, const u64 *, u64, \
                                                              u64 *, uint32_t, const DevMod *, const u64x2 *);        \
    template __global__ void encrypt_pk_kernel<LOGM, NRW, HR>(const int8_t *, const u64 *, const u64 *, u64, u64 *,     \
                                                              uint32_t, const DevMod *, const u64x2 *, uint32_t);
#define FHE_PROBE_LM(LOGM) FHE_PROBE_E(LOGM, true, 0) FHE_PROBE_E(LOGM, false, 0) FHE_PROBE_E(LOGM, false, 3) \
    FHE_PROBE_E(LOGM, false, 4) FHE_PROBE_E(LOGM, false, 5)
FHE_PROBE_LM(12)
FHE_PROBE_LM(13)
FHE_PROBE_LM(14)
}  // namespace k
}  // namespace fhe
