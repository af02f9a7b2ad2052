// TEST INFRASTRUCTURE (tests/test_mbfv_isa.py): explicit instantiations of the multiparty share kernel at the whole-row
// tile sizes of the stock parameter sets (4096 ... 16384 points), integer (narrow / general passes) and F64, in each of
// its three forms, so that their device assembly can be produced in seconds and checked for scratch (spills).
#include "kernels.hpp"
namespace fhe {
namespace k {
#define FHE_PROBE_M(LOGM, NRW, HR, FORM) \
    template __global__ void mbfv_share_kernel<LOGM, NRW, HR, FORM>(MbfvArgs, u64 *, const DevMod *, const u64x2 *);
#define FHE_PROBE_F(LOGM, NRW, HR) \
    FHE_PROBE_M(LOGM, NRW, HR, MBFV_AX) FHE_PROBE_M(LOGM, NRW, HR, MBFV_AXX) FHE_PROBE_M(LOGM, NRW, HR, MBFV_AX_WY)
#define FHE_PROBE_LM(LOGM) FHE_PROBE_F(LOGM, true, 0) FHE_PROBE_F(LOGM, false, 0) FHE_PROBE_F(LOGM, false, 3) \
    FHE_PROBE_F(LOGM, false, 4) FHE_PROBE_F(LOGM, false, 5)
FHE_PROBE_LM(12)
FHE_PROBE_LM(13)
FHE_PROBE_LM(14)
}  // namespace k
}  // namespace fhe
