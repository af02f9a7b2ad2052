// TEST INFRASTRUCTURE (tests/test_transcode_isa.py): explicit instantiations of the bit-stream encoder at the whole-row
// tile sizes of the stock parameter sets (4096 ... 16384 points), integer (narrow / general passes) and F64, so that their
// device assembly can be produced in seconds and checked for scratch (spills).  transcode_ew_kernel is no template: it is
// in the assembly as soon as the header is included.
#include "kernels.hpp"
namespace fhe {
namespace k {
#define FHE_PROBE_K(LOGM, NRW, HR)                                                                                      \
    template __global__ void encode_stream_kernel<LOGM, NRW, HR>(StreamSrc, u64 *, uint32_t, const DevMod *, const u64x2 *);
#define FHE_PROBE_LM(LOGM) FHE_PROBE_K(LOGM, true, 0) FHE_PROBE_K(LOGM, false, 0) FHE_PROBE_K(LOGM, false, 3) \
    FHE_PROBE_K(LOGM, false, 4) FHE_PROBE_K(LOGM, false, 5)
FHE_PROBE_LM(12)
FHE_PROBE_LM(13)
FHE_PROBE_LM(14)
}  // namespace k
}  // namespace fhe
