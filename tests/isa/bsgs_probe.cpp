// TEST INFRASTRUCTURE (tests/test_bsgs_isa.py): the two stage B kernels of the baby-step/giant-step hoisted matrix-vector
// product (kernels_bsgs.hpp), every shipped tile instance, referenced so that their device assembly can be produced in
// seconds and checked for scratch (spills).
#include "kernels.hpp"
namespace fhe {
namespace k {
__device__ const void *bsgs_probe_kernels[] = {reinterpret_cast<const void *>(&bsgs_baby_kernel<1>),
                                               reinterpret_cast<const void *>(&bsgs_baby_kernel<2>),
                                               reinterpret_cast<const void *>(&bsgs_baby_kernel<4>),
                                               reinterpret_cast<const void *>(&bsgs_giant_kernel)};
}  // namespace k
}  // namespace fhe
