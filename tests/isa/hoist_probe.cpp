// TEST INFRASTRUCTURE (tests/test_hoist_isa.py): stage B of the hoisted rotations (kernels_kshoist.hpp), referenced so
// that its device assembly can be produced in seconds and checked for scratch (spills).
#include "kernels.hpp"
namespace fhe {
namespace k {
__device__ const void *hoist_probe_kernels[] = {reinterpret_cast<const void *>(&hoist_mac_kernel)};
}  // namespace k
}  // namespace fhe
