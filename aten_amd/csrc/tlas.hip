// The top layer built on the device (device/tlas.hpp, docs/TLAS.md) as a translation unit of its own, and the launchers
// aten_amd.hip calls (declared in device/launch.hpp).  The general path's sort and hierarchy are lbvh.hpp's kernels, which belong
// to aten_amd.hip: PathTracing::tlas_rebuild launches them between tlas_launch_codes and tlas_launch_emit.
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_LBVH_HELPERS_ONLY 1
#define ATN_TLAS_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/tlas.hpp"

namespace atn {

void tlas_launch_block(const TlasLaunch& l, hipStream_t st, const TlasArgs& a)
{
    hipLaunchKernelGGL(k_tlas_block, dim3(1), dim3(l.block), 0, st, a);
}

void tlas_launch_codes(const TlasLaunch& l, hipStream_t st, const TlasArgs& a)
{
    hipLaunchKernelGGL(k_tlas_leaf_boxes, dim3(l.leaf_grid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_tlas_union, dim3(1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_tlas_codes, dim3(l.leaf_grid), dim3(256), 0, st, a);
}

void tlas_launch_emit(const TlasLaunch& l, hipStream_t st, const TlasArgs& a)
{
    hipLaunchKernelGGL(k_tlas_bounds, dim3(l.leaf_grid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_tlas_emit, dim3(l.node_grid), dim3(256), 0, st, a);
}

} // namespace atn
