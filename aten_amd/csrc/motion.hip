// Geometry motion vectors (device/motion.hpp) as a translation unit of its own, and the launchers aten_amd.hip calls (declared in
// device/launch.hpp): the ids capture behind the bounce-0 trace, the motion pass, and the range copies that bring the geometry history
// up to date.
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_MOTION_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/motion.hpp"

namespace atn {

void motion_launch_capture(uint32_t grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, float4* ids)
{
    hipLaunchKernelGGL(k_motion_capture_ids, dim3(grid), dim3(256), 0, st, pb, fp, ids);
}

void motion_launch_geometry(const TileLaunch& l, hipStream_t st, const MotionArgs& a)
{
    hipLaunchKernelGGL(k_motion_geometry, dim3(l.grid_x, l.grid_y), dim3(256), 0, st, a);
}

void motion_launch_copy(hipStream_t st, float4* dst, const float4* src, uint32_t n_quads)
{
    if (n_quads) hipLaunchKernelGGL(k_motion_copy, dim3((n_quads + 255u) / 256u), dim3(256), 0, st, dst, src, n_quads);
}

} // namespace atn
