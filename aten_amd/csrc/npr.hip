// NPR feature lines (device/npr.hpp) as a translation unit of their own, and the launchers aten_amd.hip calls (declared in
// device/launch.hpp).  The sample rays ride the renderer's own walk (trace_dispatch with a job over the ray list).
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_NPR_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/npr.hpp"

namespace atn {

void npr_launch_gen(uint32_t grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, const NprArgs& na)
{
    hipLaunchKernelGGL(k_npr_gen, dim3(grid), dim3(256), 0, st, pb, fp, na);
}

void npr_launch_bounce(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                       const atn_camera_param& cam, const NprArgs& na, int32_t bounce)
{
    hipLaunchKernelGGL(k_npr_prep, dim3(l.grid), dim3(256), 0, st, pb, sc, na, bounce);
    // (the refill walk over an LDS copy -- only ever forced, ATEN_AMD_TRACE=1 on a small scene -- walks global memory here: that
    // instantiation of the walk needs scratch)
    if (l.refill) hipLaunchKernelGGL((k_npr_trace<true, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, sc, na, bounce);
    else if (l.lds_bytes) hipLaunchKernelGGL((k_npr_trace<false, true>), dim3(l.trace_grid), dim3(l.trace_block), l.lds_bytes, st, sc, na, bounce);
    else hipLaunchKernelGGL((k_npr_trace<false, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, sc, na, bounce);
    hipLaunchKernelGGL(k_npr_eval, dim3(l.grid), dim3(256), 0, st, pb, sc, fp, cam, na, bounce);
    hipLaunchKernelGGL(k_npr_commit, dim3(1), dim3(64), 0, st, pb, na, bounce);
}

void npr_launch_capture0(uint32_t grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, const NprArgs& na)
{
    hipLaunchKernelGGL(k_npr_capture0, dim3(grid), dim3(256), 0, st, pb, fp, na);
}

} // namespace atn
