// The NPR shadow pre-pass (device/npr_shadow.hpp) as a translation unit of its own, and the launchers aten_amd.hip calls (declared in
// device/launch.hpp).  The primary rays and the shadow rays ride the renderer's own walk (trace_dispatch with jobs of their own).
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_NPR_SHADOW_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/npr_shadow.hpp"

namespace atn {

void ns_launch_primary(const TraceLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const NsArgs& na)
{
    if (l.lds) hipLaunchKernelGGL((k_ns_primary<true>), dim3(l.grid), dim3(l.block), l.lds_bytes, st, pb, sc, na);
    else hipLaunchKernelGGL((k_ns_primary<false>), dim3(l.grid), dim3(l.block), 0, st, pb, sc, na);
}

void ns_launch_rays(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const NsArgs& na)
{
    hipLaunchKernelGGL(k_ns_shade, dim3(l.grid), dim3(256), 0, st, pb, sc, fp, na);
    // (the refill walk over an LDS copy -- only ever forced on a small scene -- walks global memory here, as the AO rays do)
    if (l.refill) hipLaunchKernelGGL((k_ns_trace<true, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, pb, sc, fp, na);
    else if (l.lds_bytes) hipLaunchKernelGGL((k_ns_trace<false, true>), dim3(l.trace_grid), dim3(l.trace_block), l.lds_bytes, st, pb, sc, fp, na);
    else hipLaunchKernelGGL((k_ns_trace<false, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, pb, sc, fp, na);
}

void ns_launch_filter(hipStream_t st, const float* lit, const float* depth, float* out, int32_t width, int32_t height)
{
    hipLaunchKernelGGL(k_ns_filter, dim3(((uint32_t)width + 255u) / 256u, (uint32_t)height), dim3(256), 0, st, lit, depth, out, width, height);
}

} // namespace atn
