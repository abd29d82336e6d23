// Ambient occlusion (device/ao.hpp) as a translation unit of its own, and the launchers aten_amd.hip calls (declared in
// device/launch.hpp).  The primary rays and the AO rays ride the renderer's own walk (trace_dispatch with jobs of their own).
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_AO_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/ao.hpp"

namespace atn {

void ao_launch_primary(const TraceLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const AoArgs& aa)
{
    if (l.lds) hipLaunchKernelGGL((k_ao_primary<true>), dim3(l.grid), dim3(l.block), l.lds_bytes, st, pb, sc, aa);
    else hipLaunchKernelGGL((k_ao_primary<false>), dim3(l.grid), dim3(l.block), 0, st, pb, sc, aa);
}

void ao_launch_rays(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const AoArgs& aa)
{
    hipLaunchKernelGGL(k_ao_shade, dim3(l.grid), dim3(256), 0, st, pb, sc, fp, aa);
    // (the refill walk over an LDS copy -- only ever forced on a small scene -- walks global memory here, as the NPR sample rays do)
    if (l.refill) hipLaunchKernelGGL((k_ao_trace<true, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, sc, aa);
    else if (l.lds_bytes) hipLaunchKernelGGL((k_ao_trace<false, true>), dim3(l.trace_grid), dim3(l.trace_block), l.lds_bytes, st, sc, aa);
    else hipLaunchKernelGGL((k_ao_trace<false, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, sc, aa);
}

void ao_launch_resolve(const RayLaunch& l, hipStream_t st, const FrameParams& fp, const AoArgs& aa, float4* film, float4* tile_out)
{
    hipLaunchKernelGGL(k_ao_resolve, dim3(l.slot_grid), dim3(256), 0, st, fp, aa, film, tile_out);
    if (aa.filter) hipLaunchKernelGGL(k_ao_bilateral, dim3(l.slot_grid), dim3(256), 0, st, fp, aa, film, tile_out);
}

} // namespace atn
