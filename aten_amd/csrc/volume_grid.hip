// Grid media (device/volume_grid.hpp) as a translation unit of its own: the GRID flavours of the volume renderer's shade kernel and
// connection walk, and the launchers aten_amd.hip calls (declared in device/launch.hpp).  volume.hip keeps the gridless kernels.
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_VOLUME_TU 1
#define ATN_VOLUME_GRID_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/volume_grid.hpp"

namespace atn {

void vol_launch_shade_grid(int material_set, const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                           const atn_camera_param& cam, const VolArgs& va, const VolGridArgs& vg, int32_t it)
{
    const dim3 g(l.grid), t(256);
    switch (material_set) {
    case kMsCore: hipLaunchKernelGGL((k_vol_shade_grid<kMsCore>), g, t, 0, st, pb, sc, fp, cam, va, vg, it); break;
    case kMsDisney: hipLaunchKernelGGL((k_vol_shade_grid<kMsDisney>), g, t, 0, st, pb, sc, fp, cam, va, vg, it); break;
    default: hipLaunchKernelGGL((k_vol_shade_grid<kMsAnalytic>), g, t, 0, st, pb, sc, fp, cam, va, vg, it); break;
    }
}

void vol_launch_transmit_grid(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const VolArgs& va, const VolGridArgs& vg, int32_t it)
{
    if (l.refill) hipLaunchKernelGGL((k_vol_transmit_grid<true, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, pb, sc, va, vg, it);
    else if (l.lds_bytes) hipLaunchKernelGGL((k_vol_transmit_grid<false, true>), dim3(l.trace_grid), dim3(l.trace_block), l.lds_bytes, st, pb, sc, va, vg, it);
    else hipLaunchKernelGGL((k_vol_transmit_grid<false, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, pb, sc, va, vg, it);
}

} // namespace atn
