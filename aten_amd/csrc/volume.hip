// Path tracing through homogeneous media (device/volume.hpp) as a translation unit of its own, and the launchers aten_amd.hip calls
// (declared in device/launch.hpp).  The closest-hit rays and the connections ride the renderer's own walk (trace_dispatch).
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_VOLUME_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/volume.hpp"

namespace atn {

void vol_launch_begin(const RayLaunch& l, hipStream_t st, const FrameParams& fp, const VolArgs& va)
{
    hipLaunchKernelGGL(k_vol_begin, dim3(l.slot_grid), dim3(256), 0, st, fp, va);
}

// (the refill walk over an LDS copy is never planned: PassPlan picks the LDS copy for small trees, the refill walk for deep ones)
void vol_launch_closest(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const VolArgs& va, int32_t it)
{
    if (l.refill) hipLaunchKernelGGL((k_vol_closest<true, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, pb, sc, va, it);
    else if (l.lds_bytes) hipLaunchKernelGGL((k_vol_closest<false, true>), dim3(l.trace_grid), dim3(l.trace_block), l.lds_bytes, st, pb, sc, va, it);
    else hipLaunchKernelGGL((k_vol_closest<false, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, pb, sc, va, it);
}

void vol_launch_shade(int material_set, const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                      const atn_camera_param& cam, const VolArgs& va, int32_t it)
{
    const dim3 g(l.grid), t(256);
    switch (material_set) {
    case kMsCore: hipLaunchKernelGGL((k_vol_shade<kMsCore>), g, t, 0, st, pb, sc, fp, cam, va, it); break;
    case kMsDisney: hipLaunchKernelGGL((k_vol_shade<kMsDisney>), g, t, 0, st, pb, sc, fp, cam, va, it); break;
    default: hipLaunchKernelGGL((k_vol_shade<kMsAnalytic>), g, t, 0, st, pb, sc, fp, cam, va, it); break;
    }
}

void vol_launch_transmit(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const VolArgs& va, int32_t it)
{
    if (l.refill) hipLaunchKernelGGL((k_vol_transmit<true, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, pb, sc, va, it);
    else if (l.lds_bytes) hipLaunchKernelGGL((k_vol_transmit<false, true>), dim3(l.trace_grid), dim3(l.trace_block), l.lds_bytes, st, pb, sc, va, it);
    else hipLaunchKernelGGL((k_vol_transmit<false, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, pb, sc, va, it);
}

void vol_launch_reduce(const RayLaunch& l, hipStream_t st, const FrameParams& fp, const VolArgs& va)
{
    hipLaunchKernelGGL(k_vol_reduce, dim3(l.slot_grid < 1024u ? l.slot_grid : 1024u), dim3(256), 0, st, fp, va);
}

void vol_launch_phase_table(hipStream_t st, float g, uint32_t n, const float* w, const float* r1, const float* r2, const float* wo, float* out_dir, float* out_eval)
{
    hipLaunchKernelGGL(k_vol_phase_table, dim3((n + 255u) / 256u), dim3(256), 0, st, g, n, w, r1, r2, wo, out_dir, out_eval);
}

} // namespace atn
