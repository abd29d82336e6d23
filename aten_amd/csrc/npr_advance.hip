// The NPR look-through (device/npr_advance.hpp) as a translation unit of its own, and the launchers aten_amd.hip calls (declared in
// device/launch.hpp): the look-through's walk, and the shade launches' alpha-blend flavour for the material sets an NPR frame can hold
// (CarPaint is refused).
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_NPR_ADVANCE_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/npr_advance.hpp"

namespace atn {

void npr_adv_launch_init(uint32_t slot_grid, hipStream_t st, const FrameParams& fp, const NprAdvArgs& aa)
{
    hipLaunchKernelGGL(k_npr_adv_init, dim3(slot_grid), dim3(256), 0, st, fp, aa);
}

void npr_adv_launch_bounce(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const NprAdvArgs& aa, int32_t bounce)
{
    // (the refill walk over an LDS copy walks global memory here, as k_npr_trace's does)
    if (l.refill) hipLaunchKernelGGL((k_npr_advance<true, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, pb, sc, aa, bounce);
    else if (l.lds_bytes) hipLaunchKernelGGL((k_npr_advance<false, true>), dim3(l.trace_grid), dim3(l.trace_block), l.lds_bytes, st, pb, sc, aa, bounce);
    else hipLaunchKernelGGL((k_npr_advance<false, false>), dim3(l.trace_grid), dim3(l.trace_block), 0, st, pb, sc, aa, bounce);
    hipLaunchKernelGGL(k_npr_adv_commit, dim3(1), dim3(64), 0, st, pb, aa, bounce);
}

void npr_adv_launch_capture0(uint32_t slot_grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, const NprAdvArgs& aa)
{
    hipLaunchKernelGGL(k_npr_adv_capture0, dim3(slot_grid), dim3(256), 0, st, pb, fp, aa);
}

int npr_adv_launch_shade(int material_set, int waves, uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                         const atn_camera_param& cam, int32_t bounce, const float4* ab)
{
    if (material_set == kMsCarPaint) return -1;     // (refused in front of the frame: no such instantiation)
    with_shade_flavour(material_set, waves, [&](auto k) {
        using K = decltype(k);
        if constexpr (K::ms == kMsCarPaint) return;
        else if constexpr (K::waves == 0) hipLaunchKernelGGL((k_shade_ab<K::ms>), dim3(grid), dim3(256), 0, st, pb, sc, fp, cam, bounce, ab);
        else hipLaunchKernelGGL((k_shade_ab_wn<K::ms, K::waves>), dim3(grid), dim3(256), 0, st, pb, sc, fp, cam, bounce, ab);
    });
    return 0;
}

} // namespace atn
