// NPR hatching shadows (device/npr_hatching.hpp) as a translation unit of its own, and the launchers aten_amd.hip calls (declared in
// device/launch.hpp): the filter directions the shadow pre-pass's own row filter does not cover, and the resolve of the AO rays
// (ao.hip's kernels, launched through ao_launch_primary / ao_launch_rays) into the pre-pass's source plane.
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_NPR_HATCHING_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/npr_hatching.hpp"

namespace atn {

void nh_launch_resolve(uint32_t slot_grid, hipStream_t st, const FrameParams& fp, const AoArgs& aa, float* src, float* depth)
{
    hipLaunchKernelGGL(k_hatch_ao_resolve, dim3(slot_grid), dim3(256), 0, st, fp, aa, src, depth);
}

void nh_launch_filter(int32_t direction, hipStream_t st, const float* src, const float* depth, float* first, float* out, int32_t width, int32_t height)
{
    const dim3 g(((uint32_t)width + 255u) / 256u, (uint32_t)height), t(256);
    switch (direction) {
    case kHatchNone: hipLaunchKernelGGL((k_hatch_filter<kHatchNone>), g, t, 0, st, src, depth, first, out, width, height); break;
    case kHatchHorizontal: ns_launch_filter(st, src, depth, out, width, height); break;       // the row filter that exists: k_ns_filter
    case kHatchVertical: hipLaunchKernelGGL((k_hatch_filter<kHatchVertical>), g, t, 0, st, src, depth, first, out, width, height); break;
    case kHatchOrthogonal: hipLaunchKernelGGL((k_hatch_filter<kHatchOrthogonal>), g, t, 0, st, src, depth, first, out, width, height); break;
    case kHatchCross: hipLaunchKernelGGL((k_hatch_filter<kHatchCross>), g, t, 0, st, src, depth, first, out, width, height); break;
    default: hipLaunchKernelGGL((k_hatch_filter<kHatchOrthogonalCross>), g, t, 0, st, src, depth, first, out, width, height); break;
    }
}

} // namespace atn
