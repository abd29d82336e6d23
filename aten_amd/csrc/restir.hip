// ReSTIR (device/restir.hpp): the bounce-0 shade, the visibility-ray preparation, the temporal and spatial reuse passes and the
// pixel colour as a translation unit of their own, and the launchers aten_amd.hip calls (declared in device/launch.hpp).  The
// material-set templates of kernels.hpp they use are instantiated here with the main unit's flags (build.py: -fno-slp-vectorize).
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_RESTIR_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/restir.hpp"

namespace atn {

namespace {
// the material sets ReSTIR is built for (the toon set is refused by the host: the reference's ReSTIR shade has no toon path)
template <class F>
void with_restir_set(int material_set, F&& f)
{
    switch (material_set) {
    case kMsCore: f(std::integral_constant<int, kMsCore>{}); break;
    case kMsDisney: f(std::integral_constant<int, kMsDisney>{}); break;
    case kMsAnalytic: f(std::integral_constant<int, kMsAnalytic>{}); break;
    default: f(std::integral_constant<int, kMsCarPaint>{}); break;
    }
}
dim3 pixel_grid(const FrameParams& fp) { return dim3((uint32_t)(fp.width + 15) / 16u, (uint32_t)(fp.height + 15) / 16u); }
}

void restir_launch_shade(int material_set, uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                         const atn_camera_param& cam, const RestirArgs& ra)
{
    with_restir_set(material_set, [&](auto ms) {
        constexpr int MS = decltype(ms)::value;
        if constexpr (MS <= kMsDisney) hipLaunchKernelGGL((k_restir_shade<MS>), dim3(grid), dim3(256), 0, st, pb, sc, fp, cam, ra);
        else hipLaunchKernelGGL((k_restir_shade_wide<MS>), dim3(grid), dim3(256), 0, st, pb, sc, fp, cam, ra);
    });
}

void restir_launch_vis_prep(uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const RestirArgs& ra)
{
    hipLaunchKernelGGL(k_restir_vis_prep, dim3(grid), dim3(256), 0, st, pb, sc, fp, ra);
}

void restir_launch_temporal(int material_set, bool temporal, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                            const RestirArgs& ra)
{
    with_restir_set(material_set, [&](auto ms) {
        constexpr int MS = decltype(ms)::value;
        if (temporal) hipLaunchKernelGGL((k_restir_temporal<MS, true>), pixel_grid(fp), dim3(16, 16), 0, st, pb, sc, fp, ra);
        else hipLaunchKernelGGL((k_restir_temporal<MS, false>), pixel_grid(fp), dim3(16, 16), 0, st, pb, sc, fp, ra);
    });
}

void restir_launch_spatial(int material_set, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const RestirArgs& ra)
{
    with_restir_set(material_set, [&](auto ms) {
        hipLaunchKernelGGL((k_restir_spatial<decltype(ms)::value>), pixel_grid(fp), dim3(16, 16), 0, st, pb, sc, fp, ra);
    });
}

void restir_launch_color(int material_set, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const RestirArgs& ra)
{
    with_restir_set(material_set, [&](auto ms) {
        hipLaunchKernelGGL((k_restir_color<decltype(ms)::value>), pixel_grid(fp), dim3(16, 16), 0, st, pb, sc, fp, ra);
    });
}

void restir_launch_motion(hipStream_t st, const FrameParams& fp, const RestirArgs& ra)
{
    hipLaunchKernelGGL(k_restir_motion, pixel_grid(fp), dim3(16, 16), 0, st, fp, ra);
}

} // namespace atn
