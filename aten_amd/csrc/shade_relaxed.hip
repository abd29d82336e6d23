// k_shade under RELAXED floating-point rules, opt-in (atn_set_shade_math): what the reference's own GPU build does to the same
// formulas (src/libidaten/CMakeLists.txt:188 `--use_fast_math`: fused multiply-adds, approximate division and square root, the
// hardware's sin / cos / exp2 / log2 behind sinf / cosf / expf / logf / powf, denormals flushed).  NOT the parity path: the CPU
// renderer is an SSE2 build without FMA and the default kernels (aten_amd.hip) round every operation the way it does; this unit
// exists to put a number on what that costs and for callers who want the frames and not the bits.
// Same sources (device/kernels.hpp: shade_body), other flags (build.py, HIP_UNITS), the transcendental calls redirected below.
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define sinf __sinf
#define cosf __cosf
#define expf __expf
#define logf __logf
#define powf __powf
#include "../../include/aten_amd.h"
#include "device/launch.hpp"

namespace atn {

template <int MS>
__global__ void __launch_bounds__(256) k_shade_relaxed(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, int32_t bounce)
{
    shade_body<false, MS>(pb, sc, fp, cam, bounce, SvgfShade{});
}
template <int MS, int WAVES>
__global__ void __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) __launch_bounds__(256) k_shade_relaxed_wn(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, int32_t bounce)
{
    shade_body<false, MS>(pb, sc, fp, cam, bounce, SvgfShade{});
}

void relaxed_launch_shade(int material_set, int waves, uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                          const atn_camera_param& cam, int32_t bounce)
{
    with_shade_flavour(material_set, waves, [&](auto k) {
        using K = decltype(k);
        if constexpr (K::waves == 0) hipLaunchKernelGGL((k_shade_relaxed<K::ms>), dim3(grid), dim3(256), 0, st, pb, sc, fp, cam, bounce);
        else hipLaunchKernelGGL((k_shade_relaxed_wn<K::ms, K::waves>), dim3(grid), dim3(256), 0, st, pb, sc, fp, cam, bounce);
    });
}

} // namespace atn
