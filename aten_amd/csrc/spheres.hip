// Analytic spheres (device/spheres.hpp) as a translation unit of its own, and the launchers aten_amd.hip calls (declared in
// device/launch.hpp): the sphere-aware walks -- plain, lane-refilling, plain over an LDS copy -- under the closest job, the shadow job
// (fused and separate launches, counted and uncounted) and atn_trace_closest's job, and the serial loop's shade launches for the
// material sets a frame with sphere leaves can hold (toon is refused).
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/spheres.hpp"

namespace atn {

void sph_launch_trace(bool shadow, bool count, bool refill, uint32_t grid, uint32_t block, hipStream_t st, const PathBuffers& pb, const DevScene& sc, int32_t b)
{
    const dim3 g(grid), t(block);
    with_flags([&](auto c, auto rf) {
        if (shadow) hipLaunchKernelGGL((k_sph_trace_shadow<decltype(c)::value, decltype(rf)::value>), g, t, 0, st, pb, sc, b);
        else hipLaunchKernelGGL((k_sph_trace_closest<decltype(c)::value, decltype(rf)::value>), g, t, 0, st, pb, sc, b);
    }, count, refill);
}

void sph_launch_trace_fused(const TraceLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, int32_t bs, int32_t bc, int32_t launch)
{
    const dim3 g(l.grid), t(l.block);
    if (l.closest) { hipLaunchKernelGGL((k_sph_trace_closest<false, false>), g, t, l.lds_bytes, st, pb, sc, bc); return; }
    with_flags([&](auto refill, auto lds) {
        hipLaunchKernelGGL((k_sph_trace_fused<decltype(refill)::value, decltype(lds)::value>), g, t, l.lds_bytes, st, pb, sc, bs, bc, launch);
    }, l.refill, l.lds);
}

void sph_launch_batch(bool count, bool refill, uint32_t grid, uint32_t block, hipStream_t st, const DevScene& sc, const atn_ray* rays, uint32_t n,
                      float t_min, float t_max, atn_intersection* out, unsigned long long* stats)
{
    with_flags([&](auto c, auto rf) {
        hipLaunchKernelGGL((k_sph_trace_batch<decltype(c)::value, decltype(rf)::value>), dim3(grid), dim3(block), 0, st, sc, rays, n, t_min, t_max, out, stats);
    }, count, refill);
}

int sph_launch_shade(int material_set, int waves, bool la, uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                     const atn_camera_param& cam, int32_t bounce)
{
    if (material_set >= kMsToon) return -1;     // (refused in front of the frame: no such instantiation)
    with_shade_flavour(material_set, waves, [&](auto k) {
        using K = decltype(k);
        if constexpr (K::ms >= kMsToon) return;
        else if constexpr (K::waves == 0) hipLaunchKernelGGL((k_sph_shade<K::ms>), dim3(grid), dim3(256), 0, st, pb, sc, fp, cam, bounce);
        else {
            if (la) hipLaunchKernelGGL((k_sph_shade_wn<K::ms, K::waves, true>), dim3(grid), dim3(256), 0, st, pb, sc, fp, cam, bounce);
            else hipLaunchKernelGGL((k_sph_shade_wn<K::ms, K::waves, false>), dim3(grid), dim3(256), 0, st, pb, sc, fp, cam, bounce);
        }
    });
    return 0;
}

} // namespace atn
