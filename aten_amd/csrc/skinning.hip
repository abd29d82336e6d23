// Skinning on the device (device/skinning.hpp) as a translation unit of its own, and the launchers aten_amd.hip calls (declared in
// device/launch.hpp): the vertex pass, the triangle pass, and the LBVH's Morton pass reading the skin's box from device memory.
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_SKINNING_TU 1
#define ATN_LBVH_HELPERS_ONLY 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/lbvh.hpp"
#include "device/skinning.hpp"

namespace atn {

void skin_launch_vertices(const SkinLaunch& l, hipStream_t st, const SkinVtxArgs& a)
{
    if (l.palette_lds) hipLaunchKernelGGL((k_skin_vertices<true>), dim3(l.vtx_grid), dim3(kSkinBlock), 0, st, a);
    else hipLaunchKernelGGL((k_skin_vertices<false>), dim3(l.vtx_grid), dim3(kSkinBlock), 0, st, a);
}

void skin_launch_triangles(const SkinLaunch& l, hipStream_t st, const SkinTriArgs& a)
{
    hipLaunchKernelGGL(k_skin_triangles, dim3(l.tri_grid), dim3(kSkinBlock), 0, st, a);
}

void skin_launch_morton(hipStream_t st, const atn_triangle_param* tris, const float4* vtx, int32_t vtx_offset, uint32_t n, const float* box,
                        uint32_t* codes, uint32_t* indices)
{
    hipLaunchKernelGGL(k_lbvh_morton_box, dim3((n + 255u) / 256u), dim3(256), 0, st, tris, vtx, vtx_offset, n, box, codes, indices);
}

} // namespace atn
