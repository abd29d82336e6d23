// The display tail (device/taa.hpp): temporal anti-aliasing, the history write and the gamma / RGBA8 epilogue as a translation unit of
// its own, and the launcher aten_amd.hip calls (declared in device/launch.hpp).
#include <hip/hip_runtime.h>

#define ATN_TEMPLATES_ONLY 1
#define ATN_TAA_TU 1
#include "../../include/aten_amd.h"
#include "device/launch.hpp"
#include "device/taa.hpp"

namespace atn {

void taa_launch_resolve(const TileLaunch& l, hipStream_t st, const TaaArgs& a)
{
    hipLaunchKernelGGL(k_taa, dim3(l.grid_x, l.grid_y), dim3(256), 0, st, a);
}

} // namespace atn
