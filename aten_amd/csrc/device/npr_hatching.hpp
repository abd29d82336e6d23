// NPR hatching shadows (idaten::NPRPathTracing's HatchingShadowBase x HatchingShadowDirection, src/libidaten/npr/npr_pathtracing.h:14-26,
// npr_pathtracing.cu:283-347,351-386,519-605): what the shadow pre-pass (device/npr_shadow.hpp) filters -- the bounce-0 lit bit or the
// ambient-occlusion value at the primary hit -- and how: no filter, a row, a column, a diagonal, or a two-step product with the
// `< 1 ? x 0.5` darkening that makes the strokes.  docs/NPR_HATCHING.md has the decisions.
//
// Base AO, per frame in front of the frame's sample loop:  k_gen_path (sample 0) -> k_ao_primary -> k_ao_shade -> k_ao_trace (ao.hip's
//   kernels as they are, over ray lists of the frame's bank) -> k_hatch_ao_resolve (the fold in ray order into the source plane, the
//   primary t into the depth plane) -> the filter.
// The filter: direction Horizontal is k_ns_filter itself (npr_shadow.hip); every other direction is k_hatch_filter<DIR> below (there
// is no DIR = 1 instantiation).
#pragma once
#include "kernels.hpp"
#include "ao.hpp"

namespace atn {

constexpr int32_t kHatchNone = 0, kHatchHorizontal = 1, kHatchVertical = 2, kHatchOrthogonal = 3, kHatchCross = 4, kHatchOrthogonalCross = 5;
constexpr int32_t kHatchRadius = 5;     // ApplyBilateralFilter<..., 5> / ApplyBilateralFilterOrthogonal<..., 5, +-5>: 11 taps

// ---- kernels (npr_hatching.hip) -----------------------------------------------------------------------------------------------
#ifdef ATN_NPR_HATCHING_TU

// One tap line of the depth-aware bilateral filter for pixel (cx, cy), coefficients (2, 2) (aorenderer_impl.h:138-244):
//   LINE 0  ApplyBilateralFilter<., ., true, 5>               the row            (cx + i, cy)
//   LINE 1  ApplyBilateralFilter<., ., false, 5>              the column         (cx, cy + i)
//   LINE 2  ApplyBilateralFilterOrthogonal<., ., 5, 5>        the diagonal       (cx + int(1.0 * h), cy + h)
//   LINE 3  ApplyBilateralFilterOrthogonal<., ., 5, -5>       the anti-diagonal  (cx + int(-1.0 * h), cy + h)
// Both coordinates are clamped on their own (a diagonal tap outside the plane slides along the border).  The row and the column
// form -(i * i) in int and divide it by 8; the diagonals take i = sqrt(float(step * step + h * h)) and square it in float.  The depth
// term is divided by the centre depth (coeff_depth is never used); a centre that missed (depth inf) makes every weight NaN and the
// result 1.
template <int LINE>
ATN_DEV float hatch_bilateral(const float* __restrict__ src, const float* __restrict__ depth, int32_t cx, int32_t cy, int32_t width, int32_t height)
{
    const float coeff_pixel_dist_2 = 2 * (2.0F * 2.0F);
    const float center_depth = depth[(size_t)cy * (size_t)width + (size_t)cx];
    float numer = 0.0F, denom = 0.0F;
#pragma unroll
    for (int32_t h = -kHatchRadius; h <= kHatchRadius; h++) {
        int32_t x = cx, y = cy;
        float dist;
        if (LINE == 0) { x = min(max(cx + h, 0), width - 1); dist = (float)(-(h * h)) / coeff_pixel_dist_2; }
        else if (LINE == 1) { y = min(max(cy + h, 0), height - 1); dist = (float)(-(h * h)) / coeff_pixel_dist_2; }
        else {
            const float inclination = LINE == 2 ? 5.0F / 5.0F : 5.0F / -5.0F;
            const int32_t step_v = (int32_t)(inclination * (float)h);
            x = min(max(cx + step_v, 0), width - 1);
            y = min(max(cy + h, 0), height - 1);
            const float i = sqrtf((float)(step_v * step_v + h * h));
            dist = -(i * i) / coeff_pixel_dist_2;
        }
        const size_t idx = (size_t)y * (size_t)width + (size_t)x;
        const float diff = center_depth - depth[idx];
        const float kernel = expf(dist - (diff * diff) / center_depth);
        numer += src[idx] * kernel;
        denom += kernel;
    }
    const float r = denom > 0.0F ? numer / denom : 1.0F;
    return sclamp(r, 0.0F, 1.0F);
}

// One pixel per lane, a block of 256 along a row (k_ns_filter's shape): a wave's 64 lanes read 64 consecutive floats per tap row, the
// column and diagonal taps being strided by the width.  The two-step directions are one launch: both steps read only the source and
// depth planes (npr_pathtracing.cu:337-342 reads the first step's value back from the surface at the same pixel), so the first step's
// value goes to `first` for the download and stays in a register for the product.  `first` is written by DIR 4 / 5 only.
template <int DIR>
__global__ void __launch_bounds__(256) k_hatch_filter(const float* __restrict__ src, const float* __restrict__ depth, float* __restrict__ first,
                                                       float* __restrict__ out, int32_t width, int32_t height)
{
    const int32_t x = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    const int32_t y = (int32_t)blockIdx.y;
    if (x >= width || y >= height) return;
    const size_t idx = (size_t)y * (size_t)width + (size_t)x;
    float v;
    if (DIR == kHatchNone) v = src[idx];        // NO_FILTER: neither clamped nor weighted
    else if (DIR == kHatchVertical) v = hatch_bilateral<1>(src, depth, x, y, width, height);
    else if (DIR == kHatchOrthogonal) v = hatch_bilateral<2>(src, depth, x, y, width, height);
    else {
        const float a = hatch_bilateral<DIR == kHatchCross ? 0 : 2>(src, depth, x, y, width, height);
        first[idx] = a;
        v = hatch_bilateral<DIR == kHatchCross ? 1 : 3>(src, depth, x, y, width, height);
        v *= a;
        v = v < 1.0F ? v * 0.5F : v;
    }
    out[idx] = v;
}

// ShandeByAO's result for every pixel of the frame into the hatching source plane, one slot per lane: k_ao_resolve's fold (the pixel's
// rays IN INDEX ORDER, a miss SETS the value to one, / num_rays; aorenderer_impl.h:99-111) without the film.  A primary miss is 1.0 with
// depth IEEE +inf (docs/NPR_SHADOW.md: the walk's AT_MATH_INF would make a background pixel 0).  No arrays, a rolled loop: nothing goes
// to the stack, and with a float4 load and four divisions per ray it stays far below the register count that would cost a wave.
__global__ void __launch_bounds__(256) k_hatch_ao_resolve(FrameParams fp, AoArgs aa, float* __restrict__ src, float* __restrict__ depth)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= (uint32_t)fp.n_slots) return;
    int32_t x, y;
    if (!slot_to_pixel(fp, slot, x, y)) return;
    const uint32_t idx = (uint32_t)(y * fp.width + x);
    float v = 1.0F, d = __int_as_float(0x7f800000);
    if (aa.state[idx] == kAoHit) {
        const uint32_t first = aa.work[slot];
        float ao = 0.0F;
#pragma unroll 1
        for (int32_t i = 0; i < aa.num_rays; i++) {
            const float4 r = aa.ray_res[first + (uint32_t)i];
            if (r.x == 0.0F) ao = 1.0F;
            else if (r.x == 1.0F && r.z > 0.0F) ao += r.y / aa.radius * r.z / aa.ray_n[first + (uint32_t)i].w;
        }
        ao /= (float)aa.num_rays;
        v = ao;
        d = aa.depth_s[slot];
    }
    src[idx] = v;
    depth[idx] = d;
}

#endif  // ATN_NPR_HATCHING_TU

} // namespace atn
