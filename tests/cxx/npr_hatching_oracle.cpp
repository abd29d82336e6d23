/*
 * NPR HATCHING ORACLE -- TEST INFRASTRUCTURE ONLY (tests/npr_hatching_oracle.py compiles it; the product never loads it).
 *
 * A CPU restatement of the filter stage of idaten::NPRPathTracing's hatching shadows (src/libidaten/npr/npr_pathtracing.cu:283-347,
 * 519-605): ao::ApplyBilateralFilter<., float, IsHorizontal, 5> and ao::ApplyBilateralFilterOrthogonal<., float, 5, +-5>
 * (src/libaten/renderer/ao/aorenderer_impl.h:138-244) with coefficients (2, 2) in the reference's evaluation order, NO_FILTER, and the
 * second steps (IsFirstStep = false: the second filter over the SOURCE plane, times the first step's value at the pixel, then
 * v < 1 ? v * 0.5 : v).  The source and depth planes come from the AO twin and the NPR shadow twin (tests/npr_hatching_oracle.py).
 * docs/NPR_HATCHING.md has the decisions.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

inline int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return std::min(std::max(v, lo), hi); }
inline float clampf(float v, float lo, float hi) { return std::min(std::max(v, lo), hi); }      // aten::clamp

// ApplyBilateralFilter<float, float, IsHorizontal, 5>, aorenderer_impl.h:138-191: coeff_depth_2 is computed and never used, the depth
// term is divided by the centre depth, -(i * i) is formed in int
template <bool IsHorizontal>
float ApplyBilateralFilter(int32_t center_x, int32_t center_y, int32_t width, int32_t height, float coeff_pixel_dist, float coeff_depth,
                           const float* values, const float* depths)
{
    const float coeff_pixel_dist_2 = 2 * (coeff_pixel_dist * coeff_pixel_dist);
    const float coeff_depth_2 = 2 * (coeff_depth * coeff_depth);
    (void)coeff_depth_2;
    const int32_t center_idx = center_y * width + center_x;
    const float center_depth = depths[center_idx];
    float numer = 0.0F, denom = 0.0F;
    for (int32_t i = -5; i <= 5; i++) {
        int32_t x = center_x, y = center_y;
        if (IsHorizontal) x = clampi(center_x + i, 0, width - 1);
        else y = clampi(center_y + i, 0, height - 1);
        const int32_t idx = y * width + x;
        const float depth = depths[idx];
        const float diff = center_depth - depth;
        const float kernel = std::exp(-(i * i) / coeff_pixel_dist_2 - (diff * diff) / center_depth);
        const float value = values[idx];
        numer += value * kernel;
        denom += kernel;
    }
    return clampf(denom > 0.0F ? numer / denom : 1.0F, 0.0F, 1.0F);
}

// ApplyBilateralFilterOrthogonal<float, float, KernelSizeH, KernelSizeV>, aorenderer_impl.h:193-244: the loop runs over h, the x step
// is int(inclination * h), the pixel distance is sqrt(step_v * step_v + h * h) as a float, squared in float
template <int32_t KernelSizeH, int32_t KernelSizeV>
float ApplyBilateralFilterOrthogonal(int32_t center_x, int32_t center_y, int32_t width, int32_t height, float coeff_pixel_dist,
                                     float coeff_depth, const float* values, const float* depths)
{
    const float coeff_pixel_dist_2 = 2 * (coeff_pixel_dist * coeff_pixel_dist);
    const float coeff_depth_2 = 2 * (coeff_depth * coeff_depth);
    (void)coeff_depth_2;
    const int32_t center_idx = center_y * width + center_x;
    const float center_depth = depths[center_idx];
    float numer = 0.0F, denom = 0.0F;
    constexpr float inclination = static_cast<float>(KernelSizeH) / KernelSizeV;
    for (int32_t h = -KernelSizeH; h <= KernelSizeH; h++) {
        const int32_t step_v = static_cast<int32_t>(inclination * h);
        const int32_t x = clampi(center_x + step_v, 0, width - 1);
        const int32_t y = clampi(center_y + h, 0, height - 1);
        const float i = std::sqrt(static_cast<float>(step_v * step_v + h * h));
        const int32_t idx = y * width + x;
        const float depth = depths[idx];
        const float diff = center_depth - depth;
        const float kernel = std::exp(-(i * i) / coeff_pixel_dist_2 - (diff * diff) / center_depth);
        const float value = values[idx];
        numer += value * kernel;
        denom += kernel;
    }
    return clampf(denom > 0.0F ? numer / denom : 1.0F, 0.0F, 1.0F);
}

// one step: 1 Horizontal, 2 Vertical, 3 Orthogonal <5, 5>, 6 Orthogonal <5, -5> (the second step of OrthogonalCross)
float Step(int32_t line, int32_t x, int32_t y, int32_t w, int32_t h, const float* src, const float* depths)
{
    switch (line) {
    case 1: return ApplyBilateralFilter<true>(x, y, w, h, 2.0F, 2.0F, src, depths);
    case 2: return ApplyBilateralFilter<false>(x, y, w, h, 2.0F, 2.0F, src, depths);
    case 3: return ApplyBilateralFilterOrthogonal<5, 5>(x, y, w, h, 2.0F, 2.0F, src, depths);
    default: return ApplyBilateralFilterOrthogonal<5, -5>(x, y, w, h, 2.0F, 2.0F, src, depths);
    }
}

} // namespace

extern "C" {

// direction: HatchingShadowDirection 0 None, 1 Horizontal, 2 Vertical, 3 Orthogonal, 4 Cross, 5 OrthogonalCross; 6 is the
// anti-diagonal alone (the second filter of OrthogonalCross without the product).  first (may be null): the first step's plane of
// directions 4 / 5 (for the others: the final plane).  Returns 0, or -1 for another direction.
int orc_nprh_filter(int32_t width, int32_t height, int32_t direction, const float* src, const float* depths, float* first, float* out)
{
    if (direction < 0 || direction > 6) return -1;
    for (int32_t y = 0; y < height; y++)
        for (int32_t x = 0; x < width; x++) {
            const int32_t idx = y * width + x;
            float v, a;
            if (direction == 0) v = a = src[idx];          // NO_FILTER
            else if (direction == 4 || direction == 5) {
                a = Step(direction == 4 ? 1 : 3, x, y, width, height, src, depths);
                float filtered_color = Step(direction == 4 ? 2 : 6, x, y, width, height, src, depths);
                filtered_color *= a;
                filtered_color = filtered_color < 1.0F ? filtered_color * 0.5F : filtered_color;
                v = filtered_color;
            }
            else v = a = Step(direction, x, y, width, height, src, depths);
            if (first) first[idx] = a;
            out[idx] = v;
        }
    return 0;
}

} // extern "C"
