/*
 * NPR SHADOW ORACLE -- TEST INFRASTRUCTURE ONLY (tests/npr_shadow_oracle.py compiles it; the product never loads it).
 *
 * A CPU restatement of the screen-space shadow pre-pass of the reference's NPR renderers -- the first pass of
 * aten::NprPathTracer::OnRender (src/libaten/renderer/npr/npr.cpp:284-349,399-447) and idaten::NPRPathTracing::onShadeByShadowRay
 * (src/libidaten/npr/npr_pathtracing.cu:211-281,446-476,521-605) -- on top of the path-tracing oracle (oracle/orc_pt.h, read as it
 * is), with the decisions of docs/NPR_SHADOW.md: per pixel sample 0's primary ray into a FRESH intersection record, PathTracing::shade
 * at bounce 0 (it fills the shadow ray), the termination flag forced off, HitTestToTargetLight for an active ray; then
 * ApplyBilateralFilter<ShadowRay, float, true, 5> with coefficients (2, 2) (aorenderer_impl.h:138-191) over "the ray reached its
 * light" and the primary hit's t.
 */
#include "../../oracle/orc_pt.h"
#include <omp.h>
#include <algorithm>
#include <cmath>
#include <vector>

using namespace orc;

namespace {

// ApplyBilateralFilter<ShadowRay, float, /*IsHorizontal*/true, 5>, aorenderer_impl.h:138-191: the value is the ray's bit as 1 / 0,
// coeff_depth_2 is computed and never used, the depth term is divided by the centre depth
float ApplyBilateralFilterRow(int32_t center_x, int32_t center_y, int32_t width, float coeff_pixel_dist, float coeff_depth,
                              const float* lit, const float* depths)
{
    const float coeff_pixel_dist_2 = 2 * (coeff_pixel_dist * coeff_pixel_dist);
    const float coeff_depth_2 = 2 * (coeff_depth * coeff_depth);
    (void)coeff_depth_2;
    const int32_t center_idx = center_y * width + center_x;
    const float center_depth = depths[center_idx];
    float numer = 0.0F, denom = 0.0F;
    for (int32_t i = -5; i <= 5; i++) {
        const int32_t x = std::min(std::max(center_x + i, 0), width - 1);
        const int32_t idx = center_y * width + x;
        const float diff = center_depth - depths[idx];
        const float kernel = std::exp(-(i * i) / coeff_pixel_dist_2 - (diff * diff) / center_depth);
        const float value = lit[idx] != 0.0F ? 1.0F : 0.0F;
        numer += value * kernel;
        denom += kernel;
    }
    const float r = denom > 0.0F ? numer / denom : 1.0F;
    return std::min(std::max(r, 0.0F), 1.0F);      // aten::clamp
}

} // namespace

extern "C" {

struct orc_destination {    // oracle/aten_oracle.cpp's
    int32_t width, height, maxDepth, russianRouletteDepth, sample;
    uint32_t frame;
    int32_t progressive;
    int32_t nthreads;
};

// the filter alone over given planes [h][w]
void orc_nprs_filter(int32_t width, int32_t height, const float* lit, const float* depths, float* out)
{
    for (int32_t y = 0; y < height; y++)
        for (int32_t x = 0; x < width; x++)
            out[y * width + x] = ApplyBilateralFilterRow(x, y, width, 2.0F, 2.0F, lit, depths);
}

// The pre-pass of frame dst->frame: lit float[n] (1 / 0), depth float[n] (the primary t; inf for a miss), plane float[n] (filtered).
// Optional (null = skip): mtrl int32[n] the primary hit's material id (-1: a miss or a negative id).
int orc_nprs_prepass(const atn_scene_desc* scene, const atn_camera_param* camera, const uint32_t* seeds, uint32_t n_seeds,
                     const orc_destination* dst, float* lit, float* depth, float* plane, int32_t* mtrl)
{
    Scene ctxt(scene);
    const int32_t width = dst->width, height = dst->height;
    if (dst->nthreads > 0) omp_set_num_threads(dst->nthreads);
    int32_t rrDepth = dst->russianRouletteDepth;
    if (rrDepth > dst->maxDepth) rrDepth = dst->maxDepth - 1;      // pathtracing.cpp:282-284
#pragma omp parallel for schedule(dynamic, 4)
    for (int32_t y = 0; y < height; y++) {
        for (int32_t x = 0; x < width; x++) {
            const int32_t idx = y * width + x;
            const uint32_t rnd = seeds[idx % n_seeds];
            PathState path; path.samples = 0;
            Ray ray;
            GeneratePath(ray, x, y, 0, dst->frame, path, *camera, rnd);
            Isect isect;        // fresh: idaten's m_isects at bounce 0, not the CPU renderer's persistent isects_
            const bool is_hit = TraverseClosest(isect, ctxt, ray, EPS, INF, nullptr);
            bool reached = false;
            if (mtrl) mtrl[idx] = is_hit ? isect.mtrlid : -1;
            if (is_hit) {
                path.isHit = true;
                ShadowRay shadow_ray;
                shade(path, ctxt, ray, shadow_ray, isect, rrDepth, 0, nullptr);
                path.is_terminated = false;         // npr.cpp:305-307
                if (shadow_ray.isActive) {
                    const auto& light = ctxt.GetLight(shadow_ray.targetLightId);
                    const Ray original_ray(shadow_ray.rayorg, shadow_ray.raydir);
                    const int32_t stencil = isect.mtrlid >= 0 ? ctxt.GetMaterial(isect.mtrlid).stencil_type : 0;
                    reached = HitTestToTargetLight(ctxt, original_ray, light, shadow_ray.distToLight, stencil, nullptr);
                }
            }
            lit[idx] = reached ? 1.0F : 0.0F;
            depth[idx] = is_hit ? isect.t : std::numeric_limits<float>::infinity();
        }
    }
#pragma omp parallel for schedule(static)
    for (int32_t y = 0; y < height; y++)
        for (int32_t x = 0; x < width; x++)
            plane[y * width + x] = ApplyBilateralFilterRow(x, y, width, 2.0F, 2.0F, lit, depth);
    return 0;
}

} // extern "C"
