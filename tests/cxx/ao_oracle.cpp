/*
 * AO ORACLE -- TEST INFRASTRUCTURE ONLY (tests/ao_oracle.py compiles it; the product never loads it).
 *
 * A CPU restatement of the reference's ambient-occlusion renderer -- aten::AORenderer::radiance, RenderAO and
 * RenderAOWithBilateralFilter (src/libaten/renderer/ao/aorenderer.cpp:20-275) and the per-pixel code of aorenderer_impl.h
 * (ShandeByAO :33-117, ShadeByAOIfHitMiss :127-136, ApplyBilateralFilter :138-191) -- on top of the path-tracing oracle
 * (oracle/orc_pt.h, read as it is), with the decisions of docs/AO.md:
 *   idaten_miss = 0: the CPU renderer as written -- a primary miss terminates the path and `break`s out of the row's x loop, so the
 *                    missing pixel and the rest of its row are not put and keep what the film, the contributions and the
 *                    intersections held;
 *   idaten_miss = 1: idaten's kernels (src/libidaten/ao/ao.cu:14-78) -- a primary miss is 1.0 and every pixel is written.
 *   stale_isect = 1: the literal `Intersection& isect = isects_[idx]` -- Traverse does not clear it, so a frame's primary hit must
 *                    be nearer than the pixel's hit of the frame before (not reproduced by the product; off by default).
 * State across frames: path_host_ (contributions, attributes) and isects_, like the reference's members.
 */
#include "../../oracle/orc_pt.h"
#include <omp.h>
#include <cmath>
#include <cstring>
#include <vector>

using namespace orc;

namespace {

constexpr size_t MAX_LOOP = 10;     // aorenderer_impl.h:66

struct RayStage {       // the first AO ray of a pixel and its answer
    v3 org, dir;
    int32_t kind{ 0 };  // 0 miss, 1 hit, 2 ten skip-throughs
    float t{ 0 }, c{ 0 };
    int32_t skips{ 0 };
    bool valid{ false };
    bool normal_mapped{ false };    // the primary hit's material has a normal map
};

// material::isTranslucentByAlpha, material.cpp:193-210 (a negative material id is not indexed: HitTestToTargetLight's guard)
bool isTranslucentByAlpha(const Scene& ctxt, int32_t mtrlid, float u, float v)
{
    if (mtrlid < 0) return false;
    const auto& m = ctxt.GetMaterial(mtrlid);
    const v4 albedo = sampleTexture(ctxt, m.albedoMap, u, v, v4(1.0F));
    const float alpha = albedo.w * m.baseColor.w;
    return alpha < 1.0F;
}

// ShandeByAO, aorenderer_impl.h:33-117
float ShandeByAO(int32_t ao_num_rays, float ao_radius, CMJ& sampler, const Scene& ctxt, const Ray& ray, const Isect& isect,
                 RayStage* st, int32_t* skip_total, atn_vec4* all)
{
    HitRec rec;
    evaluate_hit_result(rec, ctxt.GetObject((uint32_t)isect.objid), ctxt, ray, isect);
    v3 orienting_normal = rec.normal;
    atn_material_param base_mtrl;
    FillMaterial(base_mtrl, ctxt, rec.mtrlid);
    applyNormal(ctxt, base_mtrl, orienting_normal, orienting_normal, rec.u, rec.v, ray.dir, &sampler);

    float ao_color = 0.0F;
    for (int32_t i = 0; i < ao_num_rays; i++) {
        const float r1 = sampler.nextSample();
        const float r2 = sampler.nextSample();
        const v3 nextDir = Diffuse::SampleDirection(orienting_normal, r1, r2);
        Ray ao_ray(rec.p, nextDir, orienting_normal);
        RayStage rs;
        rs.org = ao_ray.org; rs.dir = ao_ray.dir; rs.valid = true;
        rs.kind = 2;
        for (size_t n = 0; n < MAX_LOOP; n++) {
            Isect ao_isect;
            const bool isHit = TraverseClosest(ao_isect, ctxt, ao_ray, EPS, ao_radius, nullptr);
            if (isHit) {
                HitRec ao_rec;
                evaluate_hit_result(ao_rec, ctxt.GetObject((uint32_t)ao_isect.objid), ctxt, ao_ray, ao_isect);
                v3 ao_orienting_normal = ao_rec.normal;
                rs.t = ao_isect.t;
                if (isTranslucentByAlpha(ctxt, ao_isect.mtrlid, ao_rec.u, ao_rec.v)) {
                    const bool is_same_facing = dot(ao_rec.normal, ao_ray.dir) > 0.0F;
                    if (!is_same_facing) ao_orienting_normal = -ao_orienting_normal;
                    ao_ray = Ray(ao_rec.p, ao_ray.dir, ao_orienting_normal);
                    rs.skips++;
                    if (skip_total) (*skip_total)++;
                    continue;
                }
                else {
                    const float c = dot(ao_orienting_normal, nextDir);
                    if (c > 0.0F) {
                        const float pdfb = Diffuse::ComputePDF(orienting_normal, nextDir);
                        ao_color += ao_isect.t / ao_radius * c / pdfb;
                    }
                    rs.kind = 1; rs.c = c;
                    break;
                }
            }
            else {
                ao_color = 1.0F;
                rs.kind = 0; rs.t = 0.0F;
                break;
            }
        }
        rs.normal_mapped = base_mtrl.normalMap >= 0;
        if (i == 0 && st) *st = rs;
        if (all) all[i] = atn_vec4{ (float)rs.kind, rs.t, rs.c, (float)rs.skips };
    }
    ao_color /= ao_num_rays;
    return ao_color;
}

// ApplyBilateralFilter<PathContrib, float, IsHorizontal, 3>, aorenderer_impl.h:138-191 (coeff_depth_2 is computed and never used)
template <bool IsHorizontal>
float ApplyBilateralFilter(int32_t center_x, int32_t center_y, int32_t width, int32_t height, float coeff_pixel_dist, float coeff_depth,
                           const float* values, const Isect* isects)
{
    const float coeff_pixel_dist_2 = 2 * (coeff_pixel_dist * coeff_pixel_dist);
    const float coeff_depth_2 = 2 * (coeff_depth * coeff_depth);
    (void)coeff_depth_2;
    const int32_t center_idx = center_y * width + center_x;
    const float center_depth = isects[center_idx].t;
    float numer = 0.0F, denom = 0.0F;
    for (int32_t i = -3; i <= 3; i++) {
        int32_t x = center_x, y = center_y;
        if (IsHorizontal) x = std::min(std::max(center_x + i, 0), width - 1);
        else y = std::min(std::max(center_y + i, 0), height - 1);
        const int32_t idx = y * width + x;
        const float depth = isects[idx].t;
        const float diff = center_depth - depth;
        const float kernel = std::exp(-(i * i) / coeff_pixel_dist_2 - (diff * diff) / center_depth);
        const float value = values[idx];
        numer += value * kernel;
        denom += kernel;
    }
    const float r = denom > 0.0F ? numer / denom : 1.0F;
    return std::min(std::max(r, 0.0F), 1.0F);      // aten::clamp
}

struct State {
    // path_host_: contrib.x, attr.isHit / is_terminated are rewritten by GeneratePath every frame for the pixels it reaches
    std::vector<float> contrib;
    std::vector<Isect> isects;
    std::vector<float> bilateral;
    int32_t w{ 0 }, h{ 0 };
};

// FilmProgressive::put / Film::put (renderer/film.cpp:33-45,61-71)
void put(atn_vec4& cur, const v4& v, int32_t progressive)
{
    if (progressive) {
        const float nn = static_cast<float>(static_cast<int32_t>(cur.w));
        v4 cc(cur.x, cur.y, cur.z, cur.w);
        cc = nn * cc + v;
        const float d = nn + 1;
        cur.x = cc.x / d; cur.y = cc.y / d; cur.z = cc.z / d;
        cur.w = nn + 1;
    }
    else { cur.x = v.x; cur.y = v.y; cur.z = v.z; cur.w = v.w; }
}

} // namespace

extern "C" {

struct orc_destination {    // oracle/aten_oracle.cpp's
    int32_t width, height, maxDepth, russianRouletteDepth, sample;
    uint32_t frame;
    int32_t progressive;
    int32_t nthreads;
};

void* orc_ao_create() { return new State(); }
void orc_ao_destroy(void* h) { delete static_cast<State*>(h); }
void orc_ao_reset(void* h) { State& S = *static_cast<State*>(h); S.contrib.clear(); S.isects.clear(); S.bilateral.clear(); S.w = S.h = 0; }

// One frame into `film` (vec4[w*h]).  filter: RenderAOWithBilateralFilter instead of RenderAO.  Optional outputs (null = skip), per
// pixel: state uint32 {0 not rendered, 1 hit, 2 miss}; value float (contrib.x as it stands after the frame); depth float (isects_.t as
// it stands); ray float4[n][2] {org, the hit material has a normal map} {dir, 0} and answer float4[n] {kind, t, c, skip-throughs} of the first AO ray (pixels in
// state 1; zero elsewhere); skips int32[n] the skip-throughs of ALL AO rays of the pixel; first_miss int32[h] (width: none);
// answers_all float4[n][num_rays] the answers of all AO rays (zeroed first; pixels in state 1).
int orc_ao_render(void* h, const atn_scene_desc* scene, const atn_camera_param* camera, const uint32_t* seeds, uint32_t n_seeds,
                  const orc_destination* dst, int32_t num_rays, float radius, int32_t filter, int32_t idaten_miss, int32_t stale_isect,
                  atn_vec4* film, uint32_t* state, float* value, float* depth, atn_vec4* ray, atn_vec4* answer, int32_t* skips,
                  int32_t* first_miss, atn_vec4* answers_all)
{
    State& S = *static_cast<State*>(h);
    Scene ctxt(scene);
    const int32_t width = dst->width, height = dst->height;
    const size_t n = (size_t)width * height;
    if (dst->nthreads > 0) omp_set_num_threads(dst->nthreads);
    if (S.w != width || S.h != height) {
        S.contrib.assign(n, 0.0F); S.isects.assign(n, Isect()); S.bilateral.assign(n, 0.0F);
        S.w = width; S.h = height;
    }
    const uint32_t frame = dst->frame;
    if (answers_all) std::memset(answers_all, 0, n * (size_t)num_rays * sizeof(atn_vec4));

#pragma omp parallel for schedule(dynamic, 4)
    for (int32_t y = 0; y < height; y++) {
        if (first_miss) first_miss[y] = width;
        bool broke = false;
        for (int32_t x = 0; x < width; x++) {
            const int32_t idx = y * width + x;
            if (broke) {
                if (state) state[idx] = 0;
                if (ray) { ray[2 * (size_t)idx] = atn_vec4{ 0, 0, 0, 0 }; ray[2 * (size_t)idx + 1] = atn_vec4{ 0, 0, 0, 0 }; }
                if (answer) answer[idx] = atn_vec4{ 0, 0, 0, 0 };
                if (skips) skips[idx] = 0;
                continue;
            }
            const uint32_t rnd = seeds[idx % n_seeds];
            PathState path; path.samples = 0;
            Ray r;
            GeneratePath(r, x, y, 0, frame, path, *camera, rnd);
            // radiance, aorenderer.cpp:20-55
            const uint32_t scramble = rnd * 0x1fe3434f * ((frame + 331 * rnd) / (CMJ::CMJ_DIM * CMJ::CMJ_DIM));
            path.sampler.init(frame % (CMJ::CMJ_DIM * CMJ::CMJ_DIM), 4 + 5 * 300, scramble);
            Isect& isect = S.isects[idx];
            if (!stale_isect) isect = Isect();
            const bool is_hit = TraverseClosest(isect, ctxt, r, EPS, INF, nullptr);
            float ao_color = 0.0F;
            RayStage st;
            int32_t skip_total = 0;
            if (is_hit) {
                path.isHit = true;
                ao_color = ShandeByAO(num_rays, radius, path.sampler, ctxt, r, isect, &st, &skip_total,
                                      answers_all ? answers_all + (size_t)idx * num_rays : nullptr);
            }
            else {
                // ShadeByAOIfHitMiss, aorenderer_impl.h:127-136
                if (!path.is_terminated && !path.isHit) { path.is_terminated = true; ao_color = 1.0F; }
                else ao_color = -1.0F;
            }
            if (state) state[idx] = is_hit ? 1u : 2u;
            if (ray) {
                ray[2 * (size_t)idx] = st.valid ? atn_vec4{ st.org.x, st.org.y, st.org.z, st.normal_mapped ? 1.0F : 0.0F } : atn_vec4{ 0, 0, 0, 0 };
                ray[2 * (size_t)idx + 1] = st.valid ? atn_vec4{ st.dir.x, st.dir.y, st.dir.z, 0 } : atn_vec4{ 0, 0, 0, 0 };
            }
            if (answer) answer[idx] = st.valid ? atn_vec4{ (float)st.kind, st.t, st.c, (float)st.skips } : atn_vec4{ 0, 0, 0, 0 };
            if (skips) skips[idx] = skip_total;
            if (!is_hit && first_miss && first_miss[y] == width) first_miss[y] = x;
            if (idaten_miss) {
                // shadeMissAO / shadeAO, ao.cu:14-78: the miss value is written, nothing breaks
                S.contrib[idx] = ao_color;
            }
            else {
                if (!path.is_terminated) S.contrib[idx] = ao_color;
                if (path.is_terminated) { broke = true; continue; }     // `break`, aorenderer.cpp:136-138 / :208-210
            }
            if (!filter) {
                v3 col(0);
                col += v3(S.contrib[idx]);
                col /= (float)1;
                put(film[idx], v4(col, 1), dst->progressive);
            }
        }
    }
    if (filter) {
#pragma omp parallel for schedule(static)
        for (int32_t y = 0; y < height; y++)
            for (int32_t x = 0; x < width; x++)
                S.bilateral[y * width + x] = ApplyBilateralFilter<true>(x, y, width, height, 2.0F, 2.0F, S.contrib.data(), S.isects.data());
#pragma omp parallel for schedule(static)
        for (int32_t y = 0; y < height; y++) {
            for (int32_t x = 0; x < width; x++) {
                const int32_t idx = y * width + x;
                S.bilateral[idx] *= ApplyBilateralFilter<false>(x, y, width, height, 2.0F, 2.0F, S.contrib.data(), S.isects.data());
                float c = S.bilateral[idx];
                c = c < 1.0F ? c * 0.5F : c;
                put(film[idx], v4(c, c, c, 1), dst->progressive);
            }
        }
    }
    for (size_t i = 0; i < n; i++) {
        if (value) value[i] = S.contrib[i];
        if (depth) depth[i] = S.isects[i].t;
    }
    return 0;
}

// the filter alone over given planes (hand-worked cases): out[n] = the value put into the film
void orc_ao_filter(int32_t width, int32_t height, const float* values, const float* depths, float* out)
{
    std::vector<Isect> is((size_t)width * height);
    for (size_t i = 0; i < is.size(); i++) is[i].t = depths[i];
    for (int32_t y = 0; y < height; y++) {
        for (int32_t x = 0; x < width; x++) {
            float c = ApplyBilateralFilter<true>(x, y, width, height, 2.0F, 2.0F, values, is.data());
            c *= ApplyBilateralFilter<false>(x, y, width, height, 2.0F, 2.0F, values, is.data());
            out[y * width + x] = c < 1.0F ? c * 0.5F : c;
        }
    }
}

} // extern "C"
