/*
 * ORACLE -- TEST INFRASTRUCTURE ONLY.
 *
 * C entry points (ctypes) over the CPU restatement in orc_*.h.  Loaded only by tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg -- never by aten_amd/.
 * Parity status: see orc_core.h header ("parity unpinned" except the three reference KATs).
 */
#include "orc_pt.h"
#include "orc_svgf.h"
#include "orc_lbvh.h"
#include <cstdio>
#include <omp.h>

using namespace orc;

extern "C" {

// aten::initSampler, sampler/sampler.cpp:8-18
void orc_init_sampler(uint32_t* out, int w, int h, int seed)
{
    std::vector<uint32_t> s;
    init_sampler(s, w, h, seed);
    std::memcpy(out, s.data(), s.size() * 4);
}

// n successive CMJ::nextSample() values after init(index, dimension, scramble)
void orc_cmj_samples(uint32_t index, uint32_t dimension, uint32_t scramble, int n, float* out)
{
    CMJ c; c.init(index, dimension, scramble);
    for (int i = 0; i < n; i++) out[i] = c.nextSample();
}

// n successive CMJ::nextSample2D(): out[2i] = x, out[2i+1] = y (cmj.h:39-44)
void orc_cmj_samples2d(uint32_t index, uint32_t dimension, uint32_t scramble, int n, float* out)
{
    CMJ c; c.init(index, dimension, scramble);
    for (int i = 0; i < n; i++) c.nextSample2D(out[2 * i], out[2 * i + 1]);
}

// per triple k: init(idx[k], dim[k], scr[k]) then `draws` x nextSample()  (twin of oracle/ref_driver.cpp)
void orc_cmj_batch(int32_t n, const uint32_t* idx, const uint32_t* dim, const uint32_t* scr, int32_t draws, float* out)
{
    for (int32_t k = 0; k < n; k++) {
        CMJ c; c.init(idx[k], dim[k], scr[k]);
        for (int32_t d = 0; d < draws; d++) out[(size_t)k * draws + d] = c.nextSample();
    }
}

// The oracle's restatements of math/math.h's scalar helpers, by the kinds of ref_math_kat (oracle/ref_driver.cpp),
// so that tests/test_ref_pin.py can hold them against the reference's own header.
void orc_math_kat(int32_t kind, int32_t n, const float* a, const float* b, const float* c, float* out)
{
    for (int32_t i = 0; i < n; i++) {
        switch (kind) {
        case 0: out[i] = fmax_(a[i], b[i]); break;                       // math.h:146-150
        case 1: out[i] = fmin_(a[i], b[i]); break;                       // math.h:172-176
        case 2: out[i] = clamp_(a[i], b[i], c[i]); break;                // math.h:179-183
        case 3: out[i] = saturate_(a[i]); break;                         // math.h:185-189
        case 4: out[i] = ToonSpecular::sign(a[i]); break;                             // math.h:62-73
        case 5: out[i] = mix(a[i], b[i], c[i]); break;                   // math.h:294-300
        case 6: out[i] = a[i] * (1.0F - c[i]) + b[i] * c[i]; break;      // math.h:191-194 (lerp, as in orc_core.h's bilinear)
        case 7: out[i] = isCloseUlps(a[i], b[i], 2500) ? 1.0F : 0.0F; break;   // math.h:308-340
        case 8: out[i] = (std::isnan(a[i]) || std::isinf(a[i])) ? 1.0F : 0.0F; break;   // math.h:196-204
        case 9: out[i] = sqr(a[i]); break;                               // math.h:42-45
        case 10: out[i] = inversesqrt(a[i]); break;                      // math.h:33-40
        case 11: out[i] = Deg2Rad(a[i]); break;                          // math.h:18-21
        default: out[i] = 0.0F;
        }
    }
}

// The math-library functions the float path calls, as THIS build's libm answers them (the oracle's side of the ulp study,
// tools/ulp_study.py: which function's last bit the GPU's ocml disagrees on).  kind: 0 sinf 1 cosf 2 atanf 3 acosf 4 atan2f(a, b)
// 5 logf 6 expf 7 powf(a, b) 8 sqrtf 9 a / b 10 1 / sqrtf(a) as orc_math.h's inversesqrt writes it
void orc_libm_probe(int32_t kind, int32_t n, const float* a, const float* b, float* out)
{
    for (int32_t i = 0; i < n; i++) {
        switch (kind) {
        case 0: out[i] = std::sin(a[i]); break;
        case 1: out[i] = std::cos(a[i]); break;
        case 2: out[i] = std::atan(a[i]); break;
        case 3: out[i] = std::acos(a[i]); break;
        case 4: out[i] = std::atan2(a[i], b[i]); break;
        case 5: out[i] = std::log(a[i]); break;
        case 6: out[i] = std::exp(a[i]); break;
        case 7: out[i] = std::pow(a[i], b[i]); break;
        case 8: out[i] = std::sqrt(a[i]); break;
        case 9: out[i] = a[i] / b[i]; break;
        case 10: out[i] = inversesqrt(a[i]); break;
        default: out[i] = 0.0F;
        }
    }
}

void orc_create_camera(atn_camera_param* out, const float* origin, const float* lookat, const float* up,
    float vfov, float z_near, float z_far, int32_t width, int32_t height)
{
    *out = CreateCameraParam(ld3(origin), ld3(lookat), ld3(up), vfov, z_near, z_far, width, height);
}

float orc_pixel_width_at_distance(const atn_camera_param* cam, float dist)
{
    return ComputePixelWidthAtDistance(*cam, dist);
}

void orc_ray_offset(const float* o, const float* n, int count, float* out)
{
    for (int i = 0; i < count; i++) {
        v3 r = Ray::Offset(ld3(o + 3 * i), ld3(n + 3 * i));
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    }
}

// GeneratePath for every pixel of a w x h image (sample index `sample`, frame `frame`).
void orc_generate_paths(const atn_camera_param* cam, const uint32_t* seeds, uint32_t n_seeds,
    int w, int h, int sample, uint32_t frame, atn_ray* rays_out)
{
#pragma omp parallel for
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            int idx = y * w + x;
            PathState p; Ray r;
            GeneratePath(r, x, y, sample, frame, p, *cam, seeds[idx % n_seeds]);
            atn_ray& o = rays_out[idx];
            o.org[0] = r.org.x; o.org[1] = r.org.y; o.org[2] = r.org.z;
            o.dir[0] = r.dir.x; o.dir[1] = r.dir.y; o.dir[2] = r.dir.z;
        }
    }
}

// Traverse<Closest> for a batch of rays.  stats_out = {node visits, triangle tests} (may be null)
void orc_trace_closest(const atn_scene_desc* scene, const atn_ray* rays, uint32_t n,
    float t_min, float t_max, atn_intersection* out, uint64_t* stats_out)
{
    Scene ctxt(scene);
    uint64_t nodes = 0, tris = 0;
#pragma omp parallel for reduction(+:nodes,tris)
    for (int64_t i = 0; i < (int64_t)n; i++) {
        Ray r; r.org = ld3(rays[i].org); r.dir = ld3(rays[i].dir);
        Isect is; TraverseStats st;
        TraverseClosest(is, ctxt, r, t_min, t_max, &st);
        nodes += st.nodes; tris += st.tris;
        atn_intersection& o = out[i];
        o.t = is.t; o.objid = is.objid; o.mtrlid = is.mtrlid; o.meshid = is.meshid;
        o.tri_id = is.tri_id; o.a = is.a; o.b = is.b; o.isVoxel = is.isVoxel;
    }
    if (stats_out) { stats_out[0] = nodes; stats_out[1] = tris; }
}

// HitTestToTargetLight for a batch of shadow rays, with Ray(org, dir) re-normalising as HitShadowRay does.  visible[i] = the verdict;
// lookups_out (optional) = the lookups made; last_out (optional) = the last lookup's closest hit (objid < 0: a miss).
// surface_stencil_always[i] != 0: the shaded surface's material is StencilType::ALWAYS.
void orc_shadow_visible(const atn_scene_desc* scene, const atn_shadow_query* q, uint32_t n, uint8_t* visible,
    int32_t* lookups_out, atn_intersection* last_out)
{
    Scene ctxt(scene);
#pragma omp parallel for
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const Ray original_ray(ld3(q[i].org), ld3(q[i].dir));
        ShadowTrace tr;
        visible[i] = HitTestToTargetLight(ctxt, original_ray, ctxt.GetLight(q[i].light), q[i].dist_to_light, (q[i].flags & 1u) ? 1 : 0, nullptr, &tr) ? 1 : 0;
        if (lookups_out) lookups_out[i] = tr.lookups;
        if (last_out) {
            atn_intersection& o = last_out[i];
            const Isect& is = tr.last;
            o.t = is.t; o.objid = tr.last_is_hit ? is.objid : -1; o.mtrlid = is.mtrlid; o.meshid = is.meshid;
            o.tri_id = is.tri_id; o.a = is.a; o.b = is.b; o.isVoxel = is.isVoxel;
        }
    }
}

// evaluate_hit_result for a batch of (ray, intersection): out = {p.xyz, area, n.xyz, u, v} (9 floats)
void orc_evaluate_hits(const atn_scene_desc* scene, const atn_ray* rays, const atn_intersection* isects,
    uint32_t n, float* out)
{
    Scene ctxt(scene);
    for (uint32_t i = 0; i < n; i++) {
        Isect is; is.t = isects[i].t; is.objid = isects[i].objid; is.mtrlid = isects[i].mtrlid;
        is.meshid = isects[i].meshid; is.tri_id = isects[i].tri_id; is.a = isects[i].a; is.b = isects[i].b;
        float* o = out + 9 * i;
        if (is.objid < 0) { for (int k = 0; k < 9; k++) o[k] = 0; continue; }
        Ray r; r.org = ld3(rays[i].org); r.dir = ld3(rays[i].dir);
        HitRec rec;
        evaluate_hit_result(rec, ctxt.GetObject(is.objid), ctxt, r, is);
        o[0] = rec.p.x; o[1] = rec.p.y; o[2] = rec.p.z; o[3] = rec.area;
        o[4] = rec.normal.x; o[5] = rec.normal.y; o[6] = rec.normal.z; o[7] = rec.u; o[8] = rec.v;
    }
}

// BSDF tables.  For case i: normal n[i], incoming wi[i], sampler (index[i], dimension 0, scramble[i]),
// uv[i].  out_sample = {dir.xyz, bsdf.xyz, pdf} ; then pdf/bsdf re-evaluated at wo = sampled dir:
// out_eval = {samplePDF, sampleBSDF.bsdf.xyz, sampleBSDF.pdf}.
void orc_material_table(const atn_scene_desc* scene, int32_t mtrl_id, uint32_t n,
    const float* nrm, const float* wi, const uint32_t* index, const uint32_t* scramble, const float* uv,
    float* out_sample, float* out_eval)
{
    Scene ctxt(scene);
    atn_material_param m;
    FillMaterial(m, ctxt, mtrl_id);
    for (uint32_t i = 0; i < n; i++) {
        CMJ s; s.init(index[i], 0, scramble[i]);
        MaterialSampling ms;
        v3 N = ld3(nrm + 3 * i), WI = ld3(wi + 3 * i);
        float pre_r = 0.0F;
        if (m.type == ATN_MTRL_CARPAINT) {      // material::applyNormal runs first, as in shade
            v3 nn;
            pre_r = applyNormal(ctxt, m, N, nn, uv[2 * i], uv[2 * i + 1], WI, &s);
            N = nn;
        }
        sampleMaterial(&ms, ctxt, &m, N, WI, &s, uv[2 * i], uv[2 * i + 1], pre_r);
        float* o = out_sample + 7 * i;
        o[0] = ms.dir.x; o[1] = ms.dir.y; o[2] = ms.dir.z;
        o[3] = ms.bsdf.x; o[4] = ms.bsdf.y; o[5] = ms.bsdf.z; o[6] = ms.pdf;
        float p = samplePDF(ctxt, &m, N, WI, ms.dir, uv[2 * i], uv[2 * i + 1]);
        MaterialSampling ev = sampleBSDF(ctxt, &m, N, WI, ms.dir, uv[2 * i], uv[2 * i + 1], pre_r);
        float* e = out_eval + 5 * i;
        e[0] = p; e[1] = ev.bsdf.x; e[2] = ev.bsdf.y; e[3] = ev.bsdf.z; e[4] = ev.pdf;
    }
}

struct orc_destination {    // aten::Destination (renderer/renderer.h:15-23) + explicit frame
    int32_t width, height, maxDepth, russianRouletteDepth, sample;
    uint32_t frame;
    int32_t progressive;    // 1: FilmProgressive::put (film.cpp:61-71), 0: Film::put (film.cpp:33-45)
    int32_t nthreads;       // OMPUtil::setThreadNum; <=0 = all
};

// aten::PathTracing::OnRender, renderer/pathtracing/pathtracing.cpp:269-366.
// film: vec4[w*h], row 0 = bottom.  counters_out (may be null): {closest rays, shadow rays, hits,
// node visits, triangle tests}.
// Optional samplers of the product (atn_set_sampling_options), so that they too have a CPU twin to be compared with.
void orc_set_sampling_options(int32_t ibl_importance, int32_t tex_bilinear)
{
    sampling_options().ibl_importance = ibl_importance;
    sampling_options().tex_bilinear = tex_bilinear;
}

// texture::at / texture::AtWithBilinear for n lookups of one texture (current texture mode)
void orc_sample_texture(const atn_scene_desc* scene, int32_t texid, uint32_t n, const float* uv, float* out)
{
    Scene ctxt(scene);
    for (uint32_t i = 0; i < n; i++) {
        const v4 c = sampleTexture(ctxt, texid, uv[2 * i], uv[2 * i + 1], v4(0.0F));
        out[4 * i] = c.x; out[4 * i + 1] = c.y; out[4 * i + 2] = c.z; out[4 * i + 3] = c.w;
    }
}

// ImageBasedLight::preCompute's tables (cdfV[h], cdfU[h*w]) for the scene's environment map
int32_t orc_ibl_tables(const atn_scene_desc* scene, float* cdf_v, float* cdf_u)
{
    Scene ctxt(scene);
    if (ctxt.cfg().bg.envmap_tex_idx < 0) return -1;
    SamplingOptions& o = sampling_options();
    IBL_preCompute(o, ctxt);
    for (int32_t y = 0; y < o.h; y++) {
        cdf_v[y] = o.cdfV[y];
        for (int32_t x = 0; x < o.w; x++) cdf_u[(size_t)y * o.w + x] = o.cdfU[y][x];
    }
    return 0;
}

// cost_out (may be null): uint32 {BVH node visits, triangle tests}[h][w] of all the pixel's walks of this frame -- what the
// product's atn_download_path_cost reports (its stand-in for the reference's PathTimeProfiler heat map)
void orc_render_cost(const atn_scene_desc* scene, const atn_camera_param* camera,
    const uint32_t* seeds, uint32_t n_seeds, const orc_destination* dst, atn_vec4* film,
    uint64_t* counters_out, uint32_t* cost_out)
{
    Scene ctxt(scene);
    if (sampling_options().ibl_importance && ctxt.cfg().bg.envmap_tex_idx >= 0 && ctxt.cfg().bg.enable_env_map)
        IBL_preCompute(sampling_options(), ctxt);
    const int32_t width = dst->width, height = dst->height;
    const uint32_t samples = (uint32_t)dst->sample;
    int32_t maxDepth = dst->maxDepth;
    int32_t rrDepth = dst->russianRouletteDepth;
    if (rrDepth > maxDepth) rrDepth = maxDepth - 1;     // pathtracing.cpp:282-284

    uint64_t c_closest = 0, c_shadow = 0, c_hits = 0, c_nodes = 0, c_tris = 0;
    const bool count = counters_out != nullptr || cost_out != nullptr;
    if (dst->nthreads > 0) omp_set_num_threads(dst->nthreads);

#pragma omp parallel for reduction(+:c_closest,c_shadow,c_hits,c_nodes,c_tris)
    for (int32_t y = 0; y < height; y++) {
        for (int32_t x = 0; x < width; x++) {
            v3 col(0); uint32_t cnt = 0;
            int32_t idx = y * width + x;
            PathState path;     // path_host_.Clear() zeroes contrib/attrib each frame (pt_params.h:101-119)
            path.samples = 0;
            Ray ray; ShadowRay shadow_ray;
            PathCounters pc;
            for (uint32_t i = 0; i < samples; i++) {
                const uint32_t rnd = seeds[idx % n_seeds];
                GeneratePath(ray, x, y, (int32_t)i, dst->frame, path, *camera, rnd);
                path.contrib = v3(0);
                radiance(path, ray, shadow_ray, x, y, width, height, ctxt, *camera, maxDepth, rrDepth, count ? &pc : nullptr);
                if (isInvalidColor(path.contrib)) continue;
                col += path.contrib;
                cnt++;
                if (path.is_terminated) break;          // pathtracing.cpp:350-352
            }
            col /= (float)cnt;
            v4 v(col, 1);
            atn_vec4& cur = film[idx];
            if (dst->progressive) {
                float n = static_cast<float>(static_cast<int32_t>(cur.w));
                v4 c(cur.x, cur.y, cur.z, cur.w);
                c = n * c + v;
                float d = n + 1;
                cur.x = c.x / d; cur.y = c.y / d; cur.z = c.z / d;
                cur.w = n + 1;
            }
            else {
                cur.x = v.x; cur.y = v.y; cur.z = v.z; cur.w = v.w;
            }
            c_closest += pc.closest_rays; c_shadow += pc.shadow_rays; c_hits += pc.hits;
            c_nodes += pc.trav.nodes; c_tris += pc.trav.tris;
            if (cost_out) { cost_out[2 * (size_t)idx] = (uint32_t)pc.trav.nodes; cost_out[2 * (size_t)idx + 1] = (uint32_t)pc.trav.tris; }
        }
    }
    if (counters_out) {
        counters_out[0] = c_closest; counters_out[1] = c_shadow; counters_out[2] = c_hits;
        counters_out[3] = c_nodes; counters_out[4] = c_tris;
    }
}

void orc_render(const atn_scene_desc* scene, const atn_camera_param* camera,
    const uint32_t* seeds, uint32_t n_seeds, const orc_destination* dst, atn_vec4* film,
    uint64_t* counters_out)
{
    orc_render_cost(scene, camera, seeds, n_seeds, dst, film, counters_out, nullptr);
}

int orc_num_procs() { return omp_get_num_procs(); }

// ---------------------------------------------------------------------------------------------------
// The shade stage, one vertex at a time: the twin of atn_shade_stage (include/aten_amd.h).
// ---------------------------------------------------------------------------------------------------
static const uint32_t kFlagTerminated = 1u, kFlagSingular = 2u, kFlagHit = 4u, kFlagLastSpecular = 8u;
// category bits of orc_shade_stage (tests/shade_vertices.py names them in this order)
enum : uint32_t {
    CAT_MISS_B0 = 1u << 0, CAT_MISS_DEEP = 1u << 1, CAT_MISS_B1_SINGULAR = 1u << 2,
    CAT_EMIT_FRONT_B0 = 1u << 3, CAT_EMIT_FRONT_DEEP = 1u << 4, CAT_EMIT_BACK = 1u << 5, CAT_EMIT_NO_LIGHT = 1u << 6,
    CAT_TOON_FIRST = 1u << 7, CAT_TOON_DEEP = 1u << 8,
    CAT_NO_NEE = 1u << 9, CAT_BACKFACE_OPAQUE = 1u << 10, CAT_NORMAL_MAP = 1u << 11, CAT_CARPAINT = 1u << 12, CAT_MTRL_NEG = 1u << 13,
    CAT_STENCIL_ALWAYS = 1u << 14,
    CAT_NEE_POINT = 1u << 15, CAT_NEE_SPOT = 1u << 16, CAT_NEE_DIRECTION = 1u << 17, CAT_NEE_AREA = 1u << 18, CAT_NEE_IBL = 1u << 19,
    CAT_NEE_ONE_LIGHT = 1u << 20, CAT_NEE_MANY_LIGHTS = 1u << 21, CAT_NEE_INVALID = 1u << 22,
    CAT_RR_SURVIVED = 1u << 23, CAT_RR_LOST = 1u << 24, CAT_RR_ZERO = 1u << 25,
    CAT_BSDF_REJECTED = 1u << 26, CAT_LAST_VERTEX = 1u << 27
};

static void path_from_vertex(PathState& path, Ray& ray, const atn_shade_vertex& v, const uint32_t* seeds, uint32_t n_seeds,
    uint32_t frame, int32_t sample, int32_t width)
{
    path.throughput = ld3(v.throughput); path.pdfb = v.pdfb; path.contrib = ld3(v.contrib);
    path.is_terminated = (v.flags & kFlagTerminated) != 0; path.is_singular = (v.flags & kFlagSingular) != 0;
    path.screen_space_x = v.pixel % width; path.screen_space_y = v.pixel / width;
    // GeneratePath's sampler (pathtracing_impl.h:75-81) at the record's dimension
    const uint32_t rnd = seeds[(uint32_t)v.pixel % n_seeds];
    const uint32_t fs = frame + (uint32_t)sample;
    path.sampler.init(fs % (CMJ::CMJ_DIM * CMJ::CMJ_DIM), v.dimension, rnd * 0x1fe3434f * ((fs + 133 * rnd) / (CMJ::CMJ_DIM * CMJ::CMJ_DIM)));
    ray.org = ld3(v.org); ray.dir = ld3(v.dir);      // (as stored: no constructor, nothing re-normalised)
}

// PathTracing::shade / ShadeMiss once per record (pathtracing.cpp:91-236, pathtracing_impl.h:112-176), called as PathTracing::radiance
// calls them, and what the NEXT stages can observe afterwards (atn_shade_result).  Nothing of the formulas is restated: the hit record
// is completed from the triangle as the traversal fills it, the state goes in, shade runs, the state comes out.  What the reference
// computes but nobody reads is NOT reported and left zero: the shadow ray of a path that ended in this vertex (HitShadowRay returns
// before it looks at it), the next ray, pdf, throughput and sampler position of a path that does not go on.
// cat_out [n] (optional): the branch taken, CAT_* bits.  margins_out [2 n] (optional): per record {the smallest distance from its
// threshold, in ulps, of a decision that rests on a libm result; the same of the decisions that do not} (orc_pt.h, DecisionLog).
// Returns 0, or -1 for a null pointer, a bad call, a pixel outside the frame, a record that is already terminated, or a hit record
// that names no object / triangle of the scene.
int orc_shade_stage(const atn_scene_desc* scene, const atn_camera_param* camera, const uint32_t* seeds, uint32_t n_seeds,
    const atn_shade_call* call, const atn_shade_vertex* in, uint32_t n, atn_shade_result* out, uint32_t* cat_out, float* margins_out)
{
    if (!scene || !camera || !seeds || !n_seeds || !call) return -1;
    if (call->width <= 0 || call->height <= 0 || call->max_depth <= 0 || call->bounce < 0 || call->bounce >= call->max_depth) return -1;
    if ((call->flavour != 0 && call->flavour != 1) || call->chunk_items < 0 || call->chunk_items > 4) return -1;
    const bool svgf_flavour = call->flavour == 1;
    if (n == 0) return 0;
    if (!in || !out) return -1;
    Scene ctxt(scene);
    for (uint32_t i = 0; i < n; i++) {
        if (in[i].pixel < 0 || (int64_t)in[i].pixel >= (int64_t)call->width * call->height || (in[i].flags & kFlagTerminated)) return -1;
        if (in[i].flags & ~(kFlagTerminated | kFlagSingular | kFlagHit | kFlagLastSpecular)) return -1;
        // (the same refusals as atn_shade_stage's: ids inside the scene, barycentrics finite and within [-1, 2])
        if (in[i].objid >= 0 && ((uint32_t)in[i].objid >= scene->n_objects || in[i].tri_id < 0 || (uint32_t)in[i].tri_id >= scene->n_triangles
                                 || !(in[i].a >= -1.0F && in[i].a <= 2.0F && in[i].b >= -1.0F && in[i].b <= 2.0F))) return -1;
    }
    if (sampling_options().ibl_importance && ctxt.cfg().bg.envmap_tex_idx >= 0 && ctxt.cfg().bg.enable_env_map)
        IBL_preCompute(sampling_options(), ctxt);
    int32_t rrDepth = call->rr_depth;
    if (rrDepth > call->max_depth) rrDepth = call->max_depth - 1;      // pathtracing.cpp:282-284
    const int32_t bounce = call->bounce;
    // flavour "svgf": SVGFRenderer::Shade / ShadeMiss with AOV spans (svgf.cpp:89-229) under the frame's W2C.  The path's
    // last_hit_mtrl_idx is carried as one flag bit -- "the last hit's material is Specular", all Shade asks of it -- so a set bit
    // stands for the scene's first Specular material (refused where the scene has none).
    svgf::Matrices mtxs;
    mtxs.Reset(*camera);
    const m4 W2C = mtxs.GetW2C();
    int32_t specular_idx = -1;
    for (uint32_t k = 0; k < scene->n_materials && specular_idx < 0; k++) if (scene->materials[k].type == ATN_MTRL_SPECULAR) specular_idx = (int32_t)k;
    if (svgf_flavour && specular_idx < 0)
        for (uint32_t i = 0; i < n; i++) if (in[i].flags & kFlagLastSpecular) return -1;
    const uint32_t kUnwritten = 0x7fa5a5a5u;        // every component of an AOV texel nobody wrote (a NaN pattern, compared as bits)
#pragma omp parallel for
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const atn_shade_vertex& v = in[i];
        PathState path; Ray ray; ShadowRay shadow_ray;
        path_from_vertex(path, ray, v, seeds, n_seeds, call->frame, call->sample, call->width);
        shadow_ray.targetLightId = 0xffffffffu;
        v4 aov[3];
        for (v4& t : aov) { float f; std::memcpy(&f, &kUnwritten, 4); t = v4(f, f, f, f); }
        if (svgf_flavour) path.last_hit_mtrl_idx = (v.flags & kFlagLastSpecular) ? specular_idx : -1;
        DecisionLog log;
        decision_log() = &log;
        const bool is_hit = v.objid >= 0;
        uint32_t cat = 0;
        uint32_t lbits = 0;
        path.isHit = false;
        if (is_hit) {
            Isect isect;
            const auto& prim = ctxt.GetTriangle((uint32_t)v.tri_id);
            isect.objid = v.objid; isect.tri_id = v.tri_id; isect.a = v.a; isect.b = v.b;
            isect.mtrlid = (int32_t)prim.mtrlid; isect.meshid = (int32_t)prim.mesh_id;
            path.isHit = true;
            const Ray ray_in = ray;
            if (svgf_flavour) svgf::Shade(path, ctxt, ray, shadow_ray, isect, rrDepth, bounce, W2C, aov[0], aov[1], aov[2], nullptr);
            else shade(path, ctxt, ray, shadow_ray, isect, rrDepth, bounce, nullptr);
            const bool stencil_always = isect.mtrlid >= 0 && ctxt.GetMaterial(isect.mtrlid).stencil_type == 1;     // pathtracing.cpp:59-66
            lbits = shadow_ray.targetLightId | (stencil_always ? 0x40000000u : 0u);
            // ---- the branch taken, from the material and the log (labels only: no output depends on them)
            atn_material_param m;
            FillMaterial(m, ctxt, isect.mtrlid);
            HitRec rec;
            evaluate_hit_result(rec, ctxt.GetObject((uint32_t)v.objid), ctxt, ray_in, isect);
            const bool back = dot(rec.normal, -ray_in.dir) < 0.0F;
            const bool toon = m.type == ATN_MTRL_TOON || m.type == ATN_MTRL_STYLIZED_BRDF;
            if (isect.mtrlid < 0) cat |= CAT_MTRL_NEG;
            if (stencil_always) cat |= CAT_STENCIL_ALWAYS;
            if (m.type == ATN_MTRL_EMISSIVE) {
                if (back) cat |= CAT_EMIT_BACK;
                else cat |= bounce == 0 ? CAT_EMIT_FRONT_B0 : CAT_EMIT_FRONT_DEEP;
                if (ctxt.GetObject((uint32_t)v.objid).light_id < 0) cat |= CAT_EMIT_NO_LIGHT;
            }
            if (toon) cat |= bounce == 0 ? CAT_TOON_FIRST : CAT_TOON_DEEP;
            const bool reached_nee = log.roulette != 0 || log.nee != 0 || log.bsdf_rejected != 0 || shadow_ray.targetLightId != 0xffffffffu
                                     || path.sampler.m_dimension != v.dimension || !path.is_terminated;
            if (reached_nee) {
                if (!toon && (attr_singular(m) || attr_translucent(m))) cat |= CAT_NO_NEE;
                if (!attr_translucent(m) && back) cat |= CAT_BACKFACE_OPAQUE;
                if (m.normalMap >= 0) cat |= CAT_NORMAL_MAP;
                if (m.type == ATN_MTRL_CARPAINT) cat |= CAT_CARPAINT;
                if (log.nee) {
                    const int32_t lt = ctxt.GetLight(shadow_ray.targetLightId).type;
                    cat |= lt == ATN_LIGHT_POINT ? CAT_NEE_POINT : lt == ATN_LIGHT_SPOT ? CAT_NEE_SPOT : lt == ATN_LIGHT_DIRECTION ? CAT_NEE_DIRECTION
                         : lt == ATN_LIGHT_AREA ? CAT_NEE_AREA : CAT_NEE_IBL;
                    cat |= ctxt.GetLightNum() == 1 ? CAT_NEE_ONE_LIGHT : CAT_NEE_MANY_LIGHTS;
                    if (log.nee == 2) cat |= CAT_NEE_INVALID;
                }
                if (log.roulette == 1) cat |= CAT_RR_SURVIVED;
                if (log.roulette == 2) cat |= CAT_RR_LOST;
                if (log.roulette == 3) cat |= CAT_RR_ZERO;
                if (log.bsdf_rejected) cat |= CAT_BSDF_REJECTED;
                if (!path.is_terminated && bounce + 1 == call->max_depth) cat |= CAT_LAST_VERTEX;
            }
        }
        else {
            if (svgf_flavour) svgf::ShadeMissAov(path.screen_space_x, path.screen_space_y, call->width, call->height, bounce, ctxt, *camera, path, ray, aov[0], aov[1], aov[2]);
            else ShadeMiss(path.screen_space_x, path.screen_space_y, call->width, call->height, bounce, ctxt, *camera, path, ray);
            cat |= bounce == 0 ? CAT_MISS_B0 : (bounce == 1 && (v.flags & kFlagSingular)) ? CAT_MISS_B1_SINGULAR : CAT_MISS_DEEP;
        }
        decision_log() = nullptr;

        atn_shade_result& o = out[i];
        std::memset(&o, 0, sizeof(o));
        o.flags = (v.flags & ~(kFlagTerminated | kFlagSingular | kFlagHit)) | (path.is_terminated ? kFlagTerminated : 0u)
                | (path.is_singular ? kFlagSingular : 0u) | (path.isHit ? kFlagHit : 0u);
        if (svgf_flavour) {
            const int32_t last = path.last_hit_mtrl_idx;        // (PrepareForNextBounce stores mtrl.id where the path goes on, pathtracing_impl.h:739)
            const bool spec = last >= 0 && (uint32_t)last < scene->n_materials && scene->materials[last].type == ATN_MTRL_SPECULAR;
            o.flags = (o.flags & ~kFlagLastSpecular) | (spec ? kFlagLastSpecular : 0u);
            float* dst[3] = { o.aov_nd, o.aov_am, o.aov_primary };
            for (int k = 0; k < 3; k++) {
                const float c[4] = { aov[k].x, aov[k].y, aov[k].z, aov[k].w };
                uint32_t b[4]; std::memcpy(b, c, 16);
                if (b[0] != kUnwritten || b[1] != kUnwritten || b[2] != kUnwritten || b[3] != kUnwritten) { o.aov_written |= 1u << k; std::memcpy(dst[k], c, 16); }
            }
        }
        o.contrib[0] = path.contrib.x; o.contrib[1] = path.contrib.y; o.contrib[2] = path.contrib.z;
        o.goes_on = (is_hit && !path.is_terminated && bounce + 1 < call->max_depth) ? 1u : 0u;      // radiance's `willContinue` and its loop bound
        o.has_shadow = (is_hit && !path.is_terminated && shadow_ray.isActive) ? 1u : 0u;            // HitShadowRay's two early returns
        if (o.goes_on) {
            o.dimension = path.sampler.m_dimension; o.pdfb = path.pdfb;
            o.org[0] = ray.org.x; o.org[1] = ray.org.y; o.org[2] = ray.org.z;
            o.dir[0] = ray.dir.x; o.dir[1] = ray.dir.y; o.dir[2] = ray.dir.z;
            o.throughput[0] = path.throughput.x; o.throughput[1] = path.throughput.y; o.throughput[2] = path.throughput.z;
        }
        if (o.has_shadow) {
            o.light_bits = lbits; o.sh_c_w = lbits; o.sh_dist = shadow_ray.distToLight;
            o.sh_o[0] = shadow_ray.rayorg.x; o.sh_o[1] = shadow_ray.rayorg.y; o.sh_o[2] = shadow_ray.rayorg.z;
            o.sh_d[0] = shadow_ray.raydir.x; o.sh_d[1] = shadow_ray.raydir.y; o.sh_d[2] = shadow_ray.raydir.z;
            o.sh_c[0] = shadow_ray.lightcontrib.x; o.sh_c[1] = shadow_ray.lightcontrib.y; o.sh_c[2] = shadow_ray.lightcontrib.z;
        }
        if (cat_out) cat_out[i] = cat;
        if (margins_out) { margins_out[2 * i] = log.min_libm_ulps; margins_out[2 * i + 1] = log.min_exact_ulps; }
    }
    return 0;
}

// PathTracing::radiance (pathtracing.cpp:22-89) over one sample of a frame, as orc_render runs it, with an observer: one record per
// (pixel, bounce) in the order visited (pixels in raster order, a pixel's bounces ascending) -- what shade / ShadeMiss START from at
// every depth.  bounce_out [capacity]: the record's depth.  film (optional): the sample's Path.contrib per pixel, xyz + 1.
// Returns the number of records (at most width * height * maxDepth), or -1 when `capacity` is too small.
int64_t orc_record_vertices(const atn_scene_desc* scene, const atn_camera_param* camera, const uint32_t* seeds, uint32_t n_seeds,
    const orc_destination* dst, int32_t sample, atn_shade_vertex* out, int32_t* bounce_out, uint64_t capacity, atn_vec4* contrib_out)
{
    struct Recorder : VertexObserver {
        std::vector<atn_shade_vertex>* v; std::vector<int32_t>* b; int32_t pixel;
        void vertex(int32_t depth, const PathState& path, const Ray& ray, const Isect& isect, bool is_hit) override
        {
            atn_shade_vertex r{};
            r.org[0] = ray.org.x; r.org[1] = ray.org.y; r.org[2] = ray.org.z; r.pdfb = path.pdfb;
            r.dir[0] = ray.dir.x; r.dir[1] = ray.dir.y; r.dir[2] = ray.dir.z;
            r.flags = (path.is_terminated ? kFlagTerminated : 0u) | (path.is_singular ? kFlagSingular : 0u);
            r.throughput[0] = path.throughput.x; r.throughput[1] = path.throughput.y; r.throughput[2] = path.throughput.z;
            r.dimension = path.sampler.m_dimension;
            r.contrib[0] = path.contrib.x; r.contrib[1] = path.contrib.y; r.contrib[2] = path.contrib.z;
            r.objid = is_hit ? isect.objid : -1; r.a = is_hit ? isect.a : 0.0F; r.b = is_hit ? isect.b : 0.0F; r.tri_id = is_hit ? isect.tri_id : -1;
            r.pixel = pixel;
            v->push_back(r); b->push_back(depth);
        }
    };
    Scene ctxt(scene);
    if (sampling_options().ibl_importance && ctxt.cfg().bg.envmap_tex_idx >= 0 && ctxt.cfg().bg.enable_env_map)
        IBL_preCompute(sampling_options(), ctxt);
    const int32_t width = dst->width, height = dst->height;
    int32_t maxDepth = dst->maxDepth, rrDepth = dst->russianRouletteDepth;
    if (rrDepth > maxDepth) rrDepth = maxDepth - 1;
    std::vector<std::vector<atn_shade_vertex>> rows(height);
    std::vector<std::vector<int32_t>> row_b(height);
#pragma omp parallel for
    for (int32_t y = 0; y < height; y++) {
        Recorder rec; rec.v = &rows[y]; rec.b = &row_b[y];
        for (int32_t x = 0; x < width; x++) {
            const int32_t idx = y * width + x;
            PathState path; path.samples = 0;
            Ray ray; ShadowRay shadow_ray;
            GeneratePath(ray, x, y, sample, dst->frame, path, *camera, seeds[idx % n_seeds]);
            path.contrib = v3(0);
            rec.pixel = idx;
            radiance(path, ray, shadow_ray, x, y, width, height, ctxt, *camera, maxDepth, rrDepth, nullptr, &rec);
            if (contrib_out) { contrib_out[idx].x = path.contrib.x; contrib_out[idx].y = path.contrib.y; contrib_out[idx].z = path.contrib.z; contrib_out[idx].w = 1.0F; }
        }
    }
    uint64_t total = 0;
    for (int32_t y = 0; y < height; y++) total += rows[y].size();
    if (total > capacity) return -1;
    uint64_t k = 0;
    for (int32_t y = 0; y < height; y++)
        for (size_t i = 0; i < rows[y].size(); i++, k++) { out[k] = rows[y][i]; bounce_out[k] = row_b[y][i]; }
    return (int64_t)total;
}

// ---------------------------------------------------------------------------------------------------
// SVGF (next tier): aten::SVGFRenderer, src/libaten/renderer/svgf/svgf.cpp:412-637
// ---------------------------------------------------------------------------------------------------
void* orc_svgf_create() { return new svgf::Params(); }
void orc_svgf_destroy(void* h) { delete static_cast<svgf::Params*>(h); }
void orc_svgf_set_atrous_iterations(void* h, int32_t n) { static_cast<svgf::Params*>(h)->atrous_iter_cnt = n; }
void orc_svgf_set_dilate_temporal_weight(void* h, int32_t on) { static_cast<svgf::Params*>(h)->dilate_temporal_weight = on; }

// aten::FillBasicAOVs / FillBasicAOVsIfHitMiss (renderer/aov.h:158-198) on their own, for the reference's known answers
// (aten_unittest/aov_host_buffer.cpp:73-132).  w2c: 16 floats, row-major (aten::mat4)
void orc_fill_basic_aovs(const float* normal, const float* p, const float* w2c, const float* albedo, int32_t meshid, float* out_nd, float* out_am)
{
    m4 m;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) m.m[r][c] = w2c[4 * r + c];
    v4 nd, am;
    svgf::FillBasicAOVs(nd, v3(normal[0], normal[1], normal[2]), v3(p[0], p[1], p[2]), m, am, v4(albedo[0], albedo[1], albedo[2], albedo[3]), meshid);
    out_nd[0] = nd.x; out_nd[1] = nd.y; out_nd[2] = nd.z; out_nd[3] = nd.w;
    out_am[0] = am.x; out_am[1] = am.y; out_am[2] = am.z; out_am[3] = am.w;
}
void orc_fill_basic_aovs_if_hit_miss(const float* bg, float* out_nd, float* out_am)
{
    v4 nd, am;
    svgf::FillBasicAOVsIfHitMiss(nd, am, v4(bg[0], bg[1], bg[2], bg[3]));
    out_nd[0] = nd.x; out_nd[1] = nd.y; out_nd[2] = nd.z; out_nd[3] = nd.w;
    out_am[0] = am.x; out_am[1] = am.y; out_am[2] = am.z; out_am[3] = am.w;
}

// SVGFRenderer::SetMotionDepthBuffer (svgf.cpp:441-450): vec4 {motion.xy in screen fractions, depth, 1} per pixel
void orc_svgf_set_motion_depth(void* h, const atn_vec4* md, uint32_t n)
{
    auto* p = static_cast<svgf::Params*>(h);
    p->motion_depth_buffer.resize(n);
    for (uint32_t i = 0; i < n; i++) p->motion_depth_buffer[i] = v4(md[i].x, md[i].y, md[i].z, md[i].w);
}

// which: 0-3 current AOVs, 4-7 previous AOVs, 8 temporary colour, 9 motion/depth, 10 primary hit position,
// 11/12 the two a-trous ping-pong buffers
int orc_svgf_get_buffer(void* h, int32_t which, atn_vec4* out)
{
    auto* p = static_cast<svgf::Params*>(h);
    const std::vector<v4>* b = nullptr;
    if (which >= 0 && which < 4) b = &p->cur(which);
    else if (which < 8) b = &p->prev(which - 4);
    else if (which == 8) b = &p->temporary_color_buffer;
    else if (which == 9) b = &p->motion_depth_buffer;
    else if (which == 10) b = &p->primary_position;
    else if (which == 11 || which == 12) b = &p->atrous_clr_variance[which - 11];
    if (!b) return -1;
    for (size_t i = 0; i < b->size(); i++) { out[i].x = (*b)[i].x; out[i].y = (*b)[i].y; out[i].z = (*b)[i].z; out[i].w = (*b)[i].w; }
    return (int)b->size();
}

// The inverse of orc_svgf_get_buffer (same `which`): gives the oracle the history, or any other plane, a test wants both sides
// to start from.  Creates the buffers of a w x h frame first where they do not exist yet (SVGFParams::InitBuffers).
int orc_svgf_set_buffer(void* h, int32_t which, int32_t width, int32_t height, const atn_vec4* in)
{
    auto* p = static_cast<svgf::Params*>(h);
    if (p->width > 0 && (p->width != width || p->height != height)) return -1;      // a renderer keeps one frame size
    p->InitBuffers(width, height);
    const size_t n = (size_t)width * height;
    std::vector<v4>* b = nullptr;
    if (which >= 0 && which < 4) b = &p->cur(which);
    else if (which < 8) b = &p->prev(which - 4);
    else if (which == 8) b = &p->temporary_color_buffer;
    else if (which == 9) { p->motion_depth_buffer.resize(n); b = &p->motion_depth_buffer; }
    else if (which == 10) b = &p->primary_position;
    else if (which == 11 || which == 12) b = &p->atrous_clr_variance[which - 11];
    if (!b || b->size() != n) return -1;
    for (size_t i = 0; i < n; i++) (*b)[i] = v4(in[i].x, in[i].y, in[i].z, in[i].w);
    return (int)n;
}

// The filter half of SVGFRenderer::OnRender (svgf.cpp:515-637) on the planes as they stand in P: PrepareForDenoise, the motion
// pass, temporal reprojection, the optional weight dilation, variance estimation, the a-trous levels and the copy-back.
// `contribs`: Path.contrib as vec4 (contrib.xyz, samples) per pixel.  Shared by orc_svgf_render (behind its path pass) and
// orc_svgf_denoise (on a caller's planes).
static void svgf_filter_passes(svgf::Params& P, const atn_camera_param* camera, const orc_destination* dst, int32_t compute_motion,
    const std::vector<v4>& contribs, atn_vec4* film, atn_vec4* stage_out)
{
    const int32_t width = dst->width, height = dst->height;
    const size_t n = (size_t)width * height;
    const m4 W2C = P.mtxs.GetW2C();
    const m4 prevW2C = svgf::mul(P.mtxs.V2C, P.mtxs.PrevW2V);
    auto put = [&](int stage, int32_t idx, const v4& v) {
        if (stage_out && stage < 3) { atn_vec4& o = stage_out[(size_t)stage * n + idx]; o.x = v.x; o.y = v.y; o.z = v.z; o.w = v.w; }
        atn_vec4& o = film[idx]; o.x = v.x; o.y = v.y; o.z = v.z; o.w = v.w;
    };

#pragma omp parallel for
    for (int32_t idx = 0; idx < (int32_t)n; idx++) {
        // PrepareForDenoise (svgf_impl.h:119-144)
        const v4 c = contribs[idx];
        v4 contrib = c;
        svgf::operator/=(contrib, c.w);
        if (dst->frame == 0) {
            float lum = luminance(contrib.x, contrib.y, contrib.z);
            v4& mt = P.cur(svgf::MomentTemporalWeight)[idx];
            mt.x += lum * lum; mt.y += lum; mt.z += 1;
            v4& cv = P.cur(svgf::ColorVariance)[idx];
            cv = v4(contrib.x, contrib.y, contrib.z, cv.w);
        }
        P.temporary_color_buffer[idx] = c;
        put(0, idx, v4(c.x, c.y, c.z, 1));      // Film::put(x, y, vec3) -> vec4(v, 1)
    }

    if (compute_motion) {
        P.motion_depth_buffer.resize(n);
#pragma omp parallel for
        for (int32_t i = 0; i < (int32_t)n; i++) P.motion_depth_buffer[i] = svgf::ComputeMotionDepth(P.primary_position[i], W2C, prevW2C);
    }

#pragma omp parallel for
    for (int32_t y = 0; y < height; y++) {
        for (int32_t x = 0; x < width; x++) {
            int32_t idx = y * width + x;
            v4 temporal_projected_clr;
            if (dst->frame > 0) temporal_projected_clr = svgf::TemporalReprojection(x, y, width, height, 0.98f, 0.05f, contribs[idx], P);
            else temporal_projected_clr = v4(contribs[idx].x, contribs[idx].y, contribs[idx].z, 1.0f);   // vec4() then operator=(vec3): w stays 1
            put(1, idx, temporal_projected_clr);
        }
    }

    if (P.dilate_temporal_weight && dst->frame > 0) {
        const std::vector<v4> mt_in = P.cur(svgf::MomentTemporalWeight);
        std::vector<v4>& mt = P.cur(svgf::MomentTemporalWeight);
#pragma omp parallel for
        for (int32_t y = 0; y < height; y++)
            for (int32_t x = 0; x < width; x++) {
                float w;
                if (svgf::RecomputeTemporalWeightFromSurroundingPixels(x, y, width, height, P.cur(svgf::AlbedoMeshId), mt_in, w))
                    mt[y * width + x].w = w;
            }
    }

    // Camera::ComputeScreenDistance (camera.h:216-221): tan() of half the vertical fov IN DEGREES, as written
    const float camera_distance = height / (2.0f * std::tan(0.5f * camera->vfov));
    {
        const std::vector<v4> cv_in = P.cur(svgf::ColorVariance);
#pragma omp parallel for
        for (int32_t y = 0; y < height; y++) {
            for (int32_t x = 0; x < width; x++) {
                put(2, y * width + x, svgf::EstimateVariance(x, y, width, height, camera_distance, cv_in, P));
            }
        }
    }

    for (int32_t i = 0; i < P.atrous_iter_cnt; i++) {
#pragma omp parallel for
        for (int32_t y = 0; y < height; y++) {
            for (int32_t x = 0; x < width; x++) {
                v4 out;
                if (svgf::AtrousFilter(i, x, y, width, height, camera_distance, P, &out)) put(3, y * width + x, out);
            }
        }
    }

    // CopyFromTeporaryColorBufferToAov: CopyVectorBuffer<3> (svgf.cpp:402-410)
    {
        auto& cv = P.cur(svgf::ColorVariance);
        for (size_t i = 0; i < n; i++) { cv[i].z = P.temporary_color_buffer[i].z; cv[i].y = P.temporary_color_buffer[i].y; cv[i].x = P.temporary_color_buffer[i].x; }
    }
    P.curr_aov_pos = 1 - P.curr_aov_pos;
}

// SVGFRenderer::OnRender (svgf.cpp:452-637).  `film` receives what dst.buffer holds when OnRender returns (Film::put,
// film.cpp:33-45): the last a-trous iteration's albedo-multiplied colour.  `stage_out` (may be null): 3 x vec4[w*h] =
// the values put after the path pass, after the temporal pass and after the variance pass.
// compute_motion != 0: fill motion_depth_buffer from the primary hits (ComputeMotionDepth) instead of an external buffer.
void orc_svgf_render(void* h, const atn_scene_desc* scene, const atn_camera_param* camera,
    const uint32_t* seeds, uint32_t n_seeds, const orc_destination* dst, int32_t compute_motion,
    atn_vec4* film, atn_vec4* stage_out)
{
    auto& P = *static_cast<svgf::Params*>(h);
    Scene ctxt(scene);
    const int32_t width = dst->width, height = dst->height;
    const uint32_t samples = (uint32_t)dst->sample;
    int32_t maxDepth = dst->maxDepth;
    int32_t rrDepth = dst->russianRouletteDepth;
    if (rrDepth > maxDepth) rrDepth = maxDepth - 1;         // svgf.cpp:423-425
    P.InitBuffers(width, height);
    P.mtxs.Reset(*camera);
    const m4 W2C = P.mtxs.GetW2C();
    const size_t n = (size_t)width * height;
    std::vector<v4> contribs(n);
    if (dst->nthreads > 0) omp_set_num_threads(dst->nthreads);

#pragma omp parallel for
    for (int32_t y = 0; y < height; y++) {
        for (int32_t x = 0; x < width; x++) {
            int32_t idx = y * width + x;
            PathState path;             // path_host_.Clear(): contrib/attrib/throughput zeroed every frame
            path.samples = 0;
            Ray ray; ShadowRay shadow_ray;
            for (uint32_t i = 0; i < samples; i++) {
                const uint32_t rnd = seeds[idx % n_seeds];
                GeneratePath(ray, x, y, (int32_t)i, dst->frame, path, *camera, rnd);
                path.contrib = v3(0);
                svgf::ExecRendering(path, ray, shadow_ray, x, y, width, height, ctxt, *camera, maxDepth, rrDepth, W2C,
                    P.cur(svgf::NormalDepth)[idx], P.cur(svgf::AlbedoMeshId)[idx], P.primary_position[idx], nullptr);
                if (isInvalidColor(path.contrib)) continue;
                if (path.is_terminated) break;
            }
            contribs[idx] = v4(path.contrib, path.samples);
        }
    }
    svgf_filter_passes(P, camera, dst, compute_motion, contribs, film, stage_out);
}

// The filter half alone on planes the caller passes: the twin of atn_svgf_upload (contribs, normal_depth, albedo_meshid,
// primary_position into the current set) followed by atn_svgf_denoise -- buffers initialised like a fresh renderer's where they
// do not exist yet, the camera matrices advanced, then every pass of svgf_filter_passes (frame 0: PrepareForDenoise accumulates
// into the initial (0, 0, 0, 1) texels).  Outputs as orc_svgf_render's.
void orc_svgf_denoise(void* h, const atn_camera_param* camera, const orc_destination* dst, int32_t compute_motion,
    const atn_vec4* contribs_in, const atn_vec4* normal_depth, const atn_vec4* albedo_meshid, const atn_vec4* primary_position,
    atn_vec4* film, atn_vec4* stage_out)
{
    auto& P = *static_cast<svgf::Params*>(h);
    P.InitBuffers(dst->width, dst->height);
    P.mtxs.Reset(*camera);
    const size_t n = (size_t)dst->width * dst->height;
    std::vector<v4> contribs(n);
    auto& nd = P.cur(svgf::NormalDepth); auto& am = P.cur(svgf::AlbedoMeshId);
    for (size_t i = 0; i < n; i++) {
        contribs[i] = v4(contribs_in[i].x, contribs_in[i].y, contribs_in[i].z, contribs_in[i].w);
        nd[i] = v4(normal_depth[i].x, normal_depth[i].y, normal_depth[i].z, normal_depth[i].w);
        am[i] = v4(albedo_meshid[i].x, albedo_meshid[i].y, albedo_meshid[i].z, albedo_meshid[i].w);
        P.primary_position[i] = v4(primary_position[i].x, primary_position[i].y, primary_position[i].z, primary_position[i].w);
    }
    if (dst->nthreads > 0) omp_set_num_threads(dst->nthreads);
    svgf_filter_passes(P, camera, dst, compute_motion, contribs, film, stage_out);
}

// idaten::LBVHBuilder::build with threadedBvhNodes (LBVHBuilder.cu:812-833): the node array in the reference's order
int orc_lbvh_build(const atn_triangle_param* tris, uint32_t n, int32_t tri_id_offset, const float* bmin, const float* bmax,
                   const atn_vec4* vtx_pos, int32_t vtx_offset, atn_bvh_node* out_nodes, uint32_t* out_codes, uint32_t* out_indices)
{
    return orc::lbvh::build(tris, n, tri_id_offset, bmin, bmax, vtx_pos, vtx_offset, out_nodes, out_codes, out_indices) ? 0 : -1;
}

// buildTree alone on given SORTED keys (LBVHBuilder.cu:299-350): left / right / parent of the 2 n - 1 nodes
int orc_lbvh_hierarchy(const uint32_t* sorted_keys, uint32_t n, int32_t* left, int32_t* right, int32_t* parent)
{
    if (n < 2) return -1;
    std::vector<orc::lbvh::Node> nodes;
    orc::lbvh::build_tree(sorted_keys, n, nodes);
    for (size_t i = 0; i < nodes.size(); i++) { left[i] = nodes[i].left; right[i] = nodes[i].right; parent[i] = nodes[i].parent; }
    return 0;
}

} // extern "C"
