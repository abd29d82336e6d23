/*
 * NPR ORACLE -- TEST INFRASTRUCTURE ONLY (tests/npr_oracle.py compiles it; the product never loads it).
 *
 * A CPU restatement of the reference's NPR path tracer with feature lines -- aten::NprPathTracer::radiance_with_feature_line and
 * RenderPerSample (src/libaten/renderer/npr/npr.cpp:101-200,487-536), the per-path arithmetic of npr_impl.h and the geometry of
 * feature_line.h -- on top of the path-tracing oracle (oracle/orc_pt.h, read as it is), with the decisions of docs/NPR.md:
 *   one pass of the sample loop per frame (idaten::NPRPathTracing's shape), or, switched on, the CPU renderer's literal two-pass
 *   OnRender (npr.cpp:351-485: sample 0 of every pixel, then samples 0..spp-1 again, into a contribution sum never cleared).
 * AdvanceNPRPath (npr.cpp:202-282) changes nothing on the scenes the product accepts (no STENCIL material, no alpha blending with
 * alpha < 1, no CarPaint), so it is not restated.
 */
#include "../../oracle/orc_pt.h"
#include <omp.h>
#include <cmath>
#include <cstring>
#include <vector>

using namespace orc;

namespace {

constexpr int kRays = 8;    // SampleRayNum

struct FLConfig { uint8_t enabled; uint8_t pad[3]; float line_color[3]; float line_width, albedo_threshold, normal_threshold; };
static_assert(sizeof(FLConfig) == 28, "FeatureLineConfig");
struct FLMtrl { uint8_t enable; uint8_t pad[3]; int32_t metric_flag; };
static_assert(sizeof(FLMtrl) == 8, "FeatureLineMtrlConfig");
enum { kMesh = 1, kAlbedo = 2, kNormal = 4, kDepth = 8 };

FLMtrl mtrl_lines(const Scene& ctxt, int32_t id)
{
    FLMtrl f{};
    if (id >= 0 && (uint32_t)id < ctxt.d->n_materials) std::memcpy(&f, ctxt.GetMaterial((uint32_t)id).feature_line, sizeof(f));
    return f;
}

// FeatureLine::SampleRayDesc / Disc / SampleRayInfo (feature_line.h:52-86)
struct Desc { float u{ 0 }, v{ 0 }; bool is_terminated{ false }; v3 prev_ray_hit_pos, prev_ray_hit_nml; v3 ray_org, ray_dir; };
struct Disc { v3 center; float radius{ 0 }; v3 normal; float accumulated_distance{ 0 }; };
struct Info { Desc descs[kRays]; Disc disc; };

// ---- feature_line.h -----------------------------------------------------------------------------------------------------------
v3 HitPositionOnDisc(float u, float v, const Disc& disc)       // :279-305
{
    const v4 p = v4(u, v, 0, 1) * disc.radius;
    v3 t, b;
    GetTangentCoordinate(disc.normal, t, b);
    const v3& n = disc.normal;     // mat4(t, b, n): columns; applyXYZ
    v3 r(t.x * p.x + b.x * p.y + n.x * p.z, t.y * p.x + b.y * p.y + n.y * p.z, t.z * p.x + b.z * p.y + n.z * p.z);
    return v3(r.x + disc.center.x, r.y + disc.center.y, r.z + disc.center.z);
}
v4 ComputePlane(const v3& n, const v3& p) { const float d = -dot(n, p); return v4(n.x, n.y, n.z, d); }     // :313-324
bool RayHitPositionOnPlane(const v4& L, const Ray& ray, v3& pos)    // :333-371
{
    const v4 Q(ray.org, 1), V(ray.dir, 0);
    const float div = dot(L, V);
    if (div == 0) return false;
    float t = dot(L, Q);
    t = -t / div;
    pos = ray.org + t * ray.dir;
    return t >= 0;
}
Disc GenerateDisc(const Ray& q, float line_width, float pixel_width)     // :97-121
{
    const v4 plane = ComputePlane(-q.dir, q.org + q.dir);
    v3 pos;
    RayHitPositionOnPlane(plane, q, pos);
    Disc d;
    d.center = pos; d.normal = q.dir; d.radius = line_width * pixel_width;
    return d;
}
Disc DiscAtQueryRayHitPoint(const v3& p, const v3& dir, float prev_radius, float cur, float acc_without)     // :133-154
{
    Disc d;
    d.center = p;
    const float acc = acc_without + cur;
    d.radius = prev_radius * acc / acc_without;
    d.normal = -dir;
    d.accumulated_distance = acc_without;
    return d;
}
bool invalid3(const v3& v) { return std::isnan(v.x) || std::isnan(v.y) || std::isnan(v.z) || std::isinf(v.x) || std::isinf(v.y) || std::isinf(v.z); }
bool NextSampleRay(const Desc& desc, const Disc& prev, const Disc& next, Ray& out)     // :230-269
{
    const float face = dot(prev.normal, next.normal);
    const float u = face >= 0 ? desc.u : -desc.u;
    const v3 pos = HitPositionOnDisc(u, desc.v, next);
    v3 rd = pos - desc.prev_ray_hit_pos;
    rd = normalize(rd);
    if (dot(rd, desc.prev_ray_hit_nml) < 0) return false;
    const Ray r(desc.prev_ray_hit_pos, rd, desc.prev_ray_hit_nml);
    if (invalid3(r.dir)) return false;
    out = r;
    return true;
}
float ProjectPointOnRay(const v3& point, const Ray& ray, v3* on_ray)     // :381-410
{
    const v3 X = point - ray.org;
    v3 Y = dot(X, ray.dir) * ray.dir;
    Y += ray.org;
    if (on_ray) *on_ray = Y;
    return length(point - Y);
}
float DistanceOnRay(const v3& point, const Ray& ray) { v3 y; ProjectPointOnRay(point, ray, &y); return length(y - ray.org); }   // :419-427
bool IsInLineWidth(float w, const Ray& ray, const v3& point, float acc, float pixel_width)     // :621-645
{
    v3 y;
    const float len = ProjectPointOnRay(point, ray, &y);
    float dist = length(ray.org - y);
    dist = acc + dist;
    const float ws = dist * pixel_width * w;
    return len <= ws;
}
float DepthThreshold(const v3& p, float scale, const v3& pq_pos, const v3& nq, const v3& ps_pos, const v3& ns, float dq, float ds)    // :573-609
{
    const v3 p_q = pq_pos - p, p_s = ps_pos - p;
    const v3& n_closest = length(p_q) > length(p_s) ? ns : nq;
    const float max_depth = fmax_(dq, ds);
    const float div = std::fabs(dot(p_q, n_closest));
    if (div == 0.0F) return std::numeric_limits<float>::max();
    return scale * max_depth * length(p_s - p_q) / div;
}
bool EvaluateMetrics(const v3& p, const HitRec& q, const HitRec& s, const v4& aq, const v4& as, const FLConfig& cfg, int32_t flags,
                     float dq, float ds, float scale)     // :445-481
{
    const bool is_mesh = (flags & kMesh) ? q.meshid != s.meshid : false;
    const bool is_albedo = (flags & kAlbedo) ? std::fabs(luminance(aq.x, aq.y, aq.z) - luminance(as.x, as.y, as.z)) > cfg.albedo_threshold : false;
    const bool is_normal = (flags & kNormal) ? (1.0F - dot(q.normal, s.normal)) > cfg.normal_threshold : false;
    const bool is_depth = (flags & kDepth) ? std::fabs(dq - ds) > DepthThreshold(p, scale, q.p, q.normal, s.p, s.normal, dq, ds) : false;
    return is_mesh || is_albedo || is_normal || is_depth;
}
// Camera::ComputePixelWidthAtDistance (camera.h:182-197)
float PixelWidth(const atn_camera_param& c, float d)
{
    d = std::fabs(d);
    float hfov = c.vfov * c.height / float(c.width);
    hfov = PI * hfov / 180.0F;
    const float half = std::tan(hfov / 2) * d;
    return (half * 2) / float(c.width);
}

// ---- npr_impl.h ---------------------------------------------------------------------------------------------------------------
struct Ctx {
    const Scene& ctxt;
    const atn_camera_param& cam;
    FLConfig cfg;
    float pixel_width;
};

void GenerateSampleRayAndDisc(Info& info, const Ray& q, CMJ& sampler, float line_width, float pixel_width)     // :30-51
{
    info.disc = GenerateDisc(q, line_width, pixel_width);
    for (int i = 0; i < kRays; i++) {
        Desc& d = info.descs[i];
        float x, y;
        sampler.nextSample2D(x, y);
        d.u = x * 2 - 1; d.v = y * 2 - 1;
        const v3 pos = HitPositionOnDisc(d.u, d.v, info.disc);
        const Ray r(q.org, pos - q.org);
        d.ray_org = r.org; d.ray_dir = r.dir;
        d.is_terminated = false;
    }
    info.disc.accumulated_distance = 1;
}

void FeatureLineContribution(float closest, PathState& path, const FLConfig& cfg)     // :62-80
{
    const float pdf_line = (float(1) / kRays) * (closest * closest);
    const float weight = path.pdfb / (path.pdfb + pdf_line);
    path.contrib = path.throughput * weight * v3(cfg.line_color[0], cfg.line_color[1], cfg.line_color[2]);
    path.is_terminated = true;
}

Ray GetSampleRay(int32_t depth, Desc& desc, const Disc& prev, const Disc& cur)      // :101-124
{
    Ray r(desc.ray_org, desc.ray_dir);      // ExtractRayFromSampleRayDesc: the constructor normalises again
    if (depth > 0) {
        Ray n;
        if (NextSampleRay(desc, prev, cur, n)) r = n;
        else desc.is_terminated = true;
    }
    return r;
}

struct LineOut { bool found{ false }; int32_t bounce{ -1 }; float distance{ 0 }; };

// ShadeSampleRay, :383-509
void ShadeSampleRay(const Ctx& c, int32_t depth, const Ray& q, const Isect& isect, PathState& path, Info& info, LineOut& lo)
{
    const Scene& ctxt = c.ctxt;
    if (!mtrl_lines(ctxt, isect.mtrlid).enable) return;
    float closest = std::numeric_limits<float>::max();
    bool found = false;
    HitRec hq;
    evaluate_hit_result(hq, ctxt.GetObject((uint32_t)isect.objid), ctxt, q, isect);
    const float dist_q = length(hq.p - q.org);
    const float hpd = length(hq.p - info.disc.center);
    const Disc prev = info.disc;
    info.disc = DiscAtQueryRayHitPoint(hq.p, q.dir, prev.radius, hpd, info.disc.accumulated_distance);
    const Disc& disc = info.disc;
    const atn_material_param& mq_raw = ctxt.GetMaterial((uint32_t)hq.mtrlid);
    for (int i = 0; i < kRays; i++) {
        Desc& desc = info.descs[i];
        if (desc.is_terminated) continue;
        const Ray sr = GetSampleRay(depth, desc, prev, disc);
        if (desc.is_terminated) continue;
        Isect is;
        if (TraverseClosest(is, ctxt, sr, EPS, INF, nullptr)) {
            if (mtrl_lines(ctxt, is.mtrlid).enable) {
                // EvaluateQueryAndSampleRayHit, :126-212
                HitRec hs;
                evaluate_hit_result(hs, ctxt.GetObject((uint32_t)is.objid), ctxt, sr, is);
                desc.is_terminated = hs.meshid != hq.meshid;
                desc.prev_ray_hit_pos = hs.p;
                desc.prev_ray_hit_nml = hs.normal;
                const float d_s = DistanceOnRay(hs.p, q);
                if (IsInLineWidth(c.cfg.line_width, q, hs.p, disc.accumulated_distance - 1, c.pixel_width)) {
                    atn_material_param m;
                    FillMaterial(m, ctxt, hq.mtrlid);
                    const v4 aq = sampleTexture(ctxt, m.albedoMap, hq.u, hq.v, v4(m.baseColor.x, m.baseColor.y, m.baseColor.z, m.baseColor.w));
                    FillMaterial(m, ctxt, hs.mtrlid);
                    const v4 as = sampleTexture(ctxt, m.albedoMap, hs.u, hs.v, v4(m.baseColor.x, m.baseColor.y, m.baseColor.z, m.baseColor.w));
                    const v3 co(c.cam.origin[0], c.cam.origin[1], c.cam.origin[2]);
                    const float dq = length(hq.p - co), ds = length(hs.p - co);
                    if (EvaluateMetrics(q.org, hq, hs, aq, as, c.cfg, mtrl_lines(ctxt, hq.mtrlid).metric_flag, dq, ds, 2)) {
                        if (d_s < closest && d_s < dist_q) { found = true; closest = d_s; }
                        else if (dist_q < closest) { found = true; closest = dist_q; }
                    }
                }
            }
            else desc.is_terminated = true;
        }
        else {
            // EvaluateQueryRayHitButSampleRayNotHit, :214-282
            const v4 plane = ComputePlane(hq.normal, hq.p);
            v3 pos;
            if (RayHitPositionOnPlane(plane, sr, pos)) {
                const float d_s = DistanceOnRay(pos, q);
                if (IsInLineWidth(c.cfg.line_width, q, pos, disc.accumulated_distance - 1, c.pixel_width)) {
                    if (d_s < closest && d_s < dist_q) { found = true; closest = d_s; }
                    else if (dist_q < closest) { found = true; closest = dist_q; }
                }
            }
            desc.is_terminated = true;
        }
        if (!(mq_raw.attrib & ATN_MTRL_ATTR_GLOSSY)) desc.is_terminated = true;
    }
    if (found) {
        FeatureLineContribution(closest, path, c.cfg);
        lo.found = true; lo.bounce = depth; lo.distance = closest;
    }
    info.disc.accumulated_distance += hpd;
}

// ShadeMissSampleRay, :512-603 (without the CUDA path's __all_sync early exit)
void ShadeMissSampleRay(const Ctx& c, int32_t depth, const Ray& q, PathState& path, Info& info, LineOut& lo)
{
    const Scene& ctxt = c.ctxt;
    float closest = std::numeric_limits<float>::max();
    bool found = false;
    Disc prev;
    if (depth > 0) {
        // CreateNextDiscByDummyQueryRayHitPoint, :304-329
        const v3 dummy = q.org + float(100) * q.dir;
        const float hpd = length(dummy - info.disc.center);
        prev = info.disc;
        info.disc = DiscAtQueryRayHitPoint(dummy, q.dir, prev.radius, hpd, info.disc.accumulated_distance);
    }
    const Disc& disc = info.disc;
    for (int i = 0; i < kRays; i++) {
        Desc& desc = info.descs[i];
        if (desc.is_terminated) continue;
        const Ray sr = GetSampleRay(depth, desc, prev, disc);
        if (desc.is_terminated) continue;
        Isect is;
        if (TraverseClosest(is, ctxt, sr, EPS, INF, nullptr)) {
            if (mtrl_lines(ctxt, is.mtrlid).enable) {
                // EvaluateQueryRayNotHitButSampleRayHit, :331-380: the sample's hit evaluated with the QUERY ray
                HitRec hs;
                evaluate_hit_result(hs, ctxt.GetObject((uint32_t)is.objid), ctxt, q, is);
                const float d_s = DistanceOnRay(hs.p, q);
                if (d_s < closest && IsInLineWidth(c.cfg.line_width, q, hs.p, disc.accumulated_distance - 1, c.pixel_width)) {
                    found = true; closest = d_s;
                }
            }
            else desc.is_terminated = true;
        }
        else desc.is_terminated = true;
    }
    if (found) {
        FeatureLineContribution(closest, path, c.cfg);
        lo.found = true; lo.bounce = depth; lo.distance = closest;
    }
}

struct Stage0 { float u[kRays], v[kRays]; uint8_t live[kRays]; Disc disc; uint32_t dim; bool term; };

// radiance_with_feature_line, npr.cpp:101-200
void RadianceWithFeatureLine(const Ctx& c, PathState& path, Ray& ray, ShadowRay& shadow_ray, int32_t ix, int32_t iy, int32_t w, int32_t h,
                             int32_t maxDepth, int32_t rrDepth, Info& info, LineOut& lo, Stage0* st0)
{
    const Scene& ctxt = c.ctxt;
    GenerateSampleRayAndDisc(info, ray, path.sampler, c.cfg.line_width, c.pixel_width);
    int32_t depth = 0;
    while (depth < maxDepth) {
        bool cont = true;
        Isect isect;
        path.isHit = false;
        const Ray q = ray;
        if (TraverseClosest(isect, ctxt, q, EPS, INF, nullptr)) {
            ShadeSampleRay(c, depth, q, isect, path, info, lo);
            path.isHit = true;
            shade(path, ctxt, ray, shadow_ray, isect, rrDepth, depth, nullptr);
            HitShadowRay(ctxt, path, shadow_ray, isect.mtrlid >= 0 ? ctxt.GetMaterial(isect.mtrlid).stencil_type : 0, nullptr);
            cont = !path.is_terminated;
        }
        else {
            ShadeMissSampleRay(c, depth, q, path, info, lo);
            ShadeMiss(ix, iy, w, h, depth, ctxt, c.cam, path, ray);
            cont = false;
        }
        if (depth == 0 && st0) {
            for (int k = 0; k < kRays; k++) { st0->u[k] = info.descs[k].u; st0->v[k] = info.descs[k].v; st0->live[k] = info.descs[k].is_terminated ? 0 : 1; }
            st0->disc = info.disc;
            st0->dim = path.sampler.m_dimension;
            st0->term = path.is_terminated;
        }
        if (!cont) break;
        depth++;
    }
}

struct State {
    std::vector<Info> infos;
    std::vector<v4> contributes;    // NprPathTracer::contributes_ (two-pass mode)
    int32_t w{ 0 }, h{ 0 };
};

} // namespace

extern "C" {

struct orc_destination {    // oracle/aten_oracle.cpp's
    int32_t width, height, maxDepth, russianRouletteDepth, sample;
    uint32_t frame;
    int32_t progressive;
    int32_t nthreads;
};

void* orc_npr_create() { return new State(); }
void orc_npr_destroy(void* h) { delete static_cast<State*>(h); }
void orc_npr_reset(void* h) { State& S = *static_cast<State*>(h); S.infos.clear(); S.contributes.clear(); S.w = S.h = 0; }

// One frame into `film` (vec4[w*h], progressive or overwrite as orc_render; two_pass: the CPU OnRender's literal film, the mean of
// contributes_).  break_on_terminate: a terminated path ends the pixel's sample loop (pathtracing.cpp:350-352).  Optional outputs
// (null = skip): line float4[n] {found, bounce, distance, 0} of the last sample that found one; desc float4[n][8] {u, v, live,
// the path ended at bounce 0},
// disc float4[n][2] and dims uint32[n] after bounce 0 of the last sample; prim float4[n][2] the primary hit {hit, mesh id, depth,
// albedo luminance} {normal, 0}.
int orc_npr_render(void* h, const atn_scene_desc* scene, const atn_camera_param* camera, const uint32_t* seeds, uint32_t n_seeds,
                   const orc_destination* dst, int32_t break_on_terminate, int32_t two_pass, atn_vec4* film,
                   atn_vec4* line, atn_vec4* desc, atn_vec4* disc, uint32_t* dims, atn_vec4* prim)
{
    State& S = *static_cast<State*>(h);
    Scene ctxt(scene);
    const int32_t width = dst->width, height = dst->height;
    const size_t n = (size_t)width * height;
    int32_t maxDepth = dst->maxDepth;
    int32_t rrDepth = dst->russianRouletteDepth;
    if (rrDepth > maxDepth) rrDepth = maxDepth - 1;
    if (dst->nthreads > 0) omp_set_num_threads(dst->nthreads);
    if (S.w != width || S.h != height) { S.infos.assign(n, Info()); S.contributes.assign(n, v4(0, 0, 0, 0)); S.w = width; S.h = height; }
    Ctx c{ ctxt, *camera, FLConfig{}, 0.0F };
    std::memcpy(&c.cfg, scene->config.feature_line, sizeof(c.cfg));
    c.pixel_width = PixelWidth(*camera, 1);
    const uint32_t samples = (uint32_t)dst->sample;

    auto per_sample = [&](int32_t x, int32_t y, uint32_t i, PathState& path, LineOut& lo, Stage0* st0) {
        const int32_t idx = y * width + x;
        Ray ray; ShadowRay shadow_ray;
        GeneratePath(ray, x, y, (int32_t)i, dst->frame, path, *camera, seeds[idx % n_seeds]);
        path.contrib = v3(0);
        RadianceWithFeatureLine(c, path, ray, shadow_ray, x, y, width, height, maxDepth, rrDepth, S.infos[idx], lo, st0);
    };

#pragma omp parallel for schedule(dynamic, 4)
    for (int32_t y = 0; y < height; y++) {
        for (int32_t x = 0; x < width; x++) {
            const int32_t idx = y * width + x;
            LineOut lo;
            Stage0 st0{};
            if (two_pass) {
                // OnRender, npr.cpp:399-482: sample 0 (it feeds the screen-space shadow texture, out of scope), then samples 0..spp-1
                PathState path; path.samples = 0;
                per_sample(x, y, 0, path, lo, nullptr);
                if (!isInvalidColor(path.contrib)) S.contributes[idx] = S.contributes[idx] + v4(path.contrib, 1.0F);
                for (uint32_t i = 0; i < samples; i++) {
                    PathState p2; p2.samples = 0;
                    per_sample(x, y, i, p2, lo, &st0);
                    const bool invalid = isInvalidColor(p2.contrib);
                    if (!invalid) S.contributes[idx] = S.contributes[idx] + v4(p2.contrib, 1.0F);
                    if (!invalid && p2.is_terminated) break;
                }
                const v4 cc = S.contributes[idx];
                film[idx] = atn_vec4{ cc.x / cc.w, cc.y / cc.w, cc.z / cc.w, 1.0F };
            }
            else {
                v3 col(0); uint32_t cnt = 0;
                PathState path; path.samples = 0;
                for (uint32_t i = 0; i < samples; i++) {
                    per_sample(x, y, i, path, lo, &st0);
                    if (isInvalidColor(path.contrib)) continue;
                    col += path.contrib;
                    cnt++;
                    if (break_on_terminate && path.is_terminated) break;
                }
                col /= (float)cnt;
                const v4 v(col, 1);
                atn_vec4& cur = film[idx];
                if (dst->progressive) {
                    const float nn = static_cast<float>(static_cast<int32_t>(cur.w));
                    v4 cc(cur.x, cur.y, cur.z, cur.w);
                    cc = nn * cc + v;
                    const float d = nn + 1;
                    cur.x = cc.x / d; cur.y = cc.y / d; cur.z = cc.z / d;
                    cur.w = nn + 1;
                }
                else { cur.x = v.x; cur.y = v.y; cur.z = v.z; cur.w = v.w; }
            }
            if (line) line[idx] = lo.found ? atn_vec4{ 1.0F, (float)lo.bounce, lo.distance, 0.0F } : atn_vec4{ 0, 0, 0, 0 };
            if (desc) for (int k = 0; k < kRays; k++) desc[(size_t)idx * kRays + k] = atn_vec4{ st0.u[k], st0.v[k], (float)st0.live[k], st0.term ? 1.0F : 0.0F };
            if (disc) {
                disc[2 * (size_t)idx] = atn_vec4{ st0.disc.center.x, st0.disc.center.y, st0.disc.center.z, st0.disc.radius };
                disc[2 * (size_t)idx + 1] = atn_vec4{ st0.disc.normal.x, st0.disc.normal.y, st0.disc.normal.z, st0.disc.accumulated_distance };
            }
            if (dims) dims[idx] = st0.dim;
            if (prim) {
                // the primary hit of the pixel's sample-0 ray (the metrics' inputs, for the oracle-free edge test)
                PathState path; path.samples = 0;
                Ray ray;
                GeneratePath(ray, x, y, 0, dst->frame, path, *camera, seeds[idx % n_seeds]);
                Isect is;
                atn_vec4 a{ 0, -1, 0, 0 }, b{ 0, 0, 0, 0 };
                if (TraverseClosest(is, ctxt, ray, EPS, INF, nullptr)) {
                    HitRec hr;
                    evaluate_hit_result(hr, ctxt.GetObject((uint32_t)is.objid), ctxt, ray, is);
                    atn_material_param m;
                    FillMaterial(m, ctxt, hr.mtrlid);
                    const v4 al = sampleTexture(ctxt, m.albedoMap, hr.u, hr.v, v4(m.baseColor.x, m.baseColor.y, m.baseColor.z, m.baseColor.w));
                    const v3 co(camera->origin[0], camera->origin[1], camera->origin[2]);
                    a = atn_vec4{ 1.0F, (float)hr.meshid, length(hr.p - co), luminance(al.x, al.y, al.z) };
                    b = atn_vec4{ hr.normal.x, hr.normal.y, hr.normal.z, 0.0F };
                }
                prim[2 * (size_t)idx] = a; prim[2 * (size_t)idx + 1] = b;
            }
        }
    }
    return 0;
}

// ---- the geometry, for hand-worked cases (tests/test_npr_oracle_cpu.py) ----
float orc_npr_pixel_width(const atn_camera_param* cam, float d) { return PixelWidth(*cam, d); }
// disc: {center.xyz, radius, normal.xyz, accumulated_distance}
void orc_npr_generate_disc(const float* org, const float* dir, float line_width, float pixel_width, float* disc)
{
    const Disc d = GenerateDisc(Ray(v3(org[0], org[1], org[2]), v3(dir[0], dir[1], dir[2])), line_width, pixel_width);
    const float o[8] = { d.center.x, d.center.y, d.center.z, d.radius, d.normal.x, d.normal.y, d.normal.z, d.accumulated_distance };
    std::memcpy(disc, o, sizeof(o));
}
static Disc disc_of(const float* f) { Disc d; d.center = v3(f[0], f[1], f[2]); d.radius = f[3]; d.normal = v3(f[4], f[5], f[6]); d.accumulated_distance = f[7]; return d; }
void orc_npr_disc_position(float u, float v, const float* disc, float* out) { const v3 p = HitPositionOnDisc(u, v, disc_of(disc)); out[0] = p.x; out[1] = p.y; out[2] = p.z; }
void orc_npr_disc_at(const float* p, const float* dir, float prev_radius, float cur, float acc_without, float* disc)
{
    const Disc d = DiscAtQueryRayHitPoint(v3(p[0], p[1], p[2]), v3(dir[0], dir[1], dir[2]), prev_radius, cur, acc_without);
    const float o[8] = { d.center.x, d.center.y, d.center.z, d.radius, d.normal.x, d.normal.y, d.normal.z, d.accumulated_distance };
    std::memcpy(disc, o, sizeof(o));
}
// plane through p with normal n, ray (org, dir normalised): 1 = hit at t >= 0 (out = the point), 0 = behind or parallel
int32_t orc_npr_plane_hit(const float* n, const float* p, const float* org, const float* dir, float* out)
{
    v3 pos;
    const bool hit = RayHitPositionOnPlane(ComputePlane(v3(n[0], n[1], n[2]), v3(p[0], p[1], p[2])), Ray(v3(org[0], org[1], org[2]), v3(dir[0], dir[1], dir[2])), pos);
    out[0] = pos.x; out[1] = pos.y; out[2] = pos.z;
    return hit ? 1 : 0;
}
// distance of `point` from the ray, its projection (out) and the projection's distance from the origin (out[3])
float orc_npr_project(const float* point, const float* org, const float* dir, float* out)
{
    const Ray r(v3(org[0], org[1], org[2]), v3(dir[0], dir[1], dir[2]));
    v3 y;
    const float dist = ProjectPointOnRay(v3(point[0], point[1], point[2]), r, &y);
    out[0] = y.x; out[1] = y.y; out[2] = y.z; out[3] = DistanceOnRay(v3(point[0], point[1], point[2]), r);
    return dist;
}
// 1 = a next sample ray exists (out: org.xyz, dir.xyz)
int32_t orc_npr_next_ray(float u, float v, const float* prev_pos, const float* prev_nml, const float* prev_disc, const float* next_disc, float* out)
{
    Desc d; d.u = u; d.v = v; d.prev_ray_hit_pos = v3(prev_pos[0], prev_pos[1], prev_pos[2]); d.prev_ray_hit_nml = v3(prev_nml[0], prev_nml[1], prev_nml[2]);
    Ray r;
    if (!NextSampleRay(d, disc_of(prev_disc), disc_of(next_disc), r)) return 0;
    out[0] = r.org.x; out[1] = r.org.y; out[2] = r.org.z; out[3] = r.dir.x; out[4] = r.dir.y; out[5] = r.dir.z;
    return 1;
}
float orc_npr_depth_threshold(const float* p, float scale, const float* pq, const float* nq, const float* ps, const float* ns, float dq, float ds)
{
    return DepthThreshold(v3(p[0], p[1], p[2]), scale, v3(pq[0], pq[1], pq[2]), v3(nq[0], nq[1], nq[2]), v3(ps[0], ps[1], ps[2]), v3(ns[0], ns[1], ns[2]), dq, ds);
}
int32_t orc_npr_in_line_width(float w, const float* org, const float* dir, const float* point, float acc, float pixel_width)
{
    return IsInLineWidth(w, Ray(v3(org[0], org[1], org[2]), v3(dir[0], dir[1], dir[2])), v3(point[0], point[1], point[2]), acc, pixel_width) ? 1 : 0;
}
// EvaluateMetrics with the query / sample hit {p, normal, mesh id} and albedos (rgba), thresholds and flags
int32_t orc_npr_metrics(const float* p, const float* q_p, const float* q_n, int32_t q_mesh, const float* s_p, const float* s_n, int32_t s_mesh,
                        const float* aq, const float* as, float albedo_threshold, float normal_threshold, int32_t flags, float dq, float ds)
{
    HitRec q, s;
    q.p = v3(q_p[0], q_p[1], q_p[2]); q.normal = v3(q_n[0], q_n[1], q_n[2]); q.meshid = q_mesh;
    s.p = v3(s_p[0], s_p[1], s_p[2]); s.normal = v3(s_n[0], s_n[1], s_n[2]); s.meshid = s_mesh;
    FLConfig cfg{}; cfg.albedo_threshold = albedo_threshold; cfg.normal_threshold = normal_threshold;
    return EvaluateMetrics(v3(p[0], p[1], p[2]), q, s, v4(aq[0], aq[1], aq[2], aq[3]), v4(as[0], as[1], as[2], as[3]), cfg, flags, dq, ds, 2) ? 1 : 0;
}

} // extern "C"
