/*
 * ReSTIR ORACLE -- TEST INFRASTRUCTURE ONLY (tests/restir_oracle.py compiles it; the product never loads it).
 *
 * A CPU restatement of the reference's ReSTIR renderer (src/libaten/renderer/restir/restir_impl.h, restir.cpp and
 * src/libidaten/restir/) on top of the path-tracing oracle (oracle/orc_pt.h, orc_svgf.h, read as they are), with the frame
 * sequence, sample stream and quirk decisions of docs/RESTIR.md:
 *   generate the path once; bounce 0 = Shade -> EvaluateVisibility -> ApplyTemporalReuse (frame > 1) -> ApplySpatialReuse ->
 *   ComputePixelColor on the path's own sampler; bounces >= 1 = PathTracing::shade + HitShadowRay.
 */
#include "../../oracle/orc_pt.h"
#include "../../oracle/orc_svgf.h"
#include <omp.h>
#include <cmath>
#include <cstring>
#include <vector>

using namespace orc;

namespace {

// Reservoir, restir_types.h:10-78
struct Reservoir {
    float w_sum{ 0.0f }; int32_t M{ 0 }; int32_t y{ -1 }; float W{ 0.0f }; float target_pdf_of_y{ 0.0f };
    LightSampleResult light_sample_;
    void clear() { w_sum = 0.0f; M = 0; y = -1; target_pdf_of_y = 0.0f; W = 0.0f; }
    bool IsValid() const { return y >= 0; }
    bool update(const LightSampleResult& ls, int32_t sample, float weight, int32_t m, float u)     // :49-61
    {
        w_sum += weight;
        bool is_accepted = u < weight / w_sum;
        if (is_accepted) { light_sample_ = ls; y = sample; }
        M += m;
        return is_accepted;
    }
};

// ReSTIRInfo, restir_types.h:84-115 (+ whether the primary ray hit: the motion pass's input)
struct Info {
    v3 nml; int32_t mtrl_idx{ -1 };
    v3 wi; float u{ 0 };
    v3 p; float v{ 0 };
    float pre_sampled_r{ 0 }; int32_t mesh_id{ -1 }; float hit{ 0 };
    void clear() { *this = Info(); }
};

struct State {
    std::vector<Reservoir> res[2];
    std::vector<Info> info[2];
    std::vector<v4> nd, am, motion;
    int32_t pos{ 0 };
    int32_t w{ 0 }, h{ 0 };
    svgf::Matrices mtxs;
    bool motion_set{ false };
    bool offset_origin{ false };    // test switch: visibility rays from ray::Offset(p, nml) instead of the reference's p + AT_MATH_EPSILON * nml
};

// _detail::ComputeRadiance, restir_impl.h:31-65
v3 ComputeRadiance(const Scene& ctxt, const LightSampleResult& ls, uint32_t light_attrib, const v3& normal, const v3& ray_dir,
                   const atn_material_param& mtrl, float u, float v, float pre_sampled_r)
{
    const float cosShadow = std::fabs(dot(normal, ls.dir));
    const float cosLight = std::fabs(dot(ls.nml, -ls.dir));
    const float dist2 = ls.dist_to_light * ls.dist_to_light;
    const v3 brdf = sampleBSDF(ctxt, &mtrl, normal, ray_dir, ls.dir, u, v, pre_sampled_r).bsdf;
    const float G = (light_attrib & (ATN_LIGHT_ATTR_SINGULAR | ATN_LIGHT_ATTR_INFINITE)) ? cosShadow * cosLight : cosShadow * cosLight / dist2;
    return brdf * ls.light_color * G;
}

// _detail::ComputeTargetPDF, restir_impl.h:67-106
float ComputeTargetPDF(const Scene& ctxt, const LightSampleResult& ls, uint32_t light_attrib, const v3& normal, const v3& ray_dir,
                       const atn_material_param& mtrl, float u, float v, float pre_sampled_r)
{
    const float pdf = samplePDF(ctxt, &mtrl, normal, ray_dir, ls.dir, u, v);
    if (pdf == 0.0f) return 0.0f;
    const v3 e = ComputeRadiance(ctxt, ls, light_attrib, normal, ray_dir, mtrl, u, v, pre_sampled_r);
    return (e.x + e.y + e.z) / 3;
}

// GenerateInitialCandidate, restir_impl.h:126-205 (MaxLightCount = n_candidates)
void GenerateInitialCandidate(Reservoir& reservoir, const atn_material_param& mtrl, const Scene& ctxt, const v3& org, const v3& normal,
                              const v3& ray_dir, float u, float v, CMJ* sampler, float pre_sampled_r, int32_t n_candidates)
{
    const int32_t max_light_num = (int32_t)ctxt.GetLightNum();
    const int32_t light_cnt = std::min(n_candidates, max_light_num);
    reservoir.clear();
    float candidate_target_pdf = 0.0f;
    const float light_select_prob = 1.0f / (float)max_light_num;
    for (int32_t i = 0; i < light_cnt; i++) {
        const float r_light = sampler->nextSample();
        const int32_t light_pos = svgf::clampv<int32_t>((int32_t)(r_light * max_light_num), 0, max_light_num - 1);
        const atn_light_param& light = ctxt.GetLight(light_pos);
        LightSampleResult ls;
        Light_sample(ls, light, ctxt, org, normal, sampler);
        const float sampling_pdf = ls.pdf * light_select_prob;
        const float target_pdf = ComputeTargetPDF(ctxt, ls, light.attrib, normal, ray_dir, mtrl, u, v, pre_sampled_r);
        const float weight = sampling_pdf > 0 ? target_pdf / sampling_pdf : 0.0f;
        const float r = sampler->nextSample();
        if (reservoir.update(ls, light_pos, weight, 1, r)) candidate_target_pdf = target_pdf;
    }
    if (candidate_target_pdf > 0.0f) {
        reservoir.target_pdf_of_y = candidate_target_pdf;
        reservoir.W = reservoir.w_sum / (reservoir.target_pdf_of_y * reservoir.M);
    }
    if (!std::isfinite(reservoir.W)) reservoir.clear();
}

// ReSTIRRenderer::Shade, restir.cpp:102-238 (bounce 0)
void Shade(PathState& path, Ray& ray, const Isect& isect, const Scene& ctxt, int32_t rrDepth, const m4& W2C, int32_t n_candidates,
           Reservoir& reservoir, Info& info, v4& aov_nd, v4& aov_am)
{
    const Ray ray_in = ray;
    const auto& obj = ctxt.GetObject(static_cast<uint32_t>(isect.objid));
    HitRec rec;
    evaluate_hit_result(rec, obj, ctxt, ray_in, isect);
    const bool isBackfacing = dot(rec.normal, -ray_in.dir) < 0.0f;
    v3 orienting_normal = rec.normal;
    atn_material_param mtrl;
    FillMaterial(mtrl, ctxt, rec.mtrlid);
    const v4 albedo = sampleTexture(ctxt, mtrl.albedoMap, rec.u, rec.v, v4(1.0f));
    float pre_sampled_r;
    {
        v3 nn;
        pre_sampled_r = applyNormal(ctxt, mtrl, orienting_normal, nn, rec.u, rec.v, ray_in.dir, &path.sampler);
        orienting_normal = nn;
    }
    if (!attr_translucent(mtrl) && !attr_emissive(mtrl) && isBackfacing) orienting_normal = -orienting_normal;

    info.clear();
    info.nml = orienting_normal; info.mtrl_idx = rec.mtrlid; info.wi = ray_in.dir; info.u = rec.u; info.v = rec.v;
    info.p = rec.p; info.pre_sampled_r = pre_sampled_r; info.mesh_id = isect.meshid; info.hit = 1.0f;

    // AOV (restir.cpp:151-158)
    const v4 pos = W2C.apply(v4(rec.p, 1));
    aov_nd = v4(orienting_normal.x, orienting_normal.y, orienting_normal.z, pos.w);
    aov_am = v4(albedo.x, albedo.y, albedo.z, static_cast<float>(isect.meshid));

    if (mtrl.type == ATN_MTRL_EMISSIVE && HitImplicitLight(ctxt, isect.objid, isBackfacing, 0, path, ray_in, rec, mtrl)) return;

    if (!(attr_singular(mtrl) || attr_translucent(mtrl))) {
        GenerateInitialCandidate(reservoir, mtrl, ctxt, rec.p, orienting_normal, ray_in.dir, rec.u, rec.v, &path.sampler, pre_sampled_r, n_candidates);
    }
    const float russianProb = ComputeRussianProbability(0, rrDepth, path);
    MaterialSampling sampling;
    sampleMaterial(&sampling, ctxt, &mtrl, orienting_normal, ray_in.dir, &path.sampler, rec.u, rec.v, pre_sampled_r);
    PrepareForNextBounce(rec, russianProb, orienting_normal, mtrl, sampling, albedo.xyz(), path, ray);
}

// EvaluateVisibility, restir_impl.h:218-261; HitShadowRay's own terminated test counts as occluded, lightcontrib = 0
void EvaluateVisibility(const PathState& path, const Scene& ctxt, Reservoir& reservoir, const Info& info, bool offset_origin)
{
    bool isHit = false;
    if (reservoir.IsValid() && !path.is_terminated) {
        const v3 org = info.p + EPS * info.nml;
        v3 dir = reservoir.light_sample_.pos - org;
        const float dist = length(dir);
        dir = dir / dist;
        atn_material_param mtrl;
        FillMaterial(mtrl, ctxt, info.mtrl_idx);
        const Ray r = offset_origin ? Ray(info.p, dir, info.nml) : Ray(org, dir);
        isHit = HitTestToTargetLight(ctxt, r, ctxt.GetLight(reservoir.y), offset_origin ? length(reservoir.light_sample_.pos - r.org) : dist,
                                     mtrl.stencil_type, nullptr);
    }
    if (!isHit) {
        reservoir.w_sum = 0.0f; reservoir.W = 0.0f; reservoir.target_pdf_of_y = 0.0f; reservoir.y = -1;
    }
}

// IsAcceptableNeighbor, restir_impl.h:275-289
bool IsAcceptableNeighbor(const atn_material_param& mtrl, int32_t mesh_id, const v3& normal,
                          const atn_material_param& neighbor_mtrl, int32_t neighbor_mesh_id, const v3& neighbor_normal)
{
    return mtrl.type == neighbor_mtrl.type && mesh_id == neighbor_mesh_id && dot(normal, neighbor_normal) >= 0.95f;
}

// ApplyTemporalReuse, restir_impl.h:309-428
void ApplyTemporalReuse(int32_t idx, int32_t width, int32_t height, const Scene& ctxt, CMJ& sampler, Reservoir& combined,
                        const Info& self_info, const std::vector<Reservoir>& prev_res, const std::vector<Info>& prev_infos,
                        const std::vector<v4>& aov_am, const std::vector<v4>& motion)
{
    const int32_t ix = idx % width, iy = idx / width;
    atn_material_param mtrl;
    FillMaterial(mtrl, ctxt, self_info.mtrl_idx);
    const v3& normal = self_info.nml;
    const int32_t mesh_id = static_cast<int32_t>(aov_am[idx].w);
    float candidate_target_pdf = combined.IsValid() ? combined.target_pdf_of_y : 0.0f;
    const int32_t maxM = 20 * combined.M;
    const v4 md = motion[idx];
    const int32_t px = (int32_t)(ix + md.x * width);
    const int32_t py = (int32_t)(iy + md.y * height);
    if (px >= 0 && px <= width - 1 && py >= 0 && py <= height - 1) {
        LightSampleResult lightsample;
        const int32_t nidx = py * width + px;
        const Reservoir& nres = prev_res[nidx];
        const int32_t m = std::min(nres.M, maxM);
        if (nres.IsValid()) {
            const Info& ninfo = prev_infos[nidx];
            atn_material_param nmtrl;
            FillMaterial(nmtrl, ctxt, ninfo.mtrl_idx);
            const bool ok = ninfo.mtrl_idx >= 0 && IsAcceptableNeighbor(mtrl, mesh_id, normal, nmtrl, ninfo.mesh_id, ninfo.nml);
            if (ok) {
                const atn_light_param& light = ctxt.GetLight(nres.y);
                Light_sample(lightsample, light, ctxt, self_info.p, ninfo.nml, &sampler);
                const float target_pdf = ComputeTargetPDF(ctxt, lightsample, light.attrib, self_info.nml, self_info.wi, mtrl,
                                                          self_info.u, self_info.v, self_info.pre_sampled_r);
                const float weight = target_pdf * nres.W * m;
                const float r = sampler.nextSample();
                if (combined.update(lightsample, nres.y, weight, m, r)) candidate_target_pdf = target_pdf;
            }
        }
        else {
            combined.update(lightsample, -1, 0.0f, m, 0.0f);
        }
    }
    if (candidate_target_pdf > 0.0f) {
        combined.target_pdf_of_y = candidate_target_pdf;
        combined.W = combined.w_sum / (combined.target_pdf_of_y * combined.M);
    }
    if (!std::isfinite(combined.W)) combined.clear();
}

// ApplySpatialReuse, restir_impl.h:445-569
void ApplySpatialReuse(int32_t idx, int32_t width, int32_t height, const Scene& ctxt, CMJ& sampler, Reservoir& combined,
                       const std::vector<Reservoir>& reservoirs, const std::vector<Info>& infos, const std::vector<v4>& aov_am)
{
    const int32_t ix = idx % width, iy = idx / width;
    const Info& self_info = infos[idx];
    atn_material_param mtrl;
    FillMaterial(mtrl, ctxt, self_info.mtrl_idx);
    const int32_t mesh_id = static_cast<int32_t>(aov_am[idx].w);
    static const int32_t offset_x[] = { -1, 0, 1, -1, 0, 1, -1, 0, 1 };
    static const int32_t offset_y[] = { -1, -1, -1, 0, 0, 0, 1, 1, 1 };
    combined.clear();
    float candidate_target_pdf = 0.0f;
    int32_t M_sum = 0;
    for (int32_t i = 0; i < 9; i++) {
        const int32_t xx = ix + offset_x[i], yy = iy + offset_y[i];
        if (!(xx >= 0 && xx <= width - 1 && yy >= 0 && yy <= height - 1)) continue;
        const int32_t nidx = yy * width + xx;
        const Reservoir& nres = reservoirs[nidx];
        M_sum += nres.M;
        if (!nres.IsValid()) continue;
        const Info& ninfo = infos[nidx];
        atn_material_param nmtrl;
        FillMaterial(nmtrl, ctxt, ninfo.mtrl_idx);
        const int32_t nmesh = static_cast<int32_t>(aov_am[nidx].w);
        if (!(ninfo.mtrl_idx >= 0 && IsAcceptableNeighbor(mtrl, mesh_id, self_info.nml, nmtrl, nmesh, ninfo.nml))) continue;
        const atn_light_param& light = ctxt.GetLight(nres.y);
        LightSampleResult lightsample;
        Light_sample(lightsample, light, ctxt, self_info.p, ninfo.nml, &sampler);
        const float target_pdf = ComputeTargetPDF(ctxt, lightsample, light.attrib, self_info.nml, self_info.wi, mtrl,
                                                  self_info.u, self_info.v, self_info.pre_sampled_r);
        const int32_t m = nres.M;
        const float weight = target_pdf * nres.W * m;
        const float r = sampler.nextSample();
        if (combined.update(lightsample, nres.y, weight, m, r)) candidate_target_pdf = target_pdf;
    }
    combined.M = M_sum;
    if (candidate_target_pdf > 0.0f) {
        combined.target_pdf_of_y = candidate_target_pdf;
        combined.W = combined.w_sum / (combined.target_pdf_of_y * combined.M);
    }
    if (!std::isfinite(combined.W)) combined.clear();
}

// ComputePixelColor, restir_impl.h:582-621 + restir.cpp:440-470 (throughput = 1 at bounce 0)
void ComputePixelColor(PathState& path, const Scene& ctxt, const Reservoir& reservoir, const Info& info, const v4& albedo_meshid)
{
    if (!reservoir.IsValid()) return;
    atn_material_param mtrl;
    FillMaterial(mtrl, ctxt, info.mtrl_idx);
    const atn_light_param& light = ctxt.GetLight(reservoir.y);
    const v3 le = ComputeRadiance(ctxt, reservoir.light_sample_, light.attrib, info.nml, info.wi, mtrl, info.u, info.v, info.pre_sampled_r);
    v3 contrib = le * reservoir.W;
    contrib = contrib * v3(albedo_meshid.x, albedo_meshid.y, albedo_meshid.z);
    path.contrib += contrib * v3(1.0f);
}

void put(const State&, const Reservoir& r, float* o)
{
    o[0] = (float)r.y; o[1] = (float)r.M; o[2] = r.W; o[3] = r.w_sum; o[4] = r.target_pdf_of_y;
}

} // namespace

extern "C" {

struct orc_destination {    // oracle/aten_oracle.cpp's
    int32_t width, height, maxDepth, russianRouletteDepth, sample;
    uint32_t frame;
    int32_t progressive;
    int32_t nthreads;
};

void* orc_restir_create() { return new State(); }
void orc_restir_destroy(void* h) { delete static_cast<State*>(h); }

void orc_restir_set_offset_origin(void* h, int32_t on) { static_cast<State*>(h)->offset_origin = on != 0; }

void orc_restir_set_motion_depth(void* h, const atn_vec4* md, uint32_t n)
{
    State& S = *static_cast<State*>(h);
    S.motion.resize(n);
    for (uint32_t i = 0; i < n; i++) S.motion[i] = v4(md[i].x, md[i].y, md[i].z, md[i].w);
    S.motion_set = true;
}

// One frame (sample = 1).  film: vec4[w*h] (progressive or overwrite, as orc_render).  Optional outputs (null = skip):
// stages float[3][n][5] {y, M, W, w_sum, target_pdf} after shade / visibility+temporal / spatial; info float4[4][n];
// aovs float4[3][n] normal-depth, albedo-meshid, motion-depth; dims uint32[n] the sampler dimension after bounce 0's passes;
// terminated uint8[n] (1: the path ended at bounce 0).
int orc_restir_render(void* h, const atn_scene_desc* scene, const atn_camera_param* camera, const uint32_t* seeds, uint32_t n_seeds,
                      const orc_destination* dst, int32_t mode, int32_t n_candidates, int32_t compute_motion,
                      atn_vec4* film, float* stages, atn_vec4* info_out, atn_vec4* aovs, uint32_t* dims, uint8_t* terminated)
{
    State& S = *static_cast<State*>(h);
    Scene ctxt(scene);
    const int32_t width = dst->width, height = dst->height;
    const size_t n = (size_t)width * height;
    int32_t maxDepth = dst->maxDepth;
    int32_t rrDepth = dst->russianRouletteDepth;
    if (rrDepth > maxDepth) rrDepth = maxDepth - 1;
    if (dst->nthreads > 0) omp_set_num_threads(dst->nthreads);
    if (S.w != width || S.h != height) {
        for (int k = 0; k < 2; k++) { S.res[k].assign(n, Reservoir()); S.info[k].assign(n, Info()); }
        S.nd.assign(n, v4(0, 0, 0, 1)); S.am.assign(n, v4(0, 0, 0, 1));
        if (!S.motion_set || S.motion.size() < n) { S.motion.assign(n, v4(0, 0, 0, 0)); S.motion_set = false; }
        S.w = width; S.h = height; S.pos = 0;
    }
    if (!compute_motion && !S.motion_set) return -1;
    S.mtxs.Reset(*camera);
    const m4 W2C = S.mtxs.GetW2C();
    const m4 prevW2C = svgf::mul(S.mtxs.V2C, S.mtxs.PrevW2V);
    const int32_t cur = S.pos, oth = 1 - S.pos;
    std::vector<Reservoir>& cres = S.res[cur];
    std::vector<Info>& cinfo = S.info[cur];
    std::vector<PathState> paths(n);
    std::vector<Ray> rays(n);

    // bounce 0: GeneratePath once, hit test, Shade / ShadeMiss (InitReSTIR folded in: every pixel's reservoir and info is written)
#pragma omp parallel for
    for (int32_t y = 0; y < height; y++) {
        for (int32_t x = 0; x < width; x++) {
            const int32_t idx = y * width + x;
            PathState& path = paths[idx];
            path.samples = 0;
            GeneratePath(rays[idx], x, y, 0, dst->frame, path, *camera, seeds[idx % n_seeds]);
            path.contrib = v3(0);
            cres[idx].clear();
            cres[idx].light_sample_ = LightSampleResult();
            cinfo[idx].clear();
            Isect isect;
            path.isHit = false;
            if (TraverseClosest(isect, ctxt, rays[idx], EPS, INF, nullptr)) {
                path.isHit = true;
                Shade(path, rays[idx], isect, ctxt, rrDepth, W2C, n_candidates, cres[idx], cinfo[idx], S.nd[idx], S.am[idx]);
            }
            else {
                ShadeMiss(x, y, width, height, 0, ctxt, *camera, path, rays[idx]);
                const v4 bg = Background_SampleFromRay(PinholeSample(*camera, x / (float)width, y / (float)height).dir, ctxt.cfg().bg, ctxt);
                S.nd[idx] = v4(0.0f, 0.0f, 0.0f, -1.0f);
                S.am[idx] = v4(bg.x, bg.y, bg.z, -1.0f);
            }
        }
    }
    if (stages) for (size_t i = 0; i < n; i++) put(S, cres[i], stages + 5 * i);
    if (compute_motion) {
        S.motion.resize(n);
        for (size_t i = 0; i < n; i++) S.motion[i] = svgf::ComputeMotionDepth(v4(cinfo[i].p, cinfo[i].hit), W2C, prevW2C);
    }

#pragma omp parallel for
    for (int32_t i = 0; i < (int32_t)n; i++) EvaluateVisibility(paths[i], ctxt, cres[i], cinfo[i], S.offset_origin);

    if ((mode == 1 || mode == 3) && dst->frame > 1) {
#pragma omp parallel for
        for (int32_t i = 0; i < (int32_t)n; i++) {
            if (paths[i].is_terminated) continue;
            ApplyTemporalReuse(i, width, height, ctxt, paths[i].sampler, cres[i], cinfo[i], S.res[oth], S.info[oth], S.am, S.motion);
        }
    }
    if (stages) for (size_t i = 0; i < n; i++) put(S, cres[i], stages + 5 * (n + i));
    const bool spatial = mode == 1 || mode == 2;
    if (spatial) {
#pragma omp parallel for
        for (int32_t i = 0; i < (int32_t)n; i++) {
            if (paths[i].is_terminated) continue;
            ApplySpatialReuse(i, width, height, ctxt, paths[i].sampler, S.res[oth][i], cres, cinfo, S.am);
        }
        if (stages) for (size_t i = 0; i < n; i++) if (!paths[i].is_terminated) put(S, S.res[oth][i], stages + 5 * (2 * n + i));
    }
    const std::vector<Reservoir>& target = spatial ? S.res[oth] : cres;
#pragma omp parallel for
    for (int32_t i = 0; i < (int32_t)n; i++) {
        if (paths[i].is_terminated) continue;
        ComputePixelColor(paths[i], ctxt, target[i], cinfo[i], S.am[i]);
    }
    if (dims) for (size_t i = 0; i < n; i++) dims[i] = paths[i].sampler.m_dimension;
    if (terminated) for (size_t i = 0; i < n; i++) terminated[i] = paths[i].is_terminated ? 1 : 0;
    if (info_out) {
        for (size_t i = 0; i < n; i++) {
            const Info& in = cinfo[i];
            float mt, me;
            std::memcpy(&mt, &in.mtrl_idx, 4); std::memcpy(&me, &in.mesh_id, 4);
            info_out[i] = atn_vec4{ in.nml.x, in.nml.y, in.nml.z, mt };
            info_out[n + i] = atn_vec4{ in.wi.x, in.wi.y, in.wi.z, in.u };
            info_out[2 * n + i] = atn_vec4{ in.p.x, in.p.y, in.p.z, in.v };
            info_out[3 * n + i] = atn_vec4{ in.pre_sampled_r, me, in.hit, 0.0f };
        }
    }
    if (aovs) {
        for (size_t i = 0; i < n; i++) {
            aovs[i] = atn_vec4{ S.nd[i].x, S.nd[i].y, S.nd[i].z, S.nd[i].w };
            aovs[n + i] = atn_vec4{ S.am[i].x, S.am[i].y, S.am[i].z, S.am[i].w };
            aovs[2 * n + i] = atn_vec4{ S.motion[i].x, S.motion[i].y, S.motion[i].z, S.motion[i].w };
        }
    }
    S.pos = oth;        // ReuseParams::Update, every frame

    // bounces >= 1: PathTracing::radiance's loop from depth 1, then OnRender's film write (oracle/aten_oracle.cpp, orc_render_cost)
#pragma omp parallel for
    for (int32_t y = 0; y < height; y++) {
        for (int32_t x = 0; x < width; x++) {
            const int32_t idx = y * width + x;
            PathState& path = paths[idx];
            Ray& ray = rays[idx];
            ShadowRay shadow_ray;
            if (!path.is_terminated) {
                for (int32_t depth = 1; depth < maxDepth; depth++) {
                    Isect isect;
                    path.isHit = false;
                    bool willContinue = true;
                    if (TraverseClosest(isect, ctxt, ray, EPS, INF, nullptr)) {
                        path.isHit = true;
                        shade(path, ctxt, ray, shadow_ray, isect, rrDepth, depth, nullptr);
                        HitShadowRay(ctxt, path, shadow_ray, isect.mtrlid >= 0 ? ctxt.GetMaterial(isect.mtrlid).stencil_type : 0, nullptr);
                        willContinue = !path.is_terminated;
                    }
                    else {
                        ShadeMiss(x, y, width, height, depth, ctxt, *camera, path, ray);
                        willContinue = false;
                    }
                    if (!willContinue) break;
                }
            }
            v3 col(0); uint32_t cnt = 0;
            if (!isInvalidColor(path.contrib)) { col += path.contrib; cnt++; }
            col /= (float)cnt;
            v4 v(col, 1);
            atn_vec4& c = film[idx];
            if (dst->progressive) {
                float nn = static_cast<float>(static_cast<int32_t>(c.w));
                v4 cc(c.x, c.y, c.z, c.w);
                cc = nn * cc + v;
                float d = nn + 1;
                c.x = cc.x / d; c.y = cc.y / d; c.z = cc.z / d;
                c.w = nn + 1;
            }
            else { c.x = v.x; c.y = v.y; c.z = v.z; c.w = v.w; }
        }
    }
    return 0;
}

} // extern "C"
