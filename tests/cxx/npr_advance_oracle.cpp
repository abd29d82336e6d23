/*
 * NPR LOOK-THROUGH ORACLE -- TEST INFRASTRUCTURE ONLY (tests/npr_advance_oracle.py compiles it; the product never loads it).
 *
 * The NPR oracle (npr_oracle.cpp, included as it is for the feature-line helpers) with what it leaves out: AdvanceNPRPath
 * (src/libaten/renderer/npr/npr.cpp:202-282), CheckStencil and CheckMaterialTranslucentByAlpha
 * (renderer/pathtracing/pathtracing_impl.h:511-678), radiance_with_feature_line's loop with the advance in it (npr.cpp:101-200) and
 * PathTracing::shade / ShadeMiss with the path's alpha blend (pathtracing.cpp:158, pathtracing_impl.h:167), built from
 * oracle/orc_pt.h's helpers.  Written literally: both checks run their ten-iteration loops as the reference does, and after a check
 * said true the path's ray is walked AGAIN (npr.cpp:272-281) -- the device takes the last walk's answer instead, and
 * tests/test_npr_advance_cpu.py holds that shortcut to this file's literal walk.  docs/NPR_ADVANCE.md lists the quirks kept.
 */
#include "npr_oracle.cpp"

namespace {

// PathThroughput::alpha_blend and PathAttribute::is_accumulating_alpha_blending (pt_params.h), as GeneratePath leaves them
// (ClearAlphaBlend then ClearPathAttribute, pathtracing_impl.h:103-105)
struct Blend { float transmission{ 1.0F }; v3 throughput{ 0.0F }; bool accumulating{ true }; };

// what the tests look at of one AdvanceNPRPath call
struct AdvRec {
    int32_t kind{ 0 };              // the check that said true: 0 none, 1 stencil, 2 alpha
    int32_t walks{ 0 };             // closest-hit walks done inside the checks (a miss CheckStencil repeats counts once)
    int32_t stencil_verdict{ 0 };   // 0 the material is not STENCIL, 1 true (front-facing ALWAYS), 2 back-facing ALWAYS, 3 NONE, 4 miss, 5 ten STENCIL layers
    int32_t alpha_end{ 0 };         // 0 no look-through, 1 an opaque surface, 2 a miss, 3 the tenth walk ended on a pane
    bool last_hit{ false }; Isect last;     // the last walk inside the check that said true
    bool rewalk_same{ true };       // the literal re-walk gave that walk's answer
};

// CheckStencil, pathtracing_impl.h:612-678 (`bounce` is the constant 0 the NPR renderer passes)
bool CheckStencil(Ray& curr_ray, const Scene& ctxt, const v3& hit_pos, const v3& hit_nml, const atn_material_param& mtrl, AdvRec& ar)
{
    if (mtrl.stencil_type != 2) return false;       // StencilType::STENCIL
    constexpr size_t MAX_LOOKUPS = 10;
    Ray ray(hit_pos, curr_ray.dir, -hit_nml);
    bool missed = false;
    ar.stencil_verdict = 5;
    for (size_t i = 0; i < MAX_LOOKUPS; i++) {
        Isect isect;
        const bool is_hit = TraverseClosest(isect, ctxt, ray, EPS, INF, nullptr);
        if (!missed) { ar.walks++; ar.last = isect; ar.last_hit = is_hit; }
        if (is_hit) {
            const atn_material_param& hit_mtrl = ctxt.GetMaterial((uint32_t)isect.mtrlid);
            if (hit_mtrl.stencil_type == 1) {       // ALWAYS
                HitRec rec;
                evaluate_hit_result(rec, ctxt.GetObject((uint32_t)isect.objid), ctxt, ray, isect);
                const bool is_back_facing = dot(rec.normal, -ray.dir) < 0.0F;
                if (is_back_facing) { ar.stencil_verdict = 2; return false; }
                curr_ray = ray;
                ar.stencil_verdict = 1;
                return true;
            }
            else if (hit_mtrl.stencil_type == 0) { ar.stencil_verdict = 3; return false; }
            else {
                HitRec rec;
                evaluate_hit_result(rec, ctxt.GetObject((uint32_t)isect.objid), ctxt, ray, isect);
                ray = Ray(rec.p, ray.dir, -rec.normal);
            }
        }
        else { missed = true; ar.stencil_verdict = 4; }     // (the reference goes round again with the same ray)
    }
    return false;
}

// CheckMaterialTranslucentByAlpha, pathtracing_impl.h:511-610
bool CheckAlpha(const Scene& ctxt, const atn_material_param& original_mtrl, float u, float v, const v3& original_hit_pos, const v3& original_hit_nml,
                Ray& ray, PathState& path, Blend& ab, AdvRec& ar)
{
    if (!ctxt.cfg().enable_alpha_blending) return false;
    if (!ab.accumulating) return false;
    atn_material_param mtrl = original_mtrl;
    if (attr_translucent(mtrl)) return false;
    v4 albedo = sampleTexture(ctxt, mtrl.albedoMap, u, v, v4(1.0F, 1.0F, 1.0F, 1.0F));
    float alpha = albedo.w * mtrl.baseColor.w;
    constexpr size_t MAX_LOOKUPS = 10;
    if (alpha < 1.0F) {
        v3 hit_pos = original_hit_pos, hit_nml = original_hit_nml;
        ar.alpha_end = 3;
        for (size_t i = 0; i < MAX_LOOKUPS; i++) {
            ray = Ray(hit_pos, ray.dir, -hit_nml);
            const v4 base(mtrl.baseColor.x, mtrl.baseColor.y, mtrl.baseColor.z, mtrl.baseColor.w);
            const v4 radiance = ab.transmission * base * albedo * alpha;
            ab.throughput = ab.throughput + radiance.xyz();
            ab.transmission *= (1.0F - alpha);
            path.is_singular = true;
            Isect isect;
            const bool is_hit = TraverseClosest(isect, ctxt, ray, EPS, INF, nullptr);
            ar.walks++; ar.last = isect; ar.last_hit = is_hit;
            if (!is_hit) { ar.alpha_end = 2; break; }
            HitRec rec;
            evaluate_hit_result(rec, ctxt.GetObject((uint32_t)isect.objid), ctxt, ray, isect);
            FillMaterial(mtrl, ctxt, rec.mtrlid);       // (ctxt.GetMaterial(rec.mtrlid); a negative id is the fallback here)
            albedo = sampleTexture(ctxt, mtrl.albedoMap, rec.u, rec.v, v4(1.0F, 1.0F, 1.0F, 1.0F));
            alpha = albedo.w * mtrl.baseColor.w;
            if (alpha >= 1.0F) { ar.alpha_end = 1; break; }
            hit_pos = rec.p;
            hit_nml = rec.normal;
            const bool is_back_facing = dot(-ray.dir, hit_nml) < 0.0F;
            if (is_back_facing) hit_nml = -hit_nml;
        }
        return true;
    }
    else ab.accumulating = false;
    return false;
}

// NprPathTracer::AdvanceNPRPath, npr.cpp:202-282
void AdvanceNPRPath(const Scene& ctxt, PathState& path, Blend& ab, Ray& path_ray, Isect& isect, AdvRec& ar)
{
    const Ray ray = path_ray;
    HitRec rec;
    evaluate_hit_result(rec, ctxt.GetObject((uint32_t)isect.objid), ctxt, ray, isect);
    const bool isBackfacing = dot(rec.normal, -ray.dir) < 0.0F;
    v3 orienting_normal = rec.normal;
    atn_material_param mtrl;
    FillMaterial(mtrl, ctxt, rec.mtrlid);
    // applyNormal first, the back-face flip second (the other way round than PathTracing::shade)
    {
        v3 nn;
        applyNormal(ctxt, mtrl, orienting_normal, nn, rec.u, rec.v, ray.dir, &path.sampler);
        orienting_normal = nn;
    }
    if (!attr_translucent(mtrl) && isBackfacing) orienting_normal = -orienting_normal;
    bool need_advance_path_one_more = false;
    if (CheckStencil(path_ray, ctxt, rec.p, orienting_normal, mtrl, ar)) {
        need_advance_path_one_more = true;
        ar.kind = 1;
    }
    else if (ctxt.cfg().enable_alpha_blending) {
        if (CheckAlpha(ctxt, mtrl, rec.u, rec.v, rec.p, orienting_normal, path_ray, path, ab, ar)) {
            need_advance_path_one_more = true;
            ar.kind = 2;
        }
    }
    if (need_advance_path_one_more) {
        Isect isect_tmp;
        const bool isHit = TraverseClosest(isect_tmp, ctxt, path_ray, EPS, INF, nullptr);
        ar.rewalk_same = isHit == ar.last_hit
            && (!isHit || (isect_tmp.objid == ar.last.objid && isect_tmp.tri_id == ar.last.tri_id && isect_tmp.mtrlid == ar.last.mtrlid
                           && std::memcmp(&isect_tmp.a, &ar.last.a, 4) == 0 && std::memcmp(&isect_tmp.b, &ar.last.b, 4) == 0
                           && std::memcmp(&isect_tmp.t, &ar.last.t, 4) == 0));
        isect = isect_tmp;
        path.isHit = isHit;
    }
}

// PathTracing::shade (pathtracing.cpp:91-236) as oracle/orc_pt.h restates it, with the path's alpha blend at :158
void ShadeBlend(PathState& path, const Blend& ab, const Scene& ctxt, Ray& ray, ShadowRay& shadow_ray, const Isect& isect, int32_t rrDepth, int32_t bounce)
{
    if (path.is_terminated) return;
    const Ray ray_in = ray;
    HitRec rec;
    evaluate_hit_result(rec, ctxt.GetObject((uint32_t)isect.objid), ctxt, ray_in, isect);
    const bool isBackfacing = dot(rec.normal, -ray_in.dir) < 0.0F;
    v3 orienting_normal = rec.normal;
    atn_material_param mtrl;
    FillMaterial(mtrl, ctxt, rec.mtrlid);
    v4 albedo = sampleTexture(ctxt, mtrl.albedoMap, rec.u, rec.v, v4(mtrl.baseColor.x, mtrl.baseColor.y, mtrl.baseColor.z, mtrl.baseColor.w));
    shadow_ray.isActive = false;
    albedo = ab.transmission * albedo + v4(ab.throughput);
    const bool is_toon_mtrl = mtrl.type == ATN_MTRL_TOON || mtrl.type == ATN_MTRL_STYLIZED_BRDF;
    bool is_hit_implicit_light = false;
    if (mtrl.type == ATN_MTRL_EMISSIVE) {
        is_hit_implicit_light = HitImplicitLight(ctxt, isect.objid, isBackfacing, bounce, path, ray_in, rec, mtrl);
    }
    else if (is_toon_mtrl) {
        if (bounce == 0) {
            const v3 toon_bsdf = Toon::bsdf(ctxt, mtrl, path, rec.p, rec.normal, ray_in.dir, rec.u, rec.v, nullptr);
            path.contrib += path.throughput * toon_bsdf * albedo.xyz();
            path.is_terminated = true;
        }
        is_hit_implicit_light = true;
    }
    if (is_hit_implicit_light) {
        if (is_toon_mtrl && (bounce > 0 || ctxt.d->enable_shadowray_base_stylized_shadow)) {
            mtrl.type = mtrl.toon.toon_type == ATN_MTRL_DIFFUSE ? ATN_MTRL_DIFFUSE : ATN_MTRL_SPECULAR;
            const bool sing = mtrl.toon.toon_type == ATN_MTRL_TOON_SPECULAR;
            mtrl.attrib = (mtrl.attrib & ~(uint32_t)ATN_MTRL_ATTR_SINGULAR) | (sing ? ATN_MTRL_ATTR_SINGULAR : 0u);
        }
        else return;
    }
    if (!attr_translucent(mtrl) && isBackfacing) orienting_normal = -orienting_normal;
    float pre_sampled_r;
    {
        v3 nn;
        pre_sampled_r = applyNormal(ctxt, mtrl, orienting_normal, nn, rec.u, rec.v, ray_in.dir, &path.sampler);
        orienting_normal = nn;
    }
    FillShadowRay(shadow_ray, ctxt, path, mtrl, ray_in, rec.p, orienting_normal, rec.u, rec.v, albedo, pre_sampled_r);
    const float russianProb = ComputeRussianProbability(bounce, rrDepth, path);
    MaterialSampling sampling;
    sampleMaterial(&sampling, ctxt, &mtrl, orienting_normal, ray_in.dir, &path.sampler, rec.u, rec.v, pre_sampled_r);
    PrepareForNextBounce(rec, russianProb, orienting_normal, mtrl, sampling, albedo.xyz(), path, ray);
}

// ShadeMiss (pathtracing_impl.h:112-176) with ApplyAlphaBlend
void ShadeMissBlend(int32_t ix, int32_t iy, int32_t width, int32_t height, int32_t bounce, const Scene& ctxt, const atn_camera_param& camera,
                    PathState& path, const Blend& ab, const Ray& ray)
{
    if (!path.is_terminated && !path.isHit) {
        v3 dir = ray.dir;
        if (bounce == 0) {
            const float s = ix / (float)(width);
            const float t = iy / (float)(height);
            dir = PinholeSample(camera, s, t).dir;
        }
        const v4 emit = Background_SampleFromRay(dir, ctxt.cfg().bg, ctxt);
        float misW = 1.0f;
        if (bounce == 0 || (bounce == 1 && path.is_singular)) {
        }
        else {
            float pdfLight = IBL_samplePdf(emit.xyz(), ctxt.cfg().bg.avgIllum);
            if (sampling_options().ibl_importance && ctxt.cfg().bg.envmap_tex_idx >= 0 && ctxt.cfg().bg.enable_env_map)
                pdfLight = IBL_direction_pdf(ctxt, dir);
            misW = path.pdfb / (pdfLight + path.pdfb);
        }
        v3 contrib = ab.transmission * (misW * emit).xyz() + ab.throughput;
        contrib *= path.throughput;
        path.contrib += contrib;
        path.is_terminated = true;
    }
}

struct AdvStage0 { AdvRec ar; int32_t answer{ -1 }; bool singular{ false }; Blend ab; int32_t mtrl{ -1 }; };

// radiance_with_feature_line, npr.cpp:101-200, with AdvanceNPRPath
void RadianceWithAdvance(const Ctx& c, PathState& path, Ray& ray, ShadowRay& shadow_ray, int32_t ix, int32_t iy, int32_t w, int32_t h,
                         int32_t maxDepth, int32_t rrDepth, Info& info, LineOut& lo, Stage0* st0, AdvStage0* ast0)
{
    const Scene& ctxt = c.ctxt;
    GenerateSampleRayAndDisc(info, ray, path.sampler, c.cfg.line_width, c.pixel_width);
    Blend ab;
    int32_t depth = 0;
    while (depth < maxDepth) {
        bool cont = true;
        Isect isect;
        path.isHit = false;
        const Ray q = ray;
        if (TraverseClosest(isect, ctxt, q, EPS, INF, nullptr)) {
            ShadeSampleRay(c, depth, q, isect, path, info, lo);
            path.isHit = true;
            // what the stage shows of a path a line ended: the state in front of the advance (the device does not advance such a path;
            // nothing of the advance can be seen once the path is over)
            if (depth == 0 && ast0) { *ast0 = AdvStage0{}; ast0->answer = isect.tri_id; ast0->singular = path.is_singular; ast0->ab = ab; ast0->mtrl = isect.mtrlid; }
            const bool ended_by_line = path.is_terminated;
            AdvRec ar;
            AdvanceNPRPath(ctxt, path, ab, ray, isect, ar);
            if (depth == 0 && ast0 && !ended_by_line) {
                ast0->ar = ar; ast0->answer = path.isHit ? isect.tri_id : -1; ast0->singular = path.is_singular; ast0->ab = ab;
            }
            if (path.isHit) {
                ShadeBlend(path, ab, ctxt, ray, shadow_ray, isect, rrDepth, depth);
                HitShadowRay(ctxt, path, shadow_ray, isect.mtrlid >= 0 ? ctxt.GetMaterial(isect.mtrlid).stencil_type : 0, nullptr);
            }
            cont = !path.is_terminated;
        }
        else {
            ShadeMissSampleRay(c, depth, q, path, info, lo);
            ShadeMissBlend(ix, iy, w, h, depth, ctxt, c.cam, path, ab, ray);
            cont = false;
            if (depth == 0 && ast0) *ast0 = AdvStage0{};
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

} // namespace

extern "C" {

// orc_npr_render's frame (one pass of the sample loop) with the advance; the same handle, film rules and stage outputs, and
// adv float4[n][2] {kind, walks, answer, is_singular} {alpha_blend.throughput, transmission} after bounce 0 of the last sample
// (atn_npr_advance_download's layout); cat float4[n] {CheckStencil's verdict, how the alpha look-through ended, the literal re-walk gave
// the last walk's answer, the primary hit's material id} (AdvRec)
int orc_npra_render(void* h, const atn_scene_desc* scene, const atn_camera_param* camera, const uint32_t* seeds, uint32_t n_seeds,
                    const orc_destination* dst, int32_t break_on_terminate, atn_vec4* film,
                    atn_vec4* line, atn_vec4* desc, atn_vec4* disc, uint32_t* dims, atn_vec4* adv, atn_vec4* cat)
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

#pragma omp parallel for schedule(dynamic, 4)
    for (int32_t y = 0; y < height; y++) {
        for (int32_t x = 0; x < width; x++) {
            const int32_t idx = y * width + x;
            LineOut lo;
            Stage0 st0{};
            AdvStage0 ast0;
            v3 col(0); uint32_t cnt = 0;
            PathState path; path.samples = 0;
            for (uint32_t i = 0; i < samples; i++) {
                Ray ray; ShadowRay shadow_ray;
                GeneratePath(ray, x, y, (int32_t)i, dst->frame, path, *camera, seeds[idx % n_seeds]);
                path.contrib = v3(0);
                RadianceWithAdvance(c, path, ray, shadow_ray, x, y, width, height, maxDepth, rrDepth, S.infos[idx], lo, &st0, &ast0);
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
            if (line) line[idx] = lo.found ? atn_vec4{ 1.0F, (float)lo.bounce, lo.distance, 0.0F } : atn_vec4{ 0, 0, 0, 0 };
            if (desc) for (int k = 0; k < kRays; k++) desc[(size_t)idx * kRays + k] = atn_vec4{ st0.u[k], st0.v[k], (float)st0.live[k], st0.term ? 1.0F : 0.0F };
            if (disc) {
                disc[2 * (size_t)idx] = atn_vec4{ st0.disc.center.x, st0.disc.center.y, st0.disc.center.z, st0.disc.radius };
                disc[2 * (size_t)idx + 1] = atn_vec4{ st0.disc.normal.x, st0.disc.normal.y, st0.disc.normal.z, st0.disc.accumulated_distance };
            }
            if (dims) dims[idx] = st0.dim;
            if (adv) {
                adv[2 * (size_t)idx] = atn_vec4{ (float)ast0.ar.kind, (float)ast0.ar.walks, (float)ast0.answer, ast0.singular ? 1.0F : 0.0F };
                adv[2 * (size_t)idx + 1] = atn_vec4{ ast0.ab.throughput.x, ast0.ab.throughput.y, ast0.ab.throughput.z, ast0.ab.transmission };
            }
            if (cat) cat[idx] = atn_vec4{ (float)ast0.ar.stencil_verdict, (float)ast0.ar.alpha_end, ast0.ar.rewalk_same ? 1.0F : 0.0F, (float)ast0.mtrl };
        }
    }
    return 0;
}

} // extern "C"
