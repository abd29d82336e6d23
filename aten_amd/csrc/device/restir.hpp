// ReSTIR direct lighting at the primary hit (the reference's third renderer: aten::ReSTIRRenderer, src/libaten/renderer/restir/,
// and idaten::ReSTIRPathTracing, src/libidaten/restir/).  The per-pixel functions of restir_impl.h as full-frame HIP kernels,
// run inside the serial sample loop between shade(0) and shade(1):
//
//   gen_path -> trace_closest(0) -> k_restir_shade -> k_restir_vis_prep -> [visibility rays + trace_closest(1)]
//            -> k_restir_temporal -> k_restir_spatial (+ pixel colour) | k_restir_color -> k_shade(1) -> ... (the path tracer)
//
// The visibility rays ride in the shadow half of the fused launch that traces bounce 1's closest rays (k_trace_fused, the
// untouched ShadowJob): their "light contribution" is (1, 1, 1) and the plane it is added to is RestirArgs::vis, not the path's
// contrib, so a visible light leaves vis[slot].x = 1 and the path's own radiance is not touched (docs/RESTIR.md: lightcontrib).
//
// Reservoirs and infos are device-private SoA float4 planes indexed by pixel (idx = x + y * width, row 0 = bottom), two sets
// each (ReuseParams, restir_types.h:117-168): `cur` is written by this frame's shade and temporal pass, the other set holds the
// previous frame's reservoirs for the temporal pass and receives the spatial pass's output.
#pragma once
#include "kernels.hpp"
#include "svgf_frame.hpp"

namespace atn {

// Reservoir (restir_types.h:10-78) + its LightSampleResult
//   res[0] : w_sum, M (int bits), y (int bits), W
//   res[1] : target_pdf_of_y, light_sample.pos.xyz
//   res[2] : light_sample.dir.xyz, dist_to_light
//   res[3] : light_sample.nml.xyz, light_color.x
//   res[4] : light_color.y, light_color.z, -, -
// ReSTIRInfo (restir_types.h:84-115); throughput is (1, 1, 1) at bounce 0 and not kept, point_to_light is never read
// (ComputePixelColor computes two cosines from it that it does not use)
//   info[0] : nml.xyz, mtrl_idx (int bits)
//   info[1] : wi.xyz, u
//   info[2] : p.xyz, v
//   info[3] : pre_sampled_r, mesh_id (int bits), -, -
constexpr int kRestirResPlanes = 5, kRestirInfoPlanes = 4;

struct RestirSet {
    float4* res[kRestirResPlanes];
    float4* info[kRestirInfoPlanes];
};

struct RestirArgs {
    RestirSet cur, other;       // other: the previous frame's set (temporal) and the spatial destination
    float4* nd;                 // AOV normal.xyz, clip w        (restir.cpp:151-158)
    float4* am;                 // AOV albedo.rgb, mesh id
    float4* motion;             // motion.xy, depth, 1 (external or computed from the primary hits)
    float4* vis;                // [slots] x = 1 when the visibility ray reached the light
    float w2c3[4];              // fourth row of mtx_W2C
    float w2c[16], prev_w2c[16];    // the motion pass's matrices (compute_motion)
    int32_t n_candidates;       // GenerateInitialCandidate's MaxLightCount
    float4* stage_res;          // optional: [3 stages][2 planes][pixels] res[0], res[1] after shade, temporal, spatial
    float* dims;                // optional: [pixels] CMJ dimension of the pixel after bounce 0's passes
};

struct Reservoir {
    float w_sum; int32_t M, y; float W, target_pdf;
    LightSample ls;
};

ATN_DEV void res_clear(Reservoir& r) { r.w_sum = 0.0F; r.M = 0; r.y = -1; r.target_pdf = 0.0F; r.W = 0.0F; }

// Reservoir::update, restir_types.h:49-61
ATN_DEV bool res_update(Reservoir& r, const LightSample& ls, int32_t sample, float weight, int32_t m, float u)
{
    r.w_sum += weight;
    const bool accepted = u < weight / r.w_sum;
    if (accepted) { r.ls = ls; r.y = sample; }
    r.M += m;
    return accepted;
}

ATN_DEV void reservoir_put(const RestirSet& s, uint32_t idx, const Reservoir& r, bool with_sample)
{
    s.res[0][idx] = make_float4(r.w_sum, __int_as_float(r.M), __int_as_float(r.y), r.W);
    if (!with_sample) { s.res[1][idx].x = r.target_pdf; return; }
    s.res[1][idx] = make_float4(r.target_pdf, r.ls.pos.x, r.ls.pos.y, r.ls.pos.z);
    s.res[2][idx] = make_float4(r.ls.dir.x, r.ls.dir.y, r.ls.dir.z, r.ls.dist);
    s.res[3][idx] = make_float4(r.ls.nml.x, r.ls.nml.y, r.ls.nml.z, r.ls.color.x);
    s.res[4][idx] = make_float4(r.ls.color.y, r.ls.color.z, 0.0F, 0.0F);
}

ATN_DEV void reservoir_get(const RestirSet& s, uint32_t idx, Reservoir& r)
{
    const float4 a = s.res[0][idx], b = s.res[1][idx], c = s.res[2][idx], d = s.res[3][idx], e = s.res[4][idx];
    r.w_sum = a.x; r.M = __float_as_int(a.y); r.y = __float_as_int(a.z); r.W = a.w;
    r.target_pdf = b.x;
    r.ls.pos = mk3(b.y, b.z, b.w); r.ls.dir = mk3(c); r.ls.dist = c.w;
    r.ls.nml = mk3(d); r.ls.color = mk3(d.w, e.x, e.y);
    r.ls.pdf = 0.0F; r.ls.attrib = 0u;
}

struct RestirInfo { f3 nml, wi, p; int32_t mtrl_idx, mesh_id; float u, v, pre_r; };

ATN_DEV void info_load(const RestirSet& s, uint32_t idx, RestirInfo& in)
{
    const float4 a = s.info[0][idx], b = s.info[1][idx], c = s.info[2][idx], d = s.info[3][idx];
    in.nml = mk3(a); in.mtrl_idx = __float_as_int(a.w);
    in.wi = mk3(b); in.u = b.w;
    in.p = mk3(c); in.v = c.w;
    in.pre_r = d.x; in.mesh_id = __float_as_int(d.y);
}

// FillMaterial (material_impl.h:232-262): a negative id selects the white-diffuse fallback the upload appends, and is "not valid"
ATN_DEV const DevMaterial& restir_material(const DevScene& sc, int32_t mtrl_idx)
{
    return sc.materials[mtrl_idx >= 0 ? mtrl_idx : sc.n_materials];
}

// _detail::ComputeRadiance, restir_impl.h:31-65 (the BSDF with external albedo 1)
template <int MS>
ATN_DEV f3 restir_radiance(const DevScene& sc, const LightSample& ls, uint32_t light_attrib, const f3& normal, const f3& wi,
                           const DevMaterial& m, int32_t mtrl_slot, float u, float v, float pre_r)
{
    const float cosShadow = fabsf(dot(normal, ls.dir));
    const float cosLight = fabsf(dot(ls.nml, -ls.dir));
    const float dist2 = sqr(ls.dist);
    const MtrlSample ev = material_bsdf<MS>(sc, m, normal, wi, ls.dir, u, v, mtrl_slot, pre_r);
    const float G = (light_attrib & (ATN_LIGHT_ATTR_SINGULAR | ATN_LIGHT_ATTR_INFINITE)) ? cosShadow * cosLight : (cosShadow * cosLight) / dist2;
    return (ev.bsdf * ls.color) * G;
}

// _detail::ComputeTargetPDF, restir_impl.h:67-106
template <int MS>
ATN_DEV float restir_target_pdf(const DevScene& sc, const LightSample& ls, uint32_t light_attrib, const f3& normal, const f3& wi,
                                const DevMaterial& m, int32_t mtrl_slot, float u, float v, float pre_r)
{
    const float pdf = material_pdf<MS>(sc, m, normal, wi, ls.dir, u, v, mtrl_slot);
    if (pdf == 0.0F) return 0.0F;
    const f3 e = restir_radiance<MS>(sc, ls, light_attrib, normal, wi, m, mtrl_slot, u, v, pre_r);
    return ((e.x + e.y) + e.z) / 3;
}

// ComputeRussianProbability (pathtracing_impl.h:680-698) and PrepareForNextBounce's throughput update (:700-743), as shade_body
// writes them inline (device/kernels.hpp).  shade_body does not call these: routed through them, its kernels are scheduled
// differently (the k_shade / k_regen_shade / k_shade_relaxed families change instructions, and k_regen_shade_wn<1, 5> spills 37
// registers instead of 44, <0, 5> 23 instead of 21), and the existing kernels are to keep their code (docs/RESTIR.md).
// ComputeRussianProbability: the roulette below rr_depth; returns the survival probability
ATN_DEV float russian_roulette(int32_t bounce, int32_t rr_depth, const f3& throughput, uint32_t& flags, Cmj& smp)
{
    float russian_prob = 1.0f;
    if (bounce > rr_depth) {
        if (dot(throughput, throughput) > 0) {
            russian_prob = max3(throughput);
            const float p = cmj_next(smp);
            if (p >= russian_prob) flags |= F_TERMINATED; else flags &= ~F_TERMINATED;
        }
    }
    return russian_prob;
}

// PrepareForNextBounce (pathtracing_impl.h:700-743) up to the next ray: the throughput update, or the end of the path
ATN_DEV void next_bounce_throughput(const MtrlSample& ms, const f3& orienting_normal, const f3& albedo, float russian_prob, f3& throughput,
                                    uint32_t& flags, f3& next_dir, f3& ray_along_normal)
{
    next_dir = normalize(ms.dir);
    ray_along_normal = dot(orienting_normal, next_dir) >= 0.0f ? orienting_normal : -orienting_normal;
    const float c = dot(ray_along_normal, next_dir);
    if (ms.pdf > 0 && c > 0) {
        throughput = throughput * ((((albedo * ms.bsdf) * c) / ms.pdf));
        if (russian_prob != 1.0F) throughput = throughput / russian_prob;      // (x / 1 is x, bit for bit: three IEEE divisions on every vertex below the roulette depth)
    }
    else {
        flags |= F_TERMINATED;
    }
}

// The path's sampler (GeneratePath's seeding, pathtracing_impl.h:75-81), continued at the dimension its thr.w holds
ATN_DEV Cmj restir_sampler(const PathBuffers& pb, const FrameParams& fp, uint32_t slot, uint32_t pixel)
{
    const uint32_t fs = fp.frame + (uint32_t)fp.sample;
    const uint32_t rnd = pb.seeds[pixel % fp.n_seeds];
    Cmj smp;
    smp.idx = fs % 256u;
    smp.dim = __float_as_uint(pb.thr[slot].w);
    smp.scramble = rnd * 0x1fe3434fu * ((fs + 133u * rnd) / 256u);
    return smp;
}

// pixel -> slot of a one-GPU frame (slot_to_pixel's inverse for world = 1)
ATN_DEV uint32_t restir_slot(const FrameParams& fp, int32_t x, int32_t y)
{
    return ((uint32_t)(y >> 3) * (uint32_t)fp.tiles_x + (uint32_t)(x >> 3)) * 64u + (uint32_t)(y & 7) * 8u + (uint32_t)(x & 7);
}

// The kernels are compiled in restir.hip only (ATN_RESTIR_TU); aten_amd.hip sees the types it fills in.
#ifdef ATN_RESTIR_TU
// ReSTIRRenderer::Shade (restir.cpp:102-238) = idaten's `shade` (restir.cu:36-215) at bounce 0: hit evaluation, normal map, AOVs,
// HitImplicitLight, the initial candidates (GenerateInitialCandidate, restir_impl.h:126-205), Russian roulette, sampleMaterial,
// PrepareForNextBounce.  No NEE: sh_count[0] stays 0.  Misses: ShadeMiss with the AOV spans (FillBasicAOVsIfHitMiss).
// Every path of bounce 0 (= every pixel of the frame) writes its reservoir and info: the frame's InitReSTIR is folded in.
template <int MS>
ATN_DEV void restir_shade_body(const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const atn_camera_param& cam, const RestirArgs& ra)
{
    __shared__ BlockAppendShared sh;
    const uint32_t count = pb.q_count[0];
    for (uint32_t chunk = blockIdx.x * 256u; chunk < count; chunk += gridDim.x * 256u) {
        const uint32_t j = chunk + threadIdx.x;
        bool push_next = false;
        uint32_t slot = 0;
        if (j < count) {
            slot = pb.queue[0][j];
            int32_t ix = 0, iy = 0;
            slot_to_pixel(fp, slot, ix, iy);
            const uint32_t idx = (uint32_t)(iy * fp.width + ix);
            const float4 rd4 = pb.ray_d[slot];
            const f3 ray_dir = mk3(rd4);
            uint32_t flags = __float_as_uint(rd4.w) & ~F_HIT;
            const float4 is4 = pb.isect[slot];
            const int32_t hit_objid = __float_as_int(is4.x);
            f3 throughput = mk3(pb.thr[slot]);
            Cmj smp = restir_sampler(pb, fp, slot, idx);
            // the reservoir of GenerateInitialCandidate while its candidates are drawn: the sample itself is not carried through the
            // loop -- only the accepted light, its target pdf and the sampler dimension its Light::sample started at (CMJ draws are
            // pure functions of index, dimension and scramble), and the light is sampled again from there once the loop is over
            Reservoir r; res_clear(r);
            r.ls.pos = mk3(0.0F); r.ls.dir = mk3(0.0F); r.ls.nml = mk3(0.0F); r.ls.color = mk3(0.0F); r.ls.dist = 0.0F;
            f3 contrib_add = mk3(0.0F);
            bool contrib_changed = false;
            if (hit_objid < 0) {
                // ShadeMiss at bounce 0 (pathtracing_impl.h:112-176) with FillBasicAOVsIfHitMiss (renderer/aov.h:183-198)
                f3 o, dir;
                pinhole_sample(cam, (float)ix / (float)fp.width, (float)iy / (float)fp.height, o, dir);
                const float4 emit = background_sample(sc, dir);
                ra.nd[idx] = make_float4(0.0F, 0.0F, 0.0F, -1.0F);
                ra.am[idx] = make_float4(emit.x, emit.y, emit.z, -1.0F);
                contrib_add = (1.0F * mk3(mul4(1.0f, emit)) + mk3(0.0F)) * throughput;
                contrib_changed = true;
                flags |= F_TERMINATED;
                ra.cur.info[0][idx] = make_float4(0.0F, 0.0F, 0.0F, __int_as_float(-1));
                ra.cur.info[1][idx] = make_float4(0, 0, 0, 0);
                ra.cur.info[2][idx] = make_float4(0, 0, 0, 0);
                ra.cur.info[3][idx] = make_float4(0.0F, __int_as_float(-1), 0.0F, 0.0F);     // (z: 1 on a hit, for the motion pass)
                reservoir_put(ra.cur, idx, r, true);
            }
            else {
                flags |= F_HIT;
                const int32_t tri_id = __float_as_int(is4.w);
                HitRec rec;
                evaluate_hit(rec, sc, hit_objid, tri_id, is4.y, is4.z);
                const int32_t mtrlid = triangle_mtrlid(sc, tri_id);
                const int32_t prim_mesh = sc.tris[tri_id].mesh_id;
                const int32_t mesh_id = prim_mesh < 0 ? -1 : prim_mesh;
                const bool isBackfacing = dot(rec.normal, -ray_dir) < 0.0F;
                f3 orienting_normal = rec.normal;
                const int32_t mtrl_slot = mtrlid >= 0 ? mtrlid : sc.n_materials;
                const DevMaterial& m = sc.materials[mtrl_slot];
                const float4 albedo4 = sample_texture(sc, m.albedoMap, rec.u, rec.v, make_float4(1.0F, 1.0F, 1.0F, 1.0F));
                const f3 albedo = mk3(albedo4);
                // material::applyNormal BEFORE the back-face flip, and the flip spares emissive surfaces (restir.cpp:135-151)
                const float pre_r = apply_normal<MS>(sc, m, mtrl_slot, orienting_normal, rec.u, rec.v, ray_dir, smp);
                if (!(m.attrib & ATN_MTRL_ATTR_TRANSLUCENT) && !(m.attrib & ATN_MTRL_ATTR_EMISSIVE) && isBackfacing) orienting_normal = -orienting_normal;
                ra.cur.info[0][idx] = make_float4(orienting_normal.x, orienting_normal.y, orienting_normal.z, __int_as_float(mtrlid));
                ra.cur.info[1][idx] = make_float4(ray_dir.x, ray_dir.y, ray_dir.z, rec.u);
                ra.cur.info[2][idx] = make_float4(rec.p.x, rec.p.y, rec.p.z, rec.v);
                ra.cur.info[3][idx] = make_float4(pre_r, __int_as_float(mesh_id), 1.0F, 0.0F);
                const float depth = ra.w2c3[0] * rec.p.x + ra.w2c3[1] * rec.p.y + ra.w2c3[2] * rec.p.z + ra.w2c3[3] * 1.0F;
                ra.nd[idx] = make_float4(orienting_normal.x, orienting_normal.y, orienting_normal.z, depth);
                ra.am[idx] = make_float4(albedo.x, albedo.y, albedo.z, (float)mesh_id);
                // HitImplicitLight, pathtracing_impl.h:395-434 (bounce 0: weight 1)
                if (m.type == ATN_MTRL_EMISSIVE && (m.attrib & ATN_MTRL_ATTR_EMISSIVE) && !isBackfacing) {
                    const int32_t lid = sc.objects[hit_objid].light_id;
                    const f3 light_color = (lid >= 0 && lid < sc.n_lights) ? area_light_color(sc.lights[lid], rec.area) : mk3(0.0F);
                    contrib_add = (throughput * 1.0f) * light_color; contrib_changed = true;
                    flags |= F_TERMINATED;
                    reservoir_put(ra.cur, idx, r, true);
                }
                else {
                    // The candidates' draws come first in the sample stream (restir.cpp:196-227), but nothing of them is needed by
                    // the roulette and the BSDF sample: here only their DIMENSIONS are stepped over (the light pick, as many as
                    // Light::sample consumes, the acceptance draw), the next ray is made, and the candidates are evaluated at the end
                    // from the saved dimension, when the BSDF block's registers are dead -- as k_shade does with NEE.  CMJ draws are
                    // pure functions of index, dimension and scramble: the same bits.
                    const bool candidates = !(m.attrib & (ATN_MTRL_ATTR_SINGULAR | ATN_MTRL_ATTR_TRANSLUCENT));
                    const int32_t n_lights = sc.n_lights;
                    const int32_t light_cnt = candidates ? (ra.n_candidates < n_lights ? ra.n_candidates : n_lights) : 0;
                    const uint32_t cand_dim = smp.dim;
                    for (int32_t i = 0; i < light_cnt; i++) {
                        int32_t light_pos = (int32_t)(cmj_next(smp) * (float)n_lights);
                        light_pos = light_pos < 0 ? 0 : (light_pos > n_lights - 1 ? n_lights - 1 : light_pos);
                        smp.dim += light_sample_draws(sc.lights[light_pos], sc) + 1u;
                    }
                    const float russian_prob = russian_roulette(0, fp.rr_depth, throughput, flags, smp);
                    // sampleMaterial + PrepareForNextBounce, pathtracing_impl.h:700-743 (albedo: the texture with default 1)
                    {
                        HitPre hp;      // (what the BSDF sample shares with the vertex, as in k_shade)
                        tangent_coordinate(orienting_normal, hp.t, hp.b);
                        hp.rough = ggx_roughness(sc, m, rec.u, rec.v);
                        hp.lambda_v = m.type == ATN_MTRL_GGX ? ggx_lambda(hp.rough, -ray_dir, orienting_normal) : 0.0F;
                        MtrlSample ms;
                        sample_material<MS>(ms, sc, m, orienting_normal, ray_dir, smp, rec.u, rec.v, mtrl_slot, pre_r, &hp);
                        f3 next_dir, ray_along_normal;
                        next_bounce_throughput(ms, orienting_normal, albedo, russian_prob, throughput, flags, next_dir, ray_along_normal);
                        if (!(flags & F_TERMINATED)) {
                            flags = (m.attrib & ATN_MTRL_ATTR_SINGULAR) ? (flags | F_SINGULAR) : (flags & ~F_SINGULAR);
                            const f3 no = ray_offset(rec.p, ray_along_normal);
                            const f3 nd = normalize(next_dir);
                            pb.ray_o[slot] = make_float4(no.x, no.y, no.z, ms.pdf);
                            pb.ray_d[slot] = make_float4(nd.x, nd.y, nd.z, __uint_as_float(flags));
                            push_next = 1 < fp.max_depth;
                        }
                    }
                    pb.thr[slot] = make_float4(throughput.x, throughput.y, throughput.z, __uint_as_float(smp.dim));
                    if (candidates) {
                        // GenerateInitialCandidate, restir_impl.h:126-205.  The reservoir's sample is not carried through the loop
                        // either: only the accepted light, its target pdf and the dimension its Light::sample started at; the light
                        // is sampled again from there once the loop is over.
                        Cmj cs; cs.idx = smp.idx; cs.dim = cand_dim; cs.scramble = smp.scramble;
                        const float light_select_prob = sc.inv_n_lights;
                        float candidate_target_pdf = 0.0F;
                        uint32_t y_dim = 0u;
                        for (int32_t i = 0; i < light_cnt; i++) {
                            int32_t light_pos = (int32_t)(cmj_next(cs) * (float)n_lights);
                            light_pos = light_pos < 0 ? 0 : (light_pos > n_lights - 1 ? n_lights - 1 : light_pos);
                            const atn_light_param& lp = sc.lights[light_pos];
                            const uint32_t ls_dim = cs.dim;
                            LightSample ls;
                            sample_light(ls, lp, sc, rec.p, orienting_normal, cs);
                            const float sampling_pdf = ls.pdf * light_select_prob;
                            const float target_pdf = restir_target_pdf<MS>(sc, ls, lp.attrib, orienting_normal, ray_dir, m, mtrl_slot, rec.u, rec.v, pre_r);
                            const float weight = sampling_pdf > 0 ? target_pdf / sampling_pdf : 0.0f;
                            const float u = cmj_next(cs);
                            // Reservoir::update (restir_types.h:49-61) without the sample
                            r.w_sum += weight;
                            if (u < weight / r.w_sum) { r.y = light_pos; y_dim = ls_dim; candidate_target_pdf = target_pdf; }
                            r.M += 1;
                        }
                        if (candidate_target_pdf > 0.0F) {
                            r.target_pdf = candidate_target_pdf;
                            r.W = r.w_sum / (r.target_pdf * (float)r.M);
                        }
                        if (!isfinite(r.W)) res_clear(r);
                        if (r.y >= 0) {
                            Cmj sl; sl.idx = smp.idx; sl.dim = y_dim; sl.scramble = smp.scramble;
                            sample_light(r.ls, sc.lights[r.y], sc, rec.p, orienting_normal, sl);
                        }
                    }
                    reservoir_put(ra.cur, idx, r, true);
                }
            }
            if (flags & F_TERMINATED) pb.ray_d[slot] = make_float4(rd4.x, rd4.y, rd4.z, __uint_as_float(flags));
            if (!(flags & F_HIT) || (flags & F_TERMINATED)) pb.thr[slot] = make_float4(throughput.x, throughput.y, throughput.z, __uint_as_float(smp.dim));
            if (contrib_changed) {
                const f3 c = mk3(pb.contrib[slot]) + contrib_add;
                pb.contrib[slot] = make_float4(c.x, c.y, c.z, 0.0F);
            }
            if (ra.stage_res) {
                const size_t n = (size_t)fp.width * fp.height;
                ra.stage_res[idx] = ra.cur.res[0][idx];
                ra.stage_res[n + idx] = ra.cur.res[1][idx];
            }
        }
        block_append2(sh, pb.queue[1], &pb.q_count[1], push_next ? 1u : 0u, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u,
                      [&](int) { return slot; });
    }
}

// The core and Disney sets fit 128 VGPRs without a spill: held there, 4 waves per SIMD.  The analytic and car-paint sets need
// 150 / 163 (held to 128 they spill 12 / 25 registers): they keep their natural allocation, 3 waves per SIMD (docs/RESTIR.md).
template <int MS>
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) __launch_bounds__(256) k_restir_shade(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, RestirArgs ra)
{
    restir_shade_body<MS>(pb, sc, fp, cam, ra);
}
template <int MS>
__global__ void __launch_bounds__(256) k_restir_shade_wide(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, RestirArgs ra)
{
    restir_shade_body<MS>(pb, sc, fp, cam, ra);
}

// EvaluateVisibility's shadow ray (restir_impl.h:218-261): one per valid reservoir, from p + AT_MATH_EPSILON * nml to the sampled
// light position, into bounce 0's shadow queue.  Every slot's vis entry is cleared first; a path terminated at bounce 0 casts none
// (HitShadowRay's is_terminated test) and so counts as occluded.
__global__ void __launch_bounds__(256) k_restir_vis_prep(PathBuffers pb, DevScene sc, FrameParams fp, RestirArgs ra)
{
    __shared__ BlockAppendShared sh;
    const uint32_t n = (uint32_t)fp.n_slots;
    for (uint32_t chunk = blockIdx.x * 256u; chunk < n; chunk += gridDim.x * 256u) {
        const uint32_t slot = chunk + threadIdx.x;
        bool push = false;
        int32_t ix = 0, iy = 0;
        if (slot < n && slot_to_pixel(fp, slot, ix, iy)) {
            ra.vis[slot] = make_float4(0.0F, 0.0F, 0.0F, 0.0F);
            const uint32_t idx = (uint32_t)(iy * fp.width + ix);
            const uint32_t flags = __float_as_uint(pb.ray_d[slot].w);
            const float4 a = ra.cur.res[0][idx];
            const int32_t y = __float_as_int(a.z);
            if (!(flags & F_TERMINATED) && y >= 0) {
                const float4 b = ra.cur.res[1][idx], i0 = ra.cur.info[0][idx], i2 = ra.cur.info[2][idx];
                const f3 nml = mk3(i0), p = mk3(i2);
                const f3 org = p + kEps * nml;
                f3 dir = mk3(b.y, b.z, b.w) - org;
                const float dist = length(dir);
                dir = dir / dist;
                const DevMaterial& m = restir_material(sc, __float_as_int(i0.w));
                const float lbits = __uint_as_float((uint32_t)y | ((m.attrib & kAttrStencilAlways) ? kShadowStencilFlag : 0u));
                pb.sh_o[slot] = make_float4(org.x, org.y, org.z, dist);
                pb.sh_d[slot] = make_float4(dir.x, dir.y, dir.z, lbits);
                pb.sh_c[slot] = make_float4(1.0F, 1.0F, 1.0F, lbits);
                push = true;
            }
        }
        block_append2(sh, pb.shadow_q, &pb.sh_count[0], push ? 1u : 0u, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u,
                      [&](int) { return slot; });
    }
}

// IsAcceptableNeighbor, restir_impl.h:275-289
ATN_DEV bool restir_acceptable(int32_t type, int32_t mesh_id, const f3& normal, int32_t n_type, int32_t n_mesh_id, const f3& n_normal)
{
    return type == n_type && mesh_id == n_mesh_id && dot(normal, n_normal) >= 0.95f;
}

ATN_DEV bool restir_pixel(const FrameParams& fp, int32_t& ix, int32_t& iy)
{
    ix = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    iy = (int32_t)(blockIdx.y * blockDim.y + threadIdx.y);
    return ix < fp.width && iy < fp.height;
}

// The rest of EvaluateVisibility (an occluded or unsampled reservoir keeps M and loses the rest), then ApplyTemporalReuse
// (restir_impl.h:309-428) when TEMPORAL.  Every pixel gets the visibility step; the temporal step skips terminated paths.
template <int MS, bool TEMPORAL>
__global__ void __launch_bounds__(256) k_restir_temporal(PathBuffers pb, DevScene sc, FrameParams fp, RestirArgs ra)
{
    int32_t ix, iy;
    if (!restir_pixel(fp, ix, iy)) return;
    const uint32_t idx = (uint32_t)(iy * fp.width + ix);
    const uint32_t slot = restir_slot(fp, ix, iy);
    float4 a = ra.cur.res[0][idx];
    if (!(__float_as_int(a.z) >= 0 && ra.vis[slot].x != 0.0F)) {
        a = make_float4(0.0F, a.y, __int_as_float(-1), 0.0F);
        ra.cur.res[0][idx] = a;
        ra.cur.res[1][idx].x = 0.0F;
    }
    const uint32_t flags = __float_as_uint(pb.ray_d[slot].w);
    if (TEMPORAL && !(flags & F_TERMINATED)) {
        Reservoir r; reservoir_get(ra.cur, idx, r);
        RestirInfo self; info_load(ra.cur, idx, self);
        const DevMaterial& m = restir_material(sc, self.mtrl_idx);
        const int32_t mtrl_slot = self.mtrl_idx >= 0 ? self.mtrl_idx : sc.n_materials;
        const int32_t mesh_id = (int32_t)ra.am[idx].w;
        float candidate_target_pdf = r.y >= 0 ? r.target_pdf : 0.0F;
        const int32_t maxM = 20 * r.M;
        const float4 md = ra.motion[idx];
        const int32_t px = (int32_t)((float)ix + md.x * (float)fp.width);
        const int32_t py = (int32_t)((float)iy + md.y * (float)fp.height);
        Cmj smp = restir_sampler(pb, fp, slot, idx);
        bool wrote_sample = false;
        if (px >= 0 && px <= fp.width - 1 && py >= 0 && py <= fp.height - 1) {
            const uint32_t nidx = (uint32_t)(py * fp.width + px);
            const float4 na = ra.other.res[0][nidx];
            const int32_t nM = __float_as_int(na.y), ny = __float_as_int(na.z);
            const int32_t mm = nM < maxM ? nM : maxM;
            if (ny >= 0 && ny < sc.n_lights) {       // (a light of the previous frame's scene that is gone counts as no sample)
                const float4 ni0 = ra.other.info[0][nidx];
                const int32_t n_mtrl = __float_as_int(ni0.w);
                const f3 n_normal = mk3(ni0);
                const int32_t n_mesh = __float_as_int(ra.other.info[3][nidx].y);
                const bool ok = n_mtrl >= 0 && restir_acceptable(m.type, mesh_id, self.nml, restir_material(sc, n_mtrl).type, n_mesh, n_normal);
                if (ok) {
                    const atn_light_param& lp = sc.lights[ny];
                    LightSample ls;
                    sample_light(ls, lp, sc, self.p, n_normal, smp);
                    const float target_pdf = restir_target_pdf<MS>(sc, ls, lp.attrib, self.nml, self.wi, m, mtrl_slot, self.u, self.v, self.pre_r);
                    const float weight = (target_pdf * na.w) * (float)mm;
                    const float u = cmj_next(smp);
                    if (res_update(r, ls, ny, weight, mm, u)) { candidate_target_pdf = target_pdf; wrote_sample = true; }
                }
            }
            else {
                LightSample dummy;
                res_update(r, dummy, -1, 0.0f, mm, 0.0f);       // never accepted (0 < 0 / w_sum is false): M += m
            }
        }
        if (candidate_target_pdf > 0.0F) {
            r.target_pdf = candidate_target_pdf;
            r.W = r.w_sum / (r.target_pdf * (float)r.M);
        }
        if (!isfinite(r.W)) res_clear(r);
        reservoir_put(ra.cur, idx, r, wrote_sample);
        pb.thr[slot].w = __uint_as_float(smp.dim);
    }
    if (ra.stage_res) {
        const size_t n = (size_t)fp.width * fp.height;
        ra.stage_res[2 * n + idx] = ra.cur.res[0][idx];
        ra.stage_res[3 * n + idx] = ra.cur.res[1][idx];
    }
}

// ComputePixelColor, restir_impl.h:582-621, times the bounce-0 throughput (1) into the path's contribution (restir.cpp:440-470)
template <int MS>
ATN_DEV void restir_pixel_color(const PathBuffers& pb, const DevScene& sc, const RestirArgs& ra, uint32_t slot, uint32_t idx,
                                const Reservoir& r, const RestirInfo& in)
{
    if (r.y < 0) return;
    const DevMaterial& m = restir_material(sc, in.mtrl_idx);
    const int32_t mtrl_slot = in.mtrl_idx >= 0 ? in.mtrl_idx : sc.n_materials;
    const f3 le = restir_radiance<MS>(sc, r.ls, sc.lights[r.y].attrib, in.nml, in.wi, m, mtrl_slot, in.u, in.v, in.pre_r);
    const float4 alb = ra.am[idx];
    f3 c = le * r.W;
    c = c * mk3(alb.x, alb.y, alb.z);
    const f3 cur = mk3(pb.contrib[slot]) + c * mk3(1.0F);
    pb.contrib[slot] = make_float4(cur.x, cur.y, cur.z, 0.0F);
}

ATN_DEV void restir_dims(const PathBuffers& pb, const RestirArgs& ra, uint32_t slot, uint32_t idx)
{
    if (ra.dims) ra.dims[idx] = (float)__float_as_uint(pb.thr[slot].w);
}

// ApplySpatialReuse (restir_impl.h:445-569) over the 3 x 3 neighbourhood of the current set into the other set, then the pixel
// colour from the combined reservoir.  2-D blocks of 16 x 16: the taps of a block are mostly its own pixels.
template <int MS>
__global__ void __launch_bounds__(256) k_restir_spatial(PathBuffers pb, DevScene sc, FrameParams fp, RestirArgs ra)
{
    int32_t ix, iy;
    if (!restir_pixel(fp, ix, iy)) return;
    const uint32_t idx = (uint32_t)(iy * fp.width + ix);
    const uint32_t slot = restir_slot(fp, ix, iy);
    const uint32_t flags = __float_as_uint(pb.ray_d[slot].w);
    if (flags & F_TERMINATED) { restir_dims(pb, ra, slot, idx); return; }
    RestirInfo self; info_load(ra.cur, idx, self);
    const DevMaterial& m = restir_material(sc, self.mtrl_idx);
    const int32_t mtrl_slot = self.mtrl_idx >= 0 ? self.mtrl_idx : sc.n_materials;
    const int32_t mesh_id = (int32_t)ra.am[idx].w;
    Cmj smp = restir_sampler(pb, fp, slot, idx);
    Reservoir r; res_clear(r);
    r.ls.pos = mk3(0.0F); r.ls.dir = mk3(0.0F); r.ls.nml = mk3(0.0F); r.ls.color = mk3(0.0F); r.ls.dist = 0.0F;
    float candidate_target_pdf = 0.0F;
    int32_t M_sum = 0;
    for (int32_t i = 0; i < 9; i++) {
        const int32_t xx = ix + (i % 3) - 1, yy = iy + (i / 3) - 1;
        if (xx < 0 || xx > fp.width - 1 || yy < 0 || yy > fp.height - 1) continue;
        const uint32_t nidx = (uint32_t)(yy * fp.width + xx);
        const float4 na = ra.cur.res[0][nidx];
        const int32_t nM = __float_as_int(na.y), ny = __float_as_int(na.z);
        M_sum += nM;
        if (ny < 0) continue;
        const float4 ni0 = ra.cur.info[0][nidx];
        const int32_t n_mtrl = __float_as_int(ni0.w);
        const f3 n_normal = mk3(ni0);
        const int32_t n_mesh = (int32_t)ra.am[nidx].w;
        if (!(n_mtrl >= 0 && restir_acceptable(m.type, mesh_id, self.nml, restir_material(sc, n_mtrl).type, n_mesh, n_normal))) continue;
        const atn_light_param& lp = sc.lights[ny];
        LightSample ls;
        sample_light(ls, lp, sc, self.p, n_normal, smp);
        const float target_pdf = restir_target_pdf<MS>(sc, ls, lp.attrib, self.nml, self.wi, m, mtrl_slot, self.u, self.v, self.pre_r);
        const float weight = (target_pdf * na.w) * (float)nM;
        const float u = cmj_next(smp);
        if (res_update(r, ls, ny, weight, nM, u)) candidate_target_pdf = target_pdf;
    }
    r.M = M_sum;
    if (candidate_target_pdf > 0.0F) {
        r.target_pdf = candidate_target_pdf;
        r.W = r.w_sum / (r.target_pdf * (float)r.M);
    }
    if (!isfinite(r.W)) res_clear(r);
    reservoir_put(ra.other, idx, r, true);
    if (ra.stage_res) {
        const size_t n = (size_t)fp.width * fp.height;
        ra.stage_res[4 * n + idx] = ra.other.res[0][idx];
        ra.stage_res[5 * n + idx] = ra.other.res[1][idx];
    }
    pb.thr[slot].w = __uint_as_float(smp.dim);
    restir_pixel_color<MS>(pb, sc, ra, slot, idx, r, self);
    restir_dims(pb, ra, slot, idx);
}

// The pixel colour from the current set (modes 0 and 3: no spatial pass)
template <int MS>
__global__ void __launch_bounds__(256) k_restir_color(PathBuffers pb, DevScene sc, FrameParams fp, RestirArgs ra)
{
    int32_t ix, iy;
    if (!restir_pixel(fp, ix, iy)) return;
    const uint32_t idx = (uint32_t)(iy * fp.width + ix);
    const uint32_t slot = restir_slot(fp, ix, iy);
    const uint32_t flags = __float_as_uint(pb.ray_d[slot].w);
    if (!(flags & F_TERMINATED)) {
        Reservoir r; reservoir_get(ra.cur, idx, r);
        RestirInfo self; info_load(ra.cur, idx, self);
        restir_pixel_color<MS>(pb, sc, ra, slot, idx, r, self);
    }
    restir_dims(pb, ra, slot, idx);
}

// SVGF's motion pass (motion_depth) from the bounce-0 hit positions (info[2]; info[3].z = 1 on a hit)
__global__ void __launch_bounds__(256) k_restir_motion(FrameParams fp, RestirArgs ra)
{
    int32_t ix, iy;
    if (!restir_pixel(fp, ix, iy)) return;
    const uint32_t idx = (uint32_t)(iy * fp.width + ix);
    const float4 p = ra.cur.info[2][idx];
    ra.motion[idx] = motion_depth(ra.w2c, ra.prev_w2c, make_float4(p.x, p.y, p.z, ra.cur.info[3][idx].z));
}

#endif  // ATN_RESTIR_TU

} // namespace atn
