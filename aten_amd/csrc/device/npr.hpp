// NPR feature lines (aten::NprPathTracer::radiance_with_feature_line, src/libaten/renderer/npr/npr.cpp:101-200, npr_impl.h,
// feature_line.h; the frame shape of idaten::NPRPathTracing, src/libidaten/npr/npr_pathtracing.cu:388-517): the path tracer's
// sample loop with 8 sample rays per path that walk a cone of discs around the path's query ray.  docs/NPR.md has the decisions.
//
// Per sample:  k_gen_path -> k_npr_gen (disc 0 + the 8 disc draws) -> per bounce b:
//   trace(b) -> k_npr_prep (disc at the query hit, the next sample rays, compacted) -> k_npr_trace (the renderer's walk over them)
//   -> k_npr_eval (metrics, closest feature-line point, line colour; a path with a line is terminated and left out of the queue
//   k_shade reads) -> k_npr_commit -> k_shade
//
// State, SoA, indexed by path slot s (per path) or 8 s + k (per sample ray k); only what a later kernel reads:
//   disc_c / disc_n   float4: center.xyz, radius / normal.xyz, accumulated_distance            32 B per path
//   desc_p / desc_n   float4: prev_ray_hit_pos.xyz, u / prev_ray_hit_nml.xyz, v                 32 B per sample ray
//   live              uint32: bit k = sample ray k is not terminated; kNprEval = the path is evaluated this bounce
//   work              uint32: the path's first ray in the bounce's ray list (bits 0-27), its ray count (bits 28-31)
//   hpd               float:  hit_point_distance of this bounce (added to the accumulated distance after the eval)
//   ray_o / ray_d / ray_hit  float4: org.xyz, - / dir.xyz, k / the walk's answer {objid, a, b, tri}  48 B per listed ray
#pragma once
#include "kernels.hpp"

namespace atn {

constexpr int kNprRays = 8;                 // SampleRayNum, npr_pathtracing.h:12
constexpr uint32_t kNprEval = 0x100u;
constexpr uint32_t kNprMetricMesh = 1u, kNprMetricAlbedo = 2u, kNprMetricNormal = 4u, kNprMetricDepth = 8u;   // FeatureLineMetricFlag
constexpr int kNprCounters = 4;             // per bounce: 0 rays listed, 1 the walk's fetch cursor, 2 paths left for k_shade

struct NprArgs {
    float4* disc_c; float4* disc_n;
    float4* desc_p; float4* desc_n;
    uint32_t* live; uint32_t* work; float* hpd;
    float4* ray_o; float4* ray_d; float4* ray_hit;
    uint32_t* counters;         // [kNprCounters * bounce + i]
    uint32_t* queue;            // the bounce's queue without the paths a line terminated
    const uint32_t* mflags;     // per material (+ the fallback): FeatureLineMtrlConfig.enable (bit 0) | metric_flag << 8
    float line_color[3];
    float line_width, albedo_threshold, normal_threshold;
    float pixel_width;          // Camera::ComputePixelWidthAtDistance(camera, 1), computed on the host
    // stage buffers (atn_npr_capture; null = off), per pixel
    float4* st_line;            // found, bounce, closest distance, - (the frame's last sample that found a line)
    float4* st_desc;            // [8 n]: u, v, live after bounce 0, -
    float4* st_disc;            // [2 n]: the disc after bounce 0
    uint32_t* st_dims;          // CMJ dimension after bounce 0
};

struct NprDisc { f3 center; float radius; f3 normal; float acc; };

ATN_DEV NprDisc npr_load_disc(const NprArgs& na, uint32_t slot)
{
    const float4 c = na.disc_c[slot], n = na.disc_n[slot];
    NprDisc d; d.center = mk3(c); d.radius = c.w; d.normal = mk3(n); d.acc = n.w;
    return d;
}
ATN_DEV void npr_store_disc(const NprArgs& na, uint32_t slot, const NprDisc& d)
{
    na.disc_c[slot] = make_float4(d.center.x, d.center.y, d.center.z, d.radius);
    na.disc_n[slot] = make_float4(d.normal.x, d.normal.y, d.normal.z, d.acc);
}

// CMJ::nextSample2D (cmj.h:39-44,103-114): both components of one dimension
ATN_DEV void cmj_next2d(Cmj& s, float& ox, float& oy)
{
    constexpr int32_t n = 16;
    const uint32_t p = s.dim * s.scramble;
    const int32_t k = (int32_t)cmj_permute(s.idx, n * n, 0xa399d265u * s.dim * s.scramble);
    const int32_t sx = (int32_t)cmj_permute((uint32_t)(k % n), n, p * 0xa511e9b3u);
    const int32_t sy = (int32_t)cmj_permute((uint32_t)(k / n), n, p * 0x63d83595u);
    const float jx = cmj_randfloat((uint32_t)k, p * 0xa399d265u);
    const float jy = cmj_randfloat((uint32_t)k, p * 0x711ad6a5u);
    s.dim++;
    ox = ((float)(k % n) + ((float)sy + jx) / (float)n) / (float)n;
    oy = ((float)(k / n) + ((float)sx + jy) / (float)n) / (float)n;
}

// ---- FeatureLine geometry (feature_line.h) ---------------------------------------------------------------------------------

// ComputeHitPositionOnDisc, :279-305: vec4 (u, v, 0, 1) * radius through mat4(t, b, n).applyXYZ, + center
ATN_DEV f3 npr_disc_pos(float u, float v, const NprDisc& d)
{
    const float px = u * d.radius, py = v * d.radius, pz = 0.0F * d.radius;
    f3 t, b;
    tangent_coordinate(d.normal, t, b);
    const f3 n = d.normal;
    return mk3(((t.x * px + b.x * py) + n.x * pz) + d.center.x, ((t.y * px + b.y * py) + n.y * pz) + d.center.y,
               ((t.z * px + b.z * py) + n.z * pz) + d.center.z);
}

// ComputeRayHitPositionOnPlane, :333-371, plane (n, -dot(n, p)) of ComputePlane (:313-324)
ATN_DEV bool npr_ray_plane(const f3& pn, float pd, const f3& org, const f3& dir, f3& pos)
{
    const float div = ((pn.x * dir.x + pn.y * dir.y) + pn.z * dir.z) + pd * 0.0F;
    if (div == 0.0F) return false;
    float t = ((pn.x * org.x + pn.y * org.y) + pn.z * org.z) + pd * 1.0F;
    t = -t / div;
    pos = org + t * dir;
    return t >= 0.0F;
}

// GenerateDisc, :97-121
ATN_DEV NprDisc npr_first_disc(const f3& org, const f3& dir, float line_width, float pixel_width)
{
    const f3 n = -dir, p = org + dir;
    const float pd = -dot(n, p);
    f3 pos = mk3(0.0F);
    (void)npr_ray_plane(n, pd, org, dir, pos);
    NprDisc d;
    d.center = pos; d.normal = dir; d.radius = line_width * pixel_width; d.acc = 0.0F;
    return d;
}

// ComputeDiscAtQueryRayHitPoint, :133-154
ATN_DEV NprDisc npr_disc_at(const f3& p, const f3& dir, float prev_radius, float cur_dist, float acc_without)
{
    NprDisc d;
    d.center = p;
    const float acc = acc_without + cur_dist;
    d.radius = prev_radius * acc / acc_without;
    d.normal = -dir;
    d.acc = acc_without;
    return d;
}

// ComputeNextSampleRay, :230-269 (false: the ray is dropped)
ATN_DEV bool npr_next_ray(float u, float v, const f3& prev_p, const f3& prev_nml, const NprDisc& prev, const NprDisc& next, f3& org, f3& dir)
{
    const float face = dot(prev.normal, next.normal);
    const f3 pos = npr_disc_pos(face >= 0.0F ? u : -u, v, next);
    const f3 rd = normalize(pos - prev_p);
    if (dot(rd, prev_nml) < 0.0F) return false;
    dir = normalize(rd);            // ray(o, d, n) normalises again (ray.h:17-24)
    org = ray_offset(prev_p, prev_nml);
    return !(isnan(dir.x) || isnan(dir.y) || isnan(dir.z) || isinf(dir.x) || isinf(dir.y) || isinf(dir.z));
}

// ProjectPointOnRay, :381-410: the distance from the ray, and the projected point
ATN_DEV float npr_project(const f3& point, const f3& org, const f3& dir, f3& on_ray)
{
    const f3 x = point - org;
    on_ray = dot(x, dir) * dir;
    on_ray = on_ray + org;
    return length(point - on_ray);
}

// ComputeDistanceBetweenProjectedPositionOnRayAndRayOrigin, :419-427
ATN_DEV float npr_proj_dist(const f3& point, const f3& org, const f3& dir)
{
    f3 y;
    (void)npr_project(point, org, dir, y);
    return length(y - org);
}

// IsInLineWidth, :621-645
ATN_DEV bool npr_in_line_width(float w, const f3& org, const f3& dir, const f3& point, float acc, float pixel_width)
{
    f3 y;
    const float len = npr_project(point, org, dir, y);
    float dist = length(org - y);
    dist = acc + dist;
    const float w_scaled = dist * pixel_width * w;
    return len <= w_scaled;
}

// ComputeDepthThreshold, :573-609 (FLT_MAX when div == 0)
ATN_DEV float npr_depth_threshold(const f3& p, float scale, const f3& pq_pos, const f3& nq, const f3& ps_pos, const f3& ns, float dq, float ds)
{
    const f3 p_q = pq_pos - p, p_s = ps_pos - p;
    const f3 n_closest = length(p_q) > length(p_s) ? ns : nq;
    const float max_depth = smax(dq, ds);
    const float div = fabsf(dot(p_q, n_closest));
    if (div == 0.0F) return 3.402823466e+38F;
    return scale * max_depth * length(p_s - p_q) / div;
}

// ---- kernels (npr.hip) --------------------------------------------------------------------------------------------------------
#ifdef ATN_NPR_TU

// GenerateSampleRayAndDiscPerQueryRay (npr_impl.h:30-51), right after GeneratePath: disc 0 and the 8 nextSample2D draws.  The
// descriptors' previous hit point and normal are left as they are (the reference keeps SampleRayInfo across samples and frames).
__global__ void __launch_bounds__(256) k_npr_gen(PathBuffers pb, FrameParams fp, NprArgs na)
{
    const uint32_t count = pb.q_count[0];
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < count; j += gridDim.x * blockDim.x) {
        const uint32_t slot = pb.queue[0][j];
        const float4 ro = pb.ray_o[slot], rd = pb.ray_d[slot], t4 = pb.thr[slot];
        int32_t px = 0, py = 0;
        slot_to_pixel(fp, slot, px, py);
        const uint32_t idx = (uint32_t)(py * fp.width + px);
        const uint32_t rnd = pb.seeds[idx % fp.n_seeds];
        const uint32_t fs = fp.frame + (uint32_t)fp.sample;
        Cmj smp; smp.idx = fs % 256u; smp.dim = __float_as_uint(t4.w); smp.scramble = rnd * 0x1fe3434fu * ((fs + 133u * rnd) / 256u);
        NprDisc d = npr_first_disc(mk3(ro), mk3(rd), na.line_width, na.pixel_width);
#pragma unroll 1
        for (int k = 0; k < kNprRays; k++) {
            float u, v;
            cmj_next2d(smp, u, v);
            float4 dp = na.desc_p[kNprRays * slot + k], dn = na.desc_n[kNprRays * slot + k];
            dp.w = u * 2 - 1;
            dn.w = v * 2 - 1;
            na.desc_p[kNprRays * slot + k] = dp;
            na.desc_n[kNprRays * slot + k] = dn;
        }
        d.acc = 1.0F;
        npr_store_disc(na, slot, d);
        na.live[slot] = 0xffu;
        pb.thr[slot] = make_float4(t4.x, t4.y, t4.z, __uint_as_float(smp.dim));
    }
}

// Per bounce, in front of the walk: the disc at the query hit (ShadeSampleRay, npr_impl.h:397-445) or at the dummy point of a
// query miss (CreateNextDiscByDummyQueryRayHitPoint, :304-329), then GetSampleRay (:101-124) for every live sample ray.  A path's
// rays go to consecutive entries of the ray list, paths in the order of the bounce's queue (one atomic per block).
__global__ void __launch_bounds__(256) k_npr_prep(PathBuffers pb, DevScene sc, NprArgs na, int32_t bounce)
{
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t base;
    const uint32_t count = pb.q_count[bounce];
    const uint32_t* __restrict__ q = pb.queue[bounce & 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t j0 = blockIdx.x * 256u; j0 < count; j0 += gridDim.x * 256u) {
        const uint32_t j = j0 + threadIdx.x;
        uint32_t slot = 0, live = 0, listed = 0;
        f3 ro[kNprRays], rdir[kNprRays];
        if (j < count) {
            slot = q[j];
            live = na.live[slot] & 0xffu;
            const float4 is4 = pb.isect[slot];
            const int32_t objid = __float_as_int(is4.x);
            const f3 qo = mk3(pb.ray_o[slot]), qd = mk3(pb.ray_d[slot]);
            const NprDisc prev = npr_load_disc(na, slot);
            NprDisc disc = prev;
            bool eval = true;
            float hpd = 0.0F;
            if (objid >= 0) {
                const int32_t tri = __float_as_int(is4.w);
                const int32_t mtrlid = triangle_mtrlid(sc, tri);
                if (!(na.mflags[mtrlid >= 0 ? mtrlid : sc.n_materials] & 1u)) eval = false;     // :401-404, the disc is not advanced
                else {
                    HitRec rec;
                    evaluate_hit(rec, sc, objid, tri, is4.y, is4.z);
                    hpd = length(rec.p - prev.center);
                    disc = npr_disc_at(rec.p, qd, prev.radius, hpd, prev.acc);
                }
            }
            else if (bounce > 0) {
                const f3 dummy = qo + 100.0F * qd;
                hpd = length(dummy - prev.center);
                disc = npr_disc_at(dummy, qd, prev.radius, hpd, prev.acc);
            }
            if (eval) {
#pragma unroll
                for (int k = 0; k < kNprRays; k++) {
                    ro[k] = mk3(0.0F); rdir[k] = mk3(0.0F);
                    if (!((live >> k) & 1u)) continue;
                    const float4 dp = na.desc_p[kNprRays * slot + k], dn = na.desc_n[kNprRays * slot + k];
                    if (bounce == 0) {
                        // GenerateSampleRay (feature_line.h:195-219) towards disc 0 from the query ray's origin; the ray is built
                        // twice (generation, ExtractRayFromSampleRayDesc): its direction is normalised twice
                        const f3 pos = npr_disc_pos(dp.w, dn.w, prev);
                        ro[k] = qo; rdir[k] = normalize(normalize(pos - qo));
                    }
                    else if (!npr_next_ray(dp.w, dn.w, mk3(dp), mk3(dn), prev, disc, ro[k], rdir[k])) {
                        live &= ~(1u << k);
                        continue;
                    }
                    listed |= 1u << k;
                }
                if (objid >= 0 || bounce > 0) npr_store_disc(na, slot, disc);
                na.hpd[slot] = hpd;
                live |= kNprEval;
            }
        }
        // block-wide exclusive scan of the ray counts, one atomic per block
        const uint32_t n_rays = (uint32_t)__popc(listed);
        uint32_t incl = n_rays;
        for (uint32_t o = 1; o < 64u; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63u) wave_sum[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t tot = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
            base = tot ? atomicAdd(&na.counters[kNprCounters * bounce], tot) : 0u;
        }
        __syncthreads();
        uint32_t off = base + incl - n_rays;
        for (uint32_t w = 0; w < wave; w++) off += wave_sum[w];
        __syncthreads();        // (wave_sum / base belong to the next iteration)
        if (j < count) {
            na.work[slot] = off | (n_rays << 28);
#pragma unroll
            for (int k = 0; k < kNprRays; k++) {
                if ((listed >> k) & 1u) {
                    const uint32_t e = off + (uint32_t)__popc(listed & ((1u << k) - 1u));
                    na.ray_o[e] = make_float4(ro[k].x, ro[k].y, ro[k].z, 0.0F);
                    na.ray_d[e] = make_float4(rdir[k].x, rdir[k].y, rdir[k].z, __uint_as_float((uint32_t)k));
                }
            }
            na.live[slot] = live;
        }
    }
}

// The sample rays through the renderer's own walk: ClosestJob over the ray list, the count read on the device
struct NprRayJob {
    NprArgs na;
    float t_min;
    ATN_DEV void fetch(uint32_t j, float4& a, float4& b, float& stop_t) const
    {
        const float4 o = na.ray_o[j], d = na.ray_d[j];
        stop_t = -kInf;
        a = make_float4(o.x, o.y, o.z, kInf);
        b = make_float4(d.x, d.y, d.z, __uint_as_float(j));
    }
    ATN_DEV bool finish(uint32_t j, const Hit& h, bool, float4&, float4&, float&) const
    {
        na.ray_hit[j] = make_float4(__int_as_float(h.objid), h.a, h.b, __int_as_float(h.tri));
        return false;
    }
    ATN_DEV void cost(uint32_t, uint32_t, uint32_t) const {}
};

template <bool REFILL, bool LDSN>
__global__ void ATN_TRACE_ATTR __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_npr_trace(DevScene sc, NprArgs na, int32_t bounce)
{
    const uint32_t count = na.counters[kNprCounters * bounce];
    const NprRayJob job{ na, kEps };
    TravCounters tc{};
    trace_dispatch<false, REFILL, NprRayJob, LDSN>(sc, count, &na.counters[kNprCounters * bounce + 1], job, &tc);
}

// hitrecord.meshid: the triangle's mesh id (the top layer's is -1 for every instance the scene builder makes)
ATN_DEV int32_t npr_mesh_id(const DevScene& sc, int32_t tri)
{
    const int32_t m = sc.tris[tri].mesh_id;
    return m < 0 ? -1 : m;
}
ATN_DEV const DevMaterial& npr_material(const DevScene& sc, int32_t mtrlid) { return sc.materials[mtrlid >= 0 ? mtrlid : sc.n_materials]; }

// One path per lane: the four hit / miss cases (npr_impl.h:126-380), the closest feature-line point and the contribution
// (ComputeFeatureLineContribution, :62-80).  A path with a line is terminated and left out of the queue k_shade reads.
__global__ void __launch_bounds__(256) k_npr_eval(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, NprArgs na, int32_t bounce)
{
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t base;
    const uint32_t count = pb.q_count[bounce];
    const uint32_t* __restrict__ q = pb.queue[bounce & 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t j0 = blockIdx.x * 256u; j0 < count; j0 += gridDim.x * 256u) {
        const uint32_t j = j0 + threadIdx.x;
        bool keep = false;
        uint32_t slot = 0;
        if (j < count) {
            slot = q[j];
            keep = true;
            uint32_t live = na.live[slot];
            if (live & kNprEval) {
                const float4 is4 = pb.isect[slot];
                const int32_t objid = __float_as_int(is4.x);
                const float4 ro4 = pb.ray_o[slot], rd4 = pb.ray_d[slot];
                const f3 qo = mk3(ro4), qd = mk3(rd4);
                NprDisc disc = npr_load_disc(na, slot);
                const float acc1 = disc.acc - 1;        // "-1 is for initial camera distance" (npr_impl.h:170)
                const uint32_t wk = na.work[slot];
                const uint32_t first = wk & 0x0fffffffu, n_rays = wk >> 28;
                float closest = 3.402823466e+38F;
                bool found = false;
                HitRec hq;
                hq.p = mk3(0.0F); hq.normal = mk3(0.0F); hq.u = 0.0F; hq.v = 0.0F; hq.area = 0.0F;
                int32_t q_mesh = -1, q_mtrl = -1;
                float dist_q = 0.0F;
                bool glossy = true;
                if (objid >= 0) {
                    const int32_t tri = __float_as_int(is4.w);
                    evaluate_hit(hq, sc, objid, tri, is4.y, is4.z);
                    q_mtrl = triangle_mtrlid(sc, tri);
                    q_mesh = npr_mesh_id(sc, tri);
                    dist_q = length(hq.p - qo);
                    glossy = (npr_material(sc, q_mtrl).attrib & ATN_MTRL_ATTR_GLOSSY) != 0u;
                }
#pragma unroll 1
                for (uint32_t i = 0; i < n_rays; i++) {
                    const float4 so = na.ray_o[first + i], sd = na.ray_d[first + i], sh = na.ray_hit[first + i];
                    const uint32_t k = __float_as_uint(sd.w);
                    const int32_t s_obj = __float_as_int(sh.x);
                    bool term = false;
                    if (s_obj >= 0) {
                        const int32_t s_tri = __float_as_int(sh.w);
                        const int32_t s_mtrl = triangle_mtrlid(sc, s_tri);
                        if (!(na.mflags[s_mtrl >= 0 ? s_mtrl : sc.n_materials] & 1u)) term = true;
                        else {
                            HitRec hs;
                            evaluate_hit(hs, sc, s_obj, s_tri, sh.y, sh.z);
                            const float d_s = npr_proj_dist(hs.p, qo, qd);
                            if (objid >= 0) {
                                // EvaluateQueryAndSampleRayHit, :126-212
                                const int32_t s_mesh = npr_mesh_id(sc, s_tri);
                                term = s_mesh != q_mesh;
                                float4 dp = na.desc_p[kNprRays * slot + k], dn = na.desc_n[kNprRays * slot + k];
                                dp.x = hs.p.x; dp.y = hs.p.y; dp.z = hs.p.z;
                                dn.x = hs.normal.x; dn.y = hs.normal.y; dn.z = hs.normal.z;
                                na.desc_p[kNprRays * slot + k] = dp;
                                na.desc_n[kNprRays * slot + k] = dn;
                                if (npr_in_line_width(na.line_width, qo, qd, hs.p, acc1, na.pixel_width)) {
                                    const DevMaterial& mq = npr_material(sc, q_mtrl);
                                    const DevMaterial& ms = npr_material(sc, s_mtrl);
                                    const float4 aq = sample_texture(sc, mq.albedoMap, hq.u, hq.v, mq.baseColor);
                                    const float4 as = sample_texture(sc, ms.albedoMap, hs.u, hs.v, ms.baseColor);
                                    const f3 co = mk3(cam.origin[0], cam.origin[1], cam.origin[2]);
                                    const float depth_q = length(hq.p - co), depth_s = length(hs.p - co);
                                    // EvaluateMetrics (feature_line.h:445-481) with the QUERY material's flags
                                    const uint32_t mf = na.mflags[q_mtrl >= 0 ? q_mtrl : sc.n_materials] >> 8;
                                    const bool is_mesh = (mf & kNprMetricMesh) ? q_mesh != s_mesh : false;
                                    const bool is_albedo = (mf & kNprMetricAlbedo)
                                        ? fabsf(luminance(aq.x, aq.y, aq.z) - luminance(as.x, as.y, as.z)) > na.albedo_threshold : false;
                                    const bool is_normal = (mf & kNprMetricNormal) ? (1.0F - dot(hq.normal, hs.normal)) > na.normal_threshold : false;
                                    const bool is_depth = (mf & kNprMetricDepth)
                                        ? fabsf(depth_q - depth_s) > npr_depth_threshold(qo, 2.0F, hq.p, hq.normal, hs.p, hs.normal, depth_q, depth_s) : false;
                                    if (is_mesh || is_albedo || is_normal || is_depth) {
                                        if (d_s < closest && d_s < dist_q) { found = true; closest = d_s; }
                                        else if (dist_q < closest) { found = true; closest = dist_q; }
                                    }
                                }
                            }
                            else {
                                // EvaluateQueryRayNotHitButSampleRayHit, :331-380 (the sample's hit is evaluated with the QUERY ray:
                                // a triangle's hit record does not read the ray)
                                if (d_s < closest && npr_in_line_width(na.line_width, qo, qd, hs.p, acc1, na.pixel_width)) { found = true; closest = d_s; }
                            }
                        }
                    }
                    else {
                        if (objid >= 0) {
                            // EvaluateQueryRayHitButSampleRayNotHit, :214-282
                            const float pd = -dot(hq.normal, hq.p);
                            f3 pos = mk3(0.0F);
                            if (npr_ray_plane(hq.normal, pd, mk3(so), mk3(sd), pos)) {
                                const float d_s = npr_proj_dist(pos, qo, qd);
                                if (npr_in_line_width(na.line_width, qo, qd, pos, acc1, na.pixel_width)) {
                                    if (d_s < closest && d_s < dist_q) { found = true; closest = d_s; }
                                    else if (dist_q < closest) { found = true; closest = dist_q; }
                                }
                            }
                        }
                        term = true;
                    }
                    if (objid >= 0 && !glossy) term = true;      // :498-505
                    if (term) live &= ~(1u << k);
                }
                if (objid >= 0) { disc.acc += na.hpd[slot]; npr_store_disc(na, slot, disc); }
                if (found) {
                    if (na.st_line) {
                        int32_t px = 0, py = 0;
                        slot_to_pixel(fp, slot, px, py);
                        na.st_line[py * fp.width + px] = make_float4(1.0F, (float)bounce, closest, 0.0F);
                    }
                    // the line SETS the contribution (CopyVec) and terminates the path
                    const float pdf_line = (1.0F / (float)kNprRays) * (closest * closest);
                    const float pdfb = ro4.w;
                    const float weight = pdfb / (pdfb + pdf_line);     // _detail::ComputeBalanceHeuristic
                    const f3 c = (mk3(pb.thr[slot]) * weight) * mk3(na.line_color[0], na.line_color[1], na.line_color[2]);
                    pb.contrib[slot] = make_float4(c.x, c.y, c.z, 0.0F);
                    pb.ray_d[slot] = make_float4(rd4.x, rd4.y, rd4.z, __uint_as_float(__float_as_uint(rd4.w) | F_TERMINATED));
                    keep = false;
                }
            }
            na.live[slot] = live & 0xffu;
        }
        // the queue k_shade reads: the paths without a line, one atomic per block
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t tot = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
            base = tot ? atomicAdd(&na.counters[kNprCounters * bounce + 2], tot) : 0u;
        }
        __syncthreads();
        uint32_t off = base;
        for (uint32_t w = 0; w < wave; w++) off += wave_tot[w];
        if (keep) na.queue[off + bits_below_lane(m)] = slot;
        __syncthreads();
    }
}

// the survivors' count becomes the bounce's count for k_shade
__global__ void __launch_bounds__(64) k_npr_commit(PathBuffers pb, NprArgs na, int32_t bounce)
{
    if (threadIdx.x == 0) pb.q_count[bounce] = na.counters[kNprCounters * bounce + 2];
}

// the stage buffers after bounce 0 (atn_npr_capture): the disc, the sample-ray descriptors, the CMJ dimension
__global__ void __launch_bounds__(256) k_npr_capture0(PathBuffers pb, FrameParams fp, NprArgs na)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= (uint32_t)fp.n_slots) return;
    int32_t x, y;
    if (!slot_to_pixel(fp, slot, x, y)) return;
    const uint32_t idx = (uint32_t)(y * fp.width + x);
    na.st_dims[idx] = __float_as_uint(pb.thr[slot].w);
    na.st_disc[2 * idx] = na.disc_c[slot];
    na.st_disc[2 * idx + 1] = na.disc_n[slot];
    const uint32_t live = na.live[slot];
    for (int k = 0; k < kNprRays; k++)
        na.st_desc[kNprRays * idx + k] = make_float4(na.desc_p[kNprRays * slot + k].w, na.desc_n[kNprRays * slot + k].w, (float)((live >> k) & 1u), 0.0F);
}

#endif  // ATN_NPR_TU

} // namespace atn
