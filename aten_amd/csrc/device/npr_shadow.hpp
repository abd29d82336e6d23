// The NPR shadow pre-pass (aten::NprPathTracer::OnRender's first pass, src/libaten/renderer/npr/npr.cpp:284-349,399-447;
// idaten::NPRPathTracing::onShadeByShadowRay, src/libidaten/npr/npr_pathtracing.cu:211-281,446-476,521-605): the screen-space shadow
// texture Toon / StylizedBrdf materials read (toon.hpp, toon_bsdf), made from the frame's own bounce-0 shadow rays.
// docs/NPR_SHADOW.md has the decisions.
//
// Per frame, in front of the frame's sample loop:  k_gen_path (sample 0) -> k_ns_primary (the closest-hit walk of the primary rays; its
//   job also keeps t) -> k_ns_shade (PathTracing::shade at bounce 0 up to and including FillShadowRay, the termination flag forced off;
//   the active rays to a compact list) -> k_ns_trace (the renderer's walk over the list, ShadowJob's fetch and finish rules, the answer
//   a bit) -> k_ns_filter (ApplyBilateralFilter<ShadowRay, float, true, 5>, aorenderer_impl.h:138-191: 11 taps along the row)
//
// State.  The shadow ray, its list and their counters are the bank's own (sh_o / sh_d / shadow_q / sh_count[0] / fetch_shadow[0]): the
// frame's sample 0 writes them again behind the pre-pass.  What the pre-pass adds:
//   depth_s   float:  the primary hit's t (a miss: unused)                           4 B per path slot
//   lit / depth / plane   float per pixel: the ray reached its light (1.0 / 0.0), the primary t, the filtered plane    12 B per pixel
#pragma once
#include "kernels.hpp"

namespace atn {

constexpr int32_t kNsRadius = 5;        // ApplyBilateralFilter<..., 5>: 11 taps

struct NsArgs {
    float* depth_s;
    float* lit; float* depth; float* plane;
};

// ---- kernels (npr_shadow.hip) -------------------------------------------------------------------------------------------------
#ifdef ATN_NPR_SHADOW_TU

// ApplyBilateralFilter<ShadowRay, float, true, 5> with coefficients (2, 2) for pixel (cx, cy): the depth term is divided by the centre
// depth (coeff_depth is never used); a centre that missed (depth inf) makes every weight NaN and the result 1
ATN_DEV float ns_bilateral(const float* __restrict__ lit, const float* __restrict__ depth, int32_t cx, int32_t cy, int32_t width)
{
    const float coeff_pixel_dist_2 = 2 * (2.0F * 2.0F);
    const float* __restrict__ lrow = lit + (size_t)cy * (size_t)width;
    const float* __restrict__ drow = depth + (size_t)cy * (size_t)width;
    const float center_depth = drow[cx];
    float numer = 0.0F, denom = 0.0F;
#pragma unroll
    for (int32_t i = -kNsRadius; i <= kNsRadius; i++) {
        const int32_t x = min(max(cx + i, 0), width - 1);
        const float diff = center_depth - drow[x];
        const float kernel = expf((float)(-(i * i)) / coeff_pixel_dist_2 - (diff * diff) / center_depth);
        numer += lrow[x] * kernel;
        denom += kernel;
    }
    const float r = denom > 0.0F ? numer / denom : 1.0F;
    return sclamp(r, 0.0F, 1.0F);
}

// The primary rays through the renderer's walk: ClosestJob, which keeps the hit's t as well (the filter's depth)
struct NsPrimaryJob {
    PathBuffers pb;
    float* depth_s;
    float t_min;
    ATN_DEV void fetch(uint32_t j, float4& a, float4& b, float& stop_t) const
    {
        const uint32_t slot = pb.queue[0][j];
        const float4 ro = pb.ray_o[slot], rd = pb.ray_d[slot];
        stop_t = -kInf;
        a = make_float4(ro.x, ro.y, ro.z, kInf);
        b = make_float4(rd.x, rd.y, rd.z, __uint_as_float(slot));
    }
    ATN_DEV bool finish(uint32_t slot, const Hit& h, bool, float4&, float4&, float&) const
    {
        pb.isect[slot] = make_float4(__int_as_float(h.objid), h.a, h.b, __int_as_float(h.tri));
        depth_s[slot] = h.t;
        return false;
    }
    ATN_DEV void cost(uint32_t, uint32_t, uint32_t) const {}
};

template <bool LDSN>
__global__ void ATN_TRACE_ATTR __launch_bounds__(256) k_ns_primary(PathBuffers pb, DevScene sc, NsArgs na)
{
    const uint32_t count = pb.q_count[0];
    const NsPrimaryJob job{ pb, na.depth_s, kEps };
    TravCounters tc{};
    trace_dispatch<false, false, NsPrimaryJob, LDSN>(sc, count, nullptr, job, &tc);
}

// PathTracing::shade (pathtracing.cpp:91-236) at bounce 0 for one primary hit, up to and including FillShadowRay
// (pathtracing_impl.h:178-264), with the sampler dimensions of the frame's own sample 0 in their order.  Returns whether the shadow ray
// is active; then it is in the slot's shadow record (sh_o / sh_d).  Nothing of the path's state is written.
ATN_DEV bool ns_cast(const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, uint32_t slot, const float4& is4)
{
    const f3 ray_dir = mk3(pb.ray_d[slot]);
    uint4 s4;
    s4.y = __float_as_uint(pb.thr[slot].w);
    path_sampler(s4, pb, fp, slot, fp.frame + (uint32_t)fp.sample);
    Cmj smp; smp.idx = s4.x; smp.dim = s4.y; smp.scramble = s4.z;
    HitRec rec;
    int32_t mtrlid;
    bool isBackfacing;
    vertex_surface(rec, mtrlid, isBackfacing, sc, is4, ray_dir);
    const int32_t mtrl_slot = mtrlid >= 0 ? mtrlid : sc.n_materials;
    // (a copy whose type and attributes the toon rule below rewrites: its members live in registers, nothing goes to the stack)
    DevMaterial m = sc.materials[mtrl_slot];
    if (m.type == ATN_MTRL_TOON || m.type == ATN_MTRL_STYLIZED_BRDF) {
        // HitTeminatedMaterial's draws come first: Toon::bsdf samples its target light (toon.cpp:88-161); its colour and its inline
        // visibility walk consume nothing
        const atn_toon_param& tp = sc.toon[mtrl_slot];
        if (tp.target_light_idx >= 0 && tp.target_light_idx < sc.n_npr_lights) smp.dim += light_sample_draws(sc.npr_lights[tp.target_light_idx], sc);
        // pathtracing.cpp:174-184: shading goes on with the base material, or returns in front of FillShadowRay
        if (!sc.enable_shadowray_base_stylized_shadow) return false;
        const int32_t tt = tp.toon_type;
        m.type = tt == ATN_MTRL_DIFFUSE ? ATN_MTRL_DIFFUSE : ATN_MTRL_SPECULAR;
        m.attrib = (m.attrib & ~(uint32_t)ATN_MTRL_ATTR_SINGULAR) | (tt == ATN_MTRL_TOON_SPECULAR ? ATN_MTRL_ATTR_SINGULAR : 0u);
    }
    // HitImplicitLight (pathtracing_impl.h:395-451): the light's own surface returns early
    if (m.type == ATN_MTRL_EMISSIVE && (m.attrib & ATN_MTRL_ATTR_EMISSIVE) && !isBackfacing) return false;
    f3 orienting_normal = rec.normal;
    HitPre hp;
    const float pre_r = vertex_frame<kMsToon>(sc, m, mtrl_slot, rec, isBackfacing, ray_dir, smp, orienting_normal, hp);
    const bool invalid_mtrl = (m.attrib & (ATN_MTRL_ATTR_SINGULAR | ATN_MTRL_ATTR_TRANSLUCENT)) != 0;
    if (sc.n_lights <= 0 || invalid_mtrl) return false;
    int32_t li = 0;
    if (sc.n_lights > 1) {
        li = (int32_t)(cmj_next(smp) * (float)sc.n_lights);
        li = li < sc.n_lights - 1 ? li : sc.n_lights - 1;
    }
    else smp.dim++;
    // (next to the light index: HitShadowRay's surface_mtrl.stencil_type == ALWAYS, pathtracing.cpp:59-66)
    const float lbits = __uint_as_float((uint32_t)li | ((m.attrib & kAttrStencilAlways) ? kShadowStencilFlag : 0u));
    // ComputeRadianceNEE decides whether the ray is active; its value is not needed (throughput and albedo of one)
    return nee_evaluate<kMsToon>(sc, m, mtrl_slot, rec, orienting_normal, hp, pre_r, ray_dir, smp, li, mk3(1.0F), mk3(1.0F),
                                 [&](const f3&, const LightSample& ls) { store_shadow_ray(pb, slot, rec, orienting_normal, ls, lbits); });
}

// One primary ray per lane: the pixel's planes are written afresh (lit = 0; depth = the primary t, inf for a miss), the hits are
// shaded up to the shadow ray, and the slots whose ray is active go to the shadow list in the order of the queue (block scan, one
// atomic per block).
__global__ void __launch_bounds__(256) k_ns_shade(PathBuffers pb, DevScene sc, FrameParams fp, NsArgs na)
{
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t base;
    const uint32_t count = pb.q_count[0];
    const uint32_t* __restrict__ q = pb.queue[0];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t j0 = blockIdx.x * 256u; j0 < count; j0 += gridDim.x * 256u) {
        const uint32_t j = j0 + threadIdx.x;
        uint32_t slot = 0;
        bool active = false;
        if (j < count) {
            slot = q[j];
            const float4 is4 = pb.isect[slot];
            int32_t px = 0, py = 0;
            slot_to_pixel(fp, slot, px, py);
            const uint32_t idx = (uint32_t)(py * fp.width + px);
            const bool hit = __float_as_int(is4.x) >= 0;
            // a miss is IEEE +inf, not the walk's AT_MATH_INF (the largest finite float): centred on it every weight is NaN and the
            // filter falls back to 1; with the finite value the centre tap would weigh 1 and the result be 0 (docs/NPR_SHADOW.md)
            na.depth[idx] = hit ? na.depth_s[slot] : __int_as_float(0x7f800000);
            na.lit[idx] = 0.0F;
            if (hit) active = ns_cast(pb, sc, fp, slot, is4);
        }
        const unsigned long long mask = __ballot(active);
        if (lane == 0u) wave_sum[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t tot = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
            base = tot ? atomicAdd(&pb.sh_count[0], tot) : 0u;
        }
        __syncthreads();
        uint32_t off = base + bits_below_lane(mask);
        for (uint32_t w = 0; w < wave; w++) off += wave_sum[w];
        __syncthreads();        // (wave_sum / base belong to the next iteration)
        if (active) pb.shadow_q[off] = slot;
    }
}

// The shadow rays through the renderer's walk, answered as HitTestToTargetLight / scene::hitLight answer them
// (pathtracing_impl.h:266-393, scene/scene.h:64-134): ShadowJob's fetch (its early-stop rules are the frame's own) and ShadowJob's
// finish with one difference -- a ray that reached its light sets the pixel's bit and adds nothing.  The light bits are read next to the
// direction (sh_d.w): sh_c is not written by the pre-pass.
struct NsShadowJob {
    ShadowJob<true> s;
    FrameParams fp;
    float* lit;
    float t_min;
    ATN_DEV void fetch(uint32_t j, float4& a, float4& b, float& stop_t) const { s.fetch(j, a, b, stop_t); }
    ATN_DEV void cost(uint32_t, uint32_t, uint32_t) const {}
    ATN_DEV bool finish(uint32_t payload, const Hit& h, bool isHit, float4& ra, float4& rb, float& rstop) const
    {
        const PathBuffers& pb = s.pb;
        const DevScene& sc = s.sc;
        const uint32_t slot = payload & kShadowSlotMask;
        const uint32_t lookups = (payload >> 27) & 15u;
        const float4 sd = pb.sh_d[slot];
        const uint32_t lbits = __float_as_uint(sd.w);
        const atn_light_param* lp = &sc.lights[lbits & kShadowLightMask];
        const int32_t ltype = lp->type, lobj = lp->arealight_objid;
        const uint32_t lattr = lp->attrib;
        const int32_t lightobj = (ltype == ATN_LIGHT_AREA && lobj >= 0) ? lobj : -1;
        const bool same_obj = isHit ? h.objid == lightobj : (lookups == 0u || (payload & (1u << 26)) != 0u);
        bool visible;
        if (same_obj) visible = true;
        else if (lattr & ATN_LIGHT_ATTR_INFINITE) visible = !isHit;
        else if (lattr & ATN_LIGHT_ATTR_SINGULAR) visible = h.t > pb.sh_o[slot].w;     // distToLight
        else visible = false;
        if (sc.any_alpha && isHit) {
            const bool need_stencil = (lbits & kShadowStencilFlag) != 0u;
            const uint32_t max_lookups = (sc.enable_alpha_blending || need_stencil) ? 10u : 1u;
            if (visible || max_lookups > 1u) {
                const int32_t mid = triangle_mtrlid(sc, h.tri);
                const uint32_t mattr = mid >= 0 ? sc.materials[mid].attrib : 0u;
                bool ignore = need_stencil && (mattr & kAttrStencilStencil);
                f3 hit_p = mk3(0.0F), hit_n = mk3(0.0F, 1.0F, 0.0F);
                if (ignore || (mattr & kAttrMaybeAlpha)) {
                    HitRec rec;
                    evaluate_hit(rec, sc, h.objid, h.tri, h.a, h.b);
                    hit_p = rec.p; hit_n = rec.normal;
                    if (mattr & kAttrMaybeAlpha) {
                        const DevMaterial& hm = sc.materials[mid];
                        const float4 albedo = sample_texture(sc, hm.albedoMap, rec.u, rec.v, make_float4(1.0F, 1.0F, 1.0F, 1.0F));
                        if (albedo.w * hm.baseColor.w < 1.0F) ignore = true;
                    }
                }
                if (ignore) {
                    if (lookups + 1u >= max_lookups) return false;      // budget spent: the bit stays clear
                    const float distToLight = pb.sh_o[slot].w;
                    const f3 odir = normalize(mk3(sd));
                    const bool is_same_facing = dot(hit_n, odir) > 0.0F;
                    const f3 on = is_same_facing ? hit_n : -hit_n;
                    const f3 o = ray_offset(hit_p, on);
                    const f3 d = normalize(odir);
                    ra = make_float4(o.x, o.y, o.z, distToLight - kEps);
                    rb = make_float4(d.x, d.y, d.z, __uint_as_float(slot | ((lookups + 1u) << 27) | (h.objid == lightobj ? (1u << 26) : 0u)));
                    rstop = -kInf;
                    return true;
                }
            }
        }
        if (visible) {
            int32_t px = 0, py = 0;
            slot_to_pixel(fp, slot, px, py);
            lit[(uint32_t)(py * fp.width + px)] = 1.0F;
        }
        return false;
    }
};

template <bool REFILL, bool LDSN>
__global__ void ATN_TRACE_ATTR __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_ns_trace(PathBuffers pb, DevScene sc, FrameParams fp, NsArgs na)
{
    const uint32_t count = pb.sh_count[0];
    const NsShadowJob job{ ShadowJob<true>{ pb, sc, kEps }, fp, na.lit, kEps };
    TravCounters tc{};
    trace_dispatch<false, REFILL, NsShadowJob, LDSN>(sc, count, &pb.fetch_shadow[0], job, &tc);
}

// One pixel per lane, a block of 256 along a row (coalesced; the 11 taps of a lane's neighbours hit the same lines)
__global__ void __launch_bounds__(256) k_ns_filter(const float* __restrict__ lit, const float* __restrict__ depth, float* __restrict__ out,
                                                    int32_t width, int32_t height)
{
    const int32_t x = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    const int32_t y = (int32_t)blockIdx.y;
    if (x >= width || y >= height) return;
    out[(size_t)y * (size_t)width + (size_t)x] = ns_bilateral(lit, depth, x, y, width);
}

#endif  // ATN_NPR_SHADOW_TU

} // namespace atn
