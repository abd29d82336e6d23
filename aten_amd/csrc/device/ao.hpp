// Ambient occlusion (aten::AORenderer::RenderAO / RenderAOWithBilateralFilter, src/libaten/renderer/ao/aorenderer.cpp:20-275, the
// per-pixel code of aorenderer_impl.h:33-191; the miss rule of idaten's kernels, src/libidaten/ao/ao.cu:14-78, behind
// break_on_terminate = 0).  docs/AO.md has the decisions.
//
// Per frame:  k_gen_path -> k_ao_primary (the closest-hit walk of the primary rays; its job also keeps t) -> k_ao_shade (sampler,
//   hit record, normal map, the num_rays cosine-weighted directions; the rays of a pixel to consecutive entries of the ray list; a
//   miss records its x in the row's minimum) -> k_ao_trace (the renderer's walk over the list, t_max = radius, the alpha skip-through
//   as a restart of the lane) -> k_ao_resolve (the fold in ray order, the planes, the film) [-> k_ao_bilateral]
//
// State, SoA; R = num_rays; only what a later kernel reads:
//   ray_o / ray_d / ray_n / ray_res   float4: the ray's origin.xyz, - / the direction it walks (re-normalised by every restart).xyz, -
//                                     / Diffuse::sampleDirection's direction.xyz, Diffuse::pdf / the answer {0 miss | 1 hit | 2 ten
//                                     skip-throughs, t, c, skip-throughs}                                    64 B per listed ray
//   work        uint32: the pixel's first ray in the list                                                 4 B per path slot
//   depth_s     float:  the primary hit's t (inf: a miss)                                                 4 B per path slot
//   row_min     uint32: per image row, the least x whose primary ray missed (0xffffffff: none)
//   state / value / depth   per pixel: 0 not rendered | 1 hit | 2 miss, the AO value handed to the film, the primary t    12 B per pixel
#pragma once
#include "kernels.hpp"

namespace atn {

constexpr int kAoMaxRays = 64;
constexpr uint32_t kAoMaxLoop = 10u;                // MAX_LOOP, aorenderer_impl.h:66
constexpr uint32_t kAoRayMask = (1u << 28) - 1u;    // payload: ray index (bits 0-27), skip-throughs so far (bits 28-31)
constexpr uint32_t kAoNotRendered = 0u, kAoHit = 1u, kAoMiss = 2u;
constexpr int kAoCounters = 2;                      // 0 rays listed, 1 the walk's fetch cursor

struct AoArgs {
    float4* ray_o; float4* ray_d; float4* ray_n; float4* ray_res;
    uint32_t* work; float* depth_s;
    uint32_t* row_min;
    uint32_t* counters;
    uint32_t* state; float* value; float* depth;
    int32_t num_rays;
    float radius;
    int32_t literal;            // break_on_terminate: the CPU renderer's row rule / idaten's miss rule
    int32_t filter;
    // stage buffers (atn_ao_capture; null = off), per pixel
    float4* st_ray;             // [2 n]: the first AO ray as k_ao_shade made it {org.xyz, 0} {dir.xyz, 0}
    float4* st_ans;             // its answer {0 | 1 | 2, t, c, skip-throughs}
};

// ---- kernels (ao.hip) ---------------------------------------------------------------------------------------------------------
#ifdef ATN_AO_TU

// The primary rays through the renderer's walk: ClosestJob, which keeps the hit's t as well (Intersection::t is the filter's depth)
struct AoPrimaryJob {
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
__global__ void ATN_TRACE_ATTR __launch_bounds__(256) k_ao_primary(PathBuffers pb, DevScene sc, AoArgs aa)
{
    const uint32_t count = pb.q_count[0];
    const AoPrimaryJob job{ pb, aa.depth_s, kEps };
    TravCounters tc{};
    trace_dispatch<false, false, AoPrimaryJob, LDSN>(sc, count, nullptr, job, &tc);
}

// AORenderer::radiance's sampler and ShandeByAO up to the ray loop (aorenderer.cpp:27-29, aorenderer_impl.h:41-70), one primary ray
// per lane.  Nothing after the direction draws consumes samples, so all num_rays rays are made here.  A pixel's rays go to
// consecutive entries of the ray list, pixels in the order of the queue (one atomic per block).
__global__ void __launch_bounds__(256) k_ao_shade(PathBuffers pb, DevScene sc, FrameParams fp, AoArgs aa)
{
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t base;
    const uint32_t count = pb.q_count[0];
    const uint32_t* __restrict__ q = pb.queue[0];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t R = (uint32_t)aa.num_rays;
    for (uint32_t j0 = blockIdx.x * 256u; j0 < count; j0 += gridDim.x * 256u) {
        const uint32_t j = j0 + threadIdx.x;
        uint32_t slot = 0, idx = 0, n_rays = 0;
        float4 is4 = make_float4(0.0F, 0.0F, 0.0F, 0.0F);
        if (j < count) {
            slot = q[j];
            is4 = pb.isect[slot];
            int32_t px = 0, py = 0;
            slot_to_pixel(fp, slot, px, py);
            idx = (uint32_t)(py * fp.width + px);
            if (__float_as_int(is4.x) >= 0) { n_rays = R; aa.state[idx] = kAoHit; }
            else {
                aa.state[idx] = kAoMiss;
                // (the minimum only falls: a value read here that is already <= x settles it without the atomic)
                if ((uint32_t)px < aa.row_min[py]) atomicMin(&aa.row_min[py], (uint32_t)px);
            }
        }
        // block-wide exclusive scan of the ray counts, one atomic per block
        uint32_t incl = n_rays;
        for (uint32_t o = 1; o < 64u; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63u) wave_sum[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t tot = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
            base = tot ? atomicAdd(&aa.counters[0], tot) : 0u;
        }
        __syncthreads();
        uint32_t off = base + incl - n_rays;
        for (uint32_t w = 0; w < wave; w++) off += wave_sum[w];
        __syncthreads();        // (wave_sum / base belong to the next iteration)
        if (j < count) aa.work[slot] = off;
        if (n_rays) {
            const uint32_t rnd = pb.seeds[idx % fp.n_seeds];
            Cmj smp; smp.idx = fp.frame % 256u; smp.dim = 4u + 5u * 300u; smp.scramble = rnd * 0x1fe3434fu * ((fp.frame + 331u * rnd) / 256u);
            const int32_t tri = __float_as_int(is4.w);
            HitRec rec;
            evaluate_hit(rec, sc, __float_as_int(is4.x), tri, is4.y, is4.z);
            // FillMaterial: a negative id selects the white-diffuse fallback the upload appends; applyNormal without CarPaint (refused)
            const int32_t mtrlid = triangle_mtrlid(sc, tri);
            const f3 n = apply_normal_map(sc, sc.materials[mtrlid >= 0 ? mtrlid : sc.n_materials].normalMap, rec.normal, rec.u, rec.v);
            const f3 org = ray_offset(rec.p, n);        // ray(rec.p, nextDir, orienting_normal), ray.h:17-24
#pragma unroll 1
            for (uint32_t i = 0; i < R; i++) {
                const float r1 = cmj_next(smp);
                const float r2 = cmj_next(smp);
                const f3 next_dir = diffuse_dir(n, r1, r2);
                const f3 dir = normalize(next_dir);     // the ray constructor normalises again
                const uint32_t e = off + i;
                aa.ray_o[e] = make_float4(org.x, org.y, org.z, 0.0F);
                aa.ray_d[e] = make_float4(dir.x, dir.y, dir.z, 0.0F);
                aa.ray_n[e] = make_float4(next_dir.x, next_dir.y, next_dir.z, diffuse_pdf(n, next_dir));
                if (i == 0u && aa.st_ray) {
                    aa.st_ray[2u * idx] = make_float4(org.x, org.y, org.z, 0.0F);
                    aa.st_ray[2u * idx + 1u] = make_float4(dir.x, dir.y, dir.z, 0.0F);
                }
            }
        }
    }
}

// The AO rays through the renderer's walk (aorenderer_impl.h:71-112): the walk's t_max = radius caps box tests only, so a triangle
// beyond the radius can be the answer.  A hit on a translucent-by-alpha material restarts the lane behind it along the same direction,
// up to kAoMaxLoop walks in all, the way ShadowJob::finish restarts.
struct AoRayJob {
    AoArgs aa;
    DevScene sc;
    float t_min;
    ATN_DEV void fetch(uint32_t j, float4& a, float4& b, float& stop_t) const
    {
        const float4 o = aa.ray_o[j], d = aa.ray_d[j];
        stop_t = -kInf;
        a = make_float4(o.x, o.y, o.z, aa.radius);
        b = make_float4(d.x, d.y, d.z, __uint_as_float(j));
    }
    ATN_DEV bool finish(uint32_t payload, const Hit& h, bool isHit, float4& ra, float4& rb, float& rstop) const
    {
        const uint32_t j = payload & kAoRayMask, skips = payload >> 28;
        if (!isHit) {
            aa.ray_res[j] = make_float4(0.0F, 0.0F, 0.0F, (float)skips);
            return false;
        }
        HitRec rec;
        evaluate_hit(rec, sc, h.objid, h.tri, h.a, h.b);
        const int32_t mid = triangle_mtrlid(sc, h.tri);
        bool translucent = false;
        if (mid >= 0 && (sc.materials[mid].attrib & kAttrMaybeAlpha)) {
            // material::isTranslucentByAlpha (material.cpp:193-210); only flagged materials can have alpha < 1
            const DevMaterial& hm = sc.materials[mid];
            const float4 albedo = sample_texture(sc, hm.albedoMap, rec.u, rec.v, make_float4(1.0F, 1.0F, 1.0F, 1.0F));
            translucent = albedo.w * hm.baseColor.w < 1.0F;
        }
        if (translucent) {
            if (skips + 1u >= kAoMaxLoop) {     // the tenth walk ended on a pane too: nothing is added
                aa.ray_res[j] = make_float4(2.0F, h.t, 0.0F, (float)(skips + 1u));
                return false;
            }
            // ao_ray = ray(ao_rec.p, ao_ray.dir, the normal turned along the ray), :89-97
            const f3 cur = mk3(aa.ray_d[j]);
            const bool is_same_facing = dot(rec.normal, cur) > 0.0F;
            const f3 on = is_same_facing ? rec.normal : -rec.normal;
            const f3 o = ray_offset(rec.p, on);
            const f3 d = normalize(cur);
            aa.ray_d[j] = make_float4(d.x, d.y, d.z, 0.0F);
            ra = make_float4(o.x, o.y, o.z, aa.radius);
            rb = make_float4(d.x, d.y, d.z, __uint_as_float(j | ((skips + 1u) << 28)));
            rstop = -kInf;
            return true;
        }
        const float c = dot(rec.normal, mk3(aa.ray_n[j]));
        aa.ray_res[j] = make_float4(1.0F, h.t, c, (float)skips);
        return false;
    }
    ATN_DEV void cost(uint32_t, uint32_t, uint32_t) const {}
};

template <bool REFILL, bool LDSN>
__global__ void ATN_TRACE_ATTR __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_ao_trace(DevScene sc, AoArgs aa)
{
    const uint32_t count = aa.counters[0];
    const AoRayJob job{ aa, sc, kEps };
    TravCounters tc{};
    trace_dispatch<false, REFILL, AoRayJob, LDSN>(sc, count, &aa.counters[1], job, &tc);
}

// Film::put / FilmProgressive::put (renderer/film.cpp:33-45,61-71) of (c, c, c, 1): col = (0 + c) / cnt with cnt = 1
ATN_DEV float4 ao_film_put(const FrameParams& fp, float4* film, uint32_t idx, float c)
{
    const float a = (0.0F + c) / 1.0F;
    float4 out = make_float4(a, a, a, 1.0F);
    if (fp.progressive) {
        const float4 cur = film[idx];
        const float n = (float)((int32_t)cur.w);
        const float d = n + 1;
        out = make_float4((n * cur.x + a) / d, (n * cur.y + a) / d, (n * cur.z + a) / d, n + 1);
    }
    film[idx] = out;
    return out;
}

// One pixel per lane: the fold of the pixel's rays IN INDEX ORDER (a miss sets the value to one and so discards what earlier rays
// added, aorenderer_impl.h:99-111), / num_rays, the planes, and the film where the mode's rule writes it (aorenderer.cpp:128-141):
// literal -- the pixels left of the row's first primary miss; otherwise every pixel, a primary miss being 1.0 (ao.cu:14-34).
__global__ void __launch_bounds__(256) k_ao_resolve(FrameParams fp, AoArgs aa, float4* film, float4* tile_out)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= (uint32_t)fp.n_slots) return;
    int32_t x, y;
    float4 out = make_float4(0, 0, 0, 0);
    if (slot_to_pixel(fp, slot, x, y)) {
        const uint32_t idx = (uint32_t)(y * fp.width + x);
        const uint32_t st = aa.state[idx];
        const uint32_t first_miss = aa.row_min[y];
        bool put = false;
        float v = 0.0F;
        if (aa.literal && (uint32_t)x > first_miss) aa.state[idx] = kAoNotRendered;     // `break` left the row's loop
        else {
            aa.depth[idx] = aa.depth_s[slot];
            if (st == kAoHit) {
                const uint32_t first = aa.work[slot];
                float ao = 0.0F;
#pragma unroll 1
                for (int32_t i = 0; i < aa.num_rays; i++) {
                    const float4 r = aa.ray_res[first + (uint32_t)i];
                    if (r.x == 0.0F) ao = 1.0F;
                    else if (r.x == 1.0F && r.z > 0.0F) ao += r.y / aa.radius * r.z / aa.ray_n[first + (uint32_t)i].w;
                }
                ao /= (float)aa.num_rays;
                v = ao; put = true;
                if (aa.st_ans) aa.st_ans[idx] = aa.ray_res[first];
            }
            else if (!aa.literal) { v = 1.0F; put = true; }
            if (put) aa.value[idx] = v;
        }
        if (put && !aa.filter) out = ao_film_put(fp, film, idx, v);
        else out = film[idx];
    }
    if (tile_out && !aa.filter) tile_out[slot] = out;
}

// RenderAOWithBilateralFilter's two passes (aorenderer.cpp:218-243) over the value and depth planes: ApplyBilateralFilter<., ., true>
// times <., ., false> (aorenderer_impl.h:138-191), 7 taps each, both on the unfiltered plane, then c < 1 ? c / 2 : c
template <bool HORIZONTAL>
ATN_DEV float ao_bilateral(const AoArgs& aa, int32_t cx, int32_t cy, int32_t width, int32_t height)
{
    const float coeff_pixel_dist_2 = 2 * (2.0F * 2.0F);
    const float center_depth = aa.depth[cy * width + cx];
    float numer = 0.0F, denom = 0.0F;
#pragma unroll
    for (int32_t i = -3; i <= 3; i++) {
        int32_t x = cx, y = cy;
        if (HORIZONTAL) x = min(max(cx + i, 0), width - 1);
        else y = min(max(cy + i, 0), height - 1);
        const int32_t idx = y * width + x;
        const float diff = center_depth - aa.depth[idx];
        const float kernel = expf((float)(-(i * i)) / coeff_pixel_dist_2 - (diff * diff) / center_depth);
        numer += aa.value[idx] * kernel;
        denom += kernel;
    }
    const float r = denom > 0.0F ? numer / denom : 1.0F;
    return sclamp(r, 0.0F, 1.0F);
}

__global__ void __launch_bounds__(256) k_ao_bilateral(FrameParams fp, AoArgs aa, float4* film, float4* tile_out)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= (uint32_t)fp.n_slots) return;
    int32_t x, y;
    float4 out = make_float4(0, 0, 0, 0);
    if (slot_to_pixel(fp, slot, x, y)) {
        float c = ao_bilateral<true>(aa, x, y, fp.width, fp.height);
        c *= ao_bilateral<false>(aa, x, y, fp.width, fp.height);
        c = c < 1.0F ? c * 0.5F : c;
        out = ao_film_put(fp, film, (uint32_t)(y * fp.width + x), c);
    }
    if (tile_out) tile_out[slot] = out;
}

#endif  // ATN_AO_TU

} // namespace atn
