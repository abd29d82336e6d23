// Path tracing through homogeneous media (aten::VolumePathTracing::radiance / Nee, src/libaten/renderer/volume/volume_pathtracing.cpp:
// 22-89,228-407; UpdateMedium, SampleMedium, TraverseRayInMedium, TraverseShadowRay, volume_pathtracing_impl.h:24-294;
// HomogeniousMedium, volume/medium.h:26-122; HenyeyGreensteinPhaseFunction, volume/phase_function.h).  docs/VOLUME.md has the decisions.
//
// Per sample:  k_gen_path -> k_vol_begin -> 8 iterations i (MedisumStackSize, the cap of radiance's loop):
//   k_vol_closest (the renderer's walk; the hit and its distance) -> k_vol_shade (miss shade, roulette, free flight, the event or
//   the surface, UpdateMedium, all draws; at most one connection record per path) -> k_vol_transmit (the connection's walk through
//   medium boundaries; adds the contribution when the light is reached)
//
// State, SoA, indexed by path slot; only what a later kernel reads:
//   stack   uint4:  the medium stack, eight 16-bit material ids, the newest in the low half of x (push / pop shift the 128 bits)
//   meta    uint32: stack size (bits 0-3), depth_count (4-11), the shadow ray of aten::ShadowRay is active (12), the id at the
//                   BOTTOM of the stack (16-31): aten::stack::top() is queue_.front(), the first medium entered
//   hit_t   float:  Intersection::t of the iteration's closest hit
//   ev_o / ev_d float4: the last scatter event's point and direction (aten::ShadowRay::rayorg / raydir)
//   c_*     the connection record: see ConnRecord below                                              112 B per path
#pragma once
#include "kernels.hpp"
#include "volume_grid_track.h"

namespace atn {

constexpr int kVolIterations = 8;           // MedisumStackSize, pt_params.h:22
constexpr uint32_t kVolWalkMax = 64u;       // boundaries a connection may cross before it counts as blocked
constexpr uint32_t kVolMediumFlag = 1u, kVolPureFlag = 2u;      // VolMedium::flags: is_medium, type == MaterialType::Volume
// a medium that names a grid (atn_volume_set_grids): its index in flags >> kVolGridShift, and VolMedium::sigma_t holds its MAJORANT.
// Only the GRID flavours of the kernels (volume_grid.hip) meet one: a frame launches them when a material names a valid grid.
constexpr uint32_t kVolGridFlag = 4u, kVolGridShift = 8u;
// counters (uint32): [0, 9) live paths entering iteration i; [16, 24) connections of iteration i; [32, 41) fetch cursors of the
// closest-hit walks; [48, 56) of the connection walks; 64 stack overflows, 65 walk overflows, 66 connections, 67 segments (frame);
// 68 grid flights, 69 grid connections stopped at kVolGridStepsMax (frame; device/volume_grid.hpp)
constexpr int kVolCntQueue = 0, kVolCntConn = 16, kVolCntFetchC = 32, kVolCntFetchT = 48, kVolCntFrame = 64, kVolCounters = 80;
// stage flags (atn_volume_download, which = 0)
constexpr uint32_t kVolProcessed = 1u, kVolHit = 2u, kVolSampled = 4u, kVolAbsorbed = 8u, kVolScattered = 16u, kVolPassed = 32u,
                   kVolConn = 64u, kVolVisible = 128u, kVolTerminated = 256u;
// connection kinds (c_d.w bits 0-1) and the crossed-boundary count (bits 8-15)
constexpr uint32_t kVolConnSurface = 0u, kVolConnEvent = 1u, kVolConnNoAdd = 2u;

struct VolMedium { float g, sigma_a, sigma_s; uint32_t flags; float le[3]; float sigma_t; };
static_assert(sizeof(VolMedium) == 32, "VolMedium");

struct VolArgs {
    const VolMedium* med;       // one per material (+ the white-diffuse fallback: no medium)
    uint4* stack; uint32_t* meta; float* hit_t;
    float4* ev_o; float4* ev_d;
    // ConnRecord: c_o {org (offset along the normal), t_max}  c_d {dir, kind | crossed << 8}  c_w {transmittance, pixel, stack meta, segments}
    //   c_a {throughput, phase_f}  c_b {radiance | light colour, G}  c_c {albedo | pdf, select_prob, -}  c_stack: the stack BEFORE UpdateMedium
    float4* c_o; float4* c_d; float4* c_w; float4* c_a; float4* c_b; float4* c_c; uint4* c_stack;
    uint32_t* conn_q;
    uint2* segs;                // per slot: segments walked, connections made this frame (k_vol_reduce sums them)
    uint32_t* counters;
    float eps_bias;             // scene_rendering_config.epsilon_bias_for_traversing_shadow_ray_in_medium
    int32_t capture;            // the iteration of sample 0 whose state is kept (-1: none)
    uint4* st_state; uint4* st_stack; float4* st_ray; float4* st_conn;      // per pixel
};

// what the GRID flavours read besides VolArgs (a kernel argument of their own: the gridless kernels' arguments stay as they are)
struct VolGridArgs {
    const atn_vg::Grid* grids;  // atn_volume_set_grids, the densities on the device
    uint4* c_smp;               // per slot, the connection's own sample stream {idx, dim, scramble, ratio-tracking steps so far}
};

#ifdef ATN_VOLUME_TU      // (the kernels: volume.hip, volume_grid.hip; aten_amd.hip reads the declarations above)
// ---- the medium stack --------------------------------------------------------------------------------------------------------
struct VolStack { uint4 q; uint32_t n, bottom; };
ATN_DEV VolStack vol_stack_load(const uint4& q, uint32_t meta) { VolStack s; s.q = q; s.n = meta & 15u; s.bottom = meta >> 16; return s; }
ATN_DEV uint32_t vol_stack_meta(const VolStack& s) { return s.n | (s.bottom << 16); }
// false: the stack is full, the push is dropped (aten::stack only asserts, misc/stack.h:51-62)
ATN_DEV bool vol_push(VolStack& s, uint32_t id)
{
    if (s.n >= (uint32_t)kVolIterations) return false;
    s.q.w = (s.q.w << 16) | (s.q.z >> 16);
    s.q.z = (s.q.z << 16) | (s.q.y >> 16);
    s.q.y = (s.q.y << 16) | (s.q.x >> 16);
    s.q.x = (s.q.x << 16) | (id & 0xffffu);
    if (s.n == 0u) s.bottom = id & 0xffffu;
    s.n++;
    return true;
}
ATN_DEV void vol_pop(VolStack& s)
{
    s.q.x = (s.q.x >> 16) | (s.q.y << 16);
    s.q.y = (s.q.y >> 16) | (s.q.z << 16);
    s.q.z = (s.q.z >> 16) | (s.q.w << 16);
    s.q.w = s.q.w >> 16;
    s.n--;
}
// UpdateMedium, volume_pathtracing_impl.h:24-48.  false: a push was dropped
ATN_DEV bool vol_update_medium(const f3& ray_dir, const f3& wo, const f3& nml, uint32_t mflags, uint32_t id, VolStack& s)
{
    const f3 wi = -ray_dir;
    const bool is_transmitted = (dot(wo, nml) < 0) != (dot(wi, nml) < 0);
    const bool is_enter = dot(wi, nml) > 0;
    if (is_transmitted) {
        if (is_enter) { if (mflags & kVolMediumFlag) return vol_push(s, id); }
        else if (s.n > 0u) vol_pop(s);
    }
    return true;
}

// ---- HenyeyGreensteinPhaseFunction, volume/phase_function.h --------------------------------------------------------------------
ATN_DEV float hg_evaluate(float g, const f3& wi, const f3& wo)
{
    g = sclamp(g, -1.0F, 1.0F);
    const float g2 = sqr(g);
    const float costheta = dot(wi, wo);
    const float _4pi = 4 * kPi;
    return (1 - g2) / (_4pi * powf((1 + g2) - (2 * g) * costheta, 1.5F));
}
ATN_DEV f3 hg_sample(float r1, float r2, float g, const f3& w)
{
    g = sclamp(g, -1.0F, 1.0F);
    float costheta = 0.0F;
    if (fabsf(g) < kEps) costheta = 1 - 2 * r1;
    else {
        const float g2 = sqr(g);
        costheta = (1 / (2 * g)) * ((1 + g2) - sqr((1 - g2) / ((1 - g) + (2 * g) * r1)));
    }
    const float sintheta = sqrtf(1 - costheta * costheta);
    const float phi = kPi2 * r2;
    const float cosphi = cosf(phi);
    const float sinphi = sinf(phi);
    f3 t, b;
    tangent_coordinate(w, t, b);
    const f3 dir = ((t * sintheta) * cosphi + (b * sintheta) * sinphi) + w * costheta;
    return normalize(dir);
}

// ---- the closest-hit walk of an iteration: ClosestJob that keeps Intersection::t as well ------------------------------------------
struct VolClosestJob {
    PathBuffers pb;
    const uint32_t* __restrict__ q;
    float* hit_t;
    float t_min;
    ATN_DEV void fetch(uint32_t j, float4& a, float4& b, float& stop_t) const
    {
        const uint32_t slot = q[j];
        const float4 ro = pb.ray_o[slot], rd = pb.ray_d[slot];
        stop_t = -kInf;
        a = make_float4(ro.x, ro.y, ro.z, kInf);
        b = make_float4(rd.x, rd.y, rd.z, __uint_as_float(slot));
    }
    ATN_DEV bool finish(uint32_t slot, const Hit& h, bool, float4&, float4&, float&) const
    {
        pb.isect[slot] = make_float4(__int_as_float(h.objid), h.a, h.b, __int_as_float(h.tri));
        hit_t[slot] = h.t;
        return false;
    }
    ATN_DEV void cost(uint32_t, uint32_t, uint32_t) const {}
};

template <bool REFILL, bool LDSN>
__global__ void ATN_TRACE_ATTR __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_vol_closest(PathBuffers pb, DevScene sc, VolArgs va, int32_t it)
{
    const uint32_t count = va.counters[kVolCntQueue + it];
    const VolClosestJob job{ pb, pb.queue[it & 1], va.hit_t, kEps };
    TravCounters tc{};
    trace_dispatch<false, REFILL, VolClosestJob, LDSN>(sc, count, &va.counters[kVolCntFetchC + it], job, &tc);
}

// ---- the connection's walk: TraverseRayInMedium, volume_pathtracing_impl.h:111-229 ----------------------------------------------
// One connection per lane; a closest-hit walk per segment (Job::finish hands the lane the next segment's ray).  The running state
// (origin, remaining distance, transmittance, the stack's copy, boundaries crossed) lives in the connection record between segments.
// the connection's sample stream as the tracking loops draw from it (device/volume_grid_track.h)
struct VolDraw {
    Cmj& smp;
    ATN_DEV float next() { return cmj_next(smp); }
};
// the extra state of the GRID flavour: nothing for the gridless walk, so that VolWalkJobT<false> is laid out as VolWalkJob always was
template <bool GRID> struct VolWalkGrid {};
template <> struct VolWalkGrid<true> { VolGridArgs vg; };

// GRID: a segment inside a grid medium is ratio-tracked with the connection's own stream (docs/VOLUME.md, "Grid media")
template <bool GRID>
struct VolWalkJobT : VolWalkGrid<GRID> {
    PathBuffers pb;
    DevScene sc;
    VolArgs va;
    float t_min;
    // the transmittance of the segment org .. org + distance * dir in medium `md`.  false: the tracking loop hit its cap
    ATN_DEV bool segment(uint32_t slot, const VolMedium& md, const f3& org, const f3& dir, float distance, float& transmittance) const
    {
        if constexpr (GRID) {
            if (md.flags & kVolGridFlag) {
                const atn_vg::Grid g = this->vg.grids[md.flags >> kVolGridShift];
                const uint4 cs = this->vg.c_smp[slot];
                Cmj smp{ cs.x, cs.y, cs.z };
                VolDraw draw{ smp };
                atn_vg::NoTie tie;
                uint32_t steps = cs.w;
                bool capped = false;
                const float tr = atn_vg::ratio_track(g, md.sigma_a, md.sigma_s, md.sigma_t, org.x, org.y, org.z, dir.x, dir.y, dir.z, distance, draw, tie, steps, capped);
                this->vg.c_smp[slot] = make_uint4(cs.x, smp.dim, cs.z, steps);
                transmittance = transmittance * tr;
                if (capped) atomicAdd(&va.counters[kVolCntFrame + 5], 1u);
                return !capped;
            }
        }
        transmittance = transmittance * expf(-md.sigma_t * distance);
        return true;
    }
    ATN_DEV void fetch(uint32_t j, float4& a, float4& b, float& stop_t) const
    {
        const uint32_t slot = va.conn_q[j];
        const float4 o = va.c_o[slot], d = va.c_d[slot];
        stop_t = -kInf;
        a = o;
        b = make_float4(d.x, d.y, d.z, __uint_as_float(slot));
    }
    ATN_DEV void cost(uint32_t, uint32_t, uint32_t) const {}
    ATN_DEV void end(uint32_t slot, bool visible, float transmittance, uint32_t kind, uint32_t pixel, uint32_t segments) const
    {
        if (visible && !(kind & kVolConnNoAdd)) {
            const float4 A = va.c_a[slot], B = va.c_b[slot], C = va.c_c[slot];
            f3 add;
            if (kind & kVolConnEvent) {
                // Ls = transmittance * phase_f * G * light_color / pdf / select_prob; contrib += throughput * Ls
                const f3 Ls = ((((transmittance * A.w) * B.w) * mk3(B)) / C.x) / C.y;
                add = mk3(A) * Ls;
            }
            else add = ((mk3(A) * transmittance) * mk3(B)) * mk3(C);     // throughput * transmittance * radiance * albedo
            const float4 c = pb.contrib[slot];
            pb.contrib[slot] = make_float4(c.x + add.x, c.y + add.y, c.z + add.z, 0.0F);
        }
        uint2 sg = va.segs[slot];
        sg.x += segments; sg.y += 1u;
        va.segs[slot] = sg;
        if (va.st_conn && (pixel >> 31)) {
            float4* o = va.st_conn + 3u * (size_t)(pixel & 0x7fffffffu);
            o[2] = make_float4((float)segments, visible ? 1.0F : 0.0F, 0.0F, 0.0F);
            o[1].w = transmittance;
            if constexpr (GRID) {       // the ratio-tracking steps and the final dimension of the connection's stream
                const uint4 cs = this->vg.c_smp[slot];
                o[2].z = (float)cs.w; o[2].w = (float)cs.y;
            }
        }
    }
    ATN_DEV bool finish(uint32_t slot, const Hit& h, bool is_hit, float4& ra, float4& rb, float& rstop) const
    {
        const float4 o4 = va.c_o[slot], d4 = va.c_d[slot], w4 = va.c_w[slot];
        const f3 org = mk3(o4), dir = mk3(d4);
        float t_max = o4.w;
        const uint32_t bits = __float_as_uint(d4.w);
        const uint32_t crossed = (bits >> 8) & 255u;
        float transmittance = w4.x;
        const uint32_t pixel = __float_as_uint(w4.y);
        const uint32_t segments = __float_as_uint(w4.w) + 1u;
        VolStack st = vol_stack_load(va.c_stack[slot], __float_as_uint(w4.z));
        if (is_hit) {
            HitRec rec;
            evaluate_hit(rec, sc, h.objid, h.tri, h.a, h.b);
            const int32_t mid = triangle_mtrlid(sc, h.tri);
            const uint32_t mslot = (uint32_t)(mid >= 0 ? mid : sc.n_materials);
            const uint32_t mflags = va.med[mslot].flags;
            const bool is_enter = dot(-dir, rec.normal) > 0;
            // a surface, or a surface with an interior entered from outside, blocks the light; a pure medium boundary is stepped
            // through in both directions (docs/VOLUME.md: the one place that does not follow volume_pathtracing_impl.h:152-160 as written)
            if (!(mflags & kVolMediumFlag) || (is_enter && !(mflags & kVolPureFlag))) { end(slot, false, transmittance, bits, pixel, segments); return false; }
            if (crossed >= kVolWalkMax) {
                atomicAdd(&va.counters[kVolCntFrame + 1], 1u);
                end(slot, false, transmittance, bits, pixel, segments);
                return false;
            }
            if (st.n > 0u) {
                const float distance = length(org - rec.p);
                if (!segment(slot, va.med[st.bottom], org, dir, distance, transmittance)) { end(slot, false, transmittance, bits, pixel, segments); return false; }
            }
            if (!vol_update_medium(dir, dir, rec.normal, mflags, (uint32_t)sc.materials[mslot].id, st)) atomicAdd(&va.counters[kVolCntFrame + 0], 1u);
            const f3 nml = dot(dir, rec.normal) > 0 ? rec.normal : -rec.normal;
            const f3 no = ray_offset(rec.p, nml);
            const f3 nd = normalize(dir);
            t_max = t_max - h.t;
            va.c_o[slot] = make_float4(no.x, no.y, no.z, t_max);
            va.c_d[slot] = make_float4(nd.x, nd.y, nd.z, __uint_as_float((bits & 0xffu) | ((crossed + 1u) << 8)));
            va.c_w[slot] = make_float4(transmittance, w4.y, __uint_as_float(vol_stack_meta(st)), __uint_as_float(segments));
            va.c_stack[slot] = st.q;
            ra = make_float4(no.x, no.y, no.z, t_max);
            rb = make_float4(nd.x, nd.y, nd.z, __uint_as_float(slot));
            rstop = -kInf;
            return true;
        }
        if (st.n > 0u) {
            const f3 end_p = org + t_max * dir;
            const float distance = length(org - end_p);
            if (!segment(slot, va.med[st.bottom], org, dir, distance, transmittance)) { end(slot, false, transmittance, bits, pixel, segments); return false; }
        }
        end(slot, true, transmittance, bits, pixel, segments);
        return false;
    }
};
using VolWalkJob = VolWalkJobT<false>;

#ifndef ATN_VOLUME_GRID_TU      // (volume_grid.hip instantiates the GRID flavours only: the gridless kernels live in volume.hip)
template <bool REFILL, bool LDSN>
__global__ void ATN_TRACE_ATTR __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_vol_transmit(PathBuffers pb, DevScene sc, VolArgs va, int32_t it)
{
    const uint32_t count = va.counters[kVolCntConn + it];
    const VolWalkJob job{ {}, pb, sc, va, kEps };
    TravCounters tc{};
    trace_dispatch<false, REFILL, VolWalkJob, LDSN>(sc, count, &va.counters[kVolCntFetchT + it], job, &tc);
}

// a fresh path: empty stack, depth_count 0, no shadow ray (PathThroughput::medium is cleared with the path)
__global__ void __launch_bounds__(256) k_vol_begin(FrameParams fp, VolArgs va)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= (uint32_t)fp.n_slots) return;
    va.stack[slot] = make_uint4(0u, 0u, 0u, 0u);
    va.meta[slot] = 0u;
    if (fp.sample == 0) va.segs[slot] = make_uint2(0u, 0u);
}

// per-slot segment / connection counts -> the frame's counters (one atomic per block and counter)
__global__ void __launch_bounds__(256) k_vol_reduce(FrameParams fp, VolArgs va)
{
    __shared__ uint32_t tot[2][4];
    uint32_t a = 0, b = 0;
    for (uint32_t slot = blockIdx.x * 256u + threadIdx.x; slot < (uint32_t)fp.n_slots; slot += gridDim.x * 256u) {
        const uint2 s = va.segs[slot];
        a += s.x; b += s.y;
    }
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off); b += __shfl_down(b, off); }
    if ((threadIdx.x & 63u) == 0u) { tot[0][threadIdx.x >> 6] = a; tot[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t sa = tot[0][0] + tot[0][1] + tot[0][2] + tot[0][3], sb = tot[1][0] + tot[1][1] + tot[1][2] + tot[1][3];
        if (sa) atomicAdd(&va.counters[kVolCntFrame + 3], sa);
        if (sb) atomicAdd(&va.counters[kVolCntFrame + 2], sb);
    }
}

#endif  // !ATN_VOLUME_GRID_TU

// SampleLight (pathtracing_impl.h:178-208) + the connection record of a scatter event (TraverseShadowRay, volume_pathtracing_impl.h:
// 231-283): the ray direction stands in for a normal.  Returns whether a record was written.
ATN_DEV bool vol_event_connection(const DevScene& sc, const VolArgs& va, uint32_t slot, uint32_t pixel_bits, Cmj& smp, const f3& org, const f3& evd,
                                  const f3& throughput, const VolStack& st)
{
    if (sc.n_lights <= 0) return false;
    int32_t li = (int32_t)(cmj_next(smp) * (float)sc.n_lights);
    li = li < sc.n_lights - 1 ? li : sc.n_lights - 1;
    LightSample ls;
    ls.attrib = sc.lights[li].attrib;
    sample_light(ls, sc.lights[li], sc, org, evd, smp);
    const f3 nml = dot(ls.dir, evd) > 0 ? evd : -evd;
    const f3 o = ray_offset(org, nml);
    const f3 d = normalize(ls.dir);
    float dist = ls.dist;
    if (ls.attrib & ATN_LIGHT_ATTR_INFINITE) dist = length(ls.pos - org);
    const float t_max = dist - va.eps_bias;
    const float phase_f = hg_evaluate(va.med[st.bottom].g, -evd, ls.dir);
    const float G = 1.0F / sqr(ls.dist);
    va.c_o[slot] = make_float4(o.x, o.y, o.z, t_max);
    va.c_d[slot] = make_float4(d.x, d.y, d.z, __uint_as_float(kVolConnEvent));
    va.c_w[slot] = make_float4(1.0F, __uint_as_float(pixel_bits), __uint_as_float(vol_stack_meta(st)), __uint_as_float(0u));
    va.c_a[slot] = make_float4(throughput.x, throughput.y, throughput.z, phase_f);
    va.c_b[slot] = make_float4(ls.color.x, ls.color.y, ls.color.z, G);
    va.c_c[slot] = make_float4(ls.pdf, sc.inv_n_lights, 0.0F, 0.0F);
    va.c_stack[slot] = st.q;
    if (va.st_conn && (pixel_bits >> 31)) {
        float4* so = va.st_conn + 3u * (size_t)(pixel_bits & 0x7fffffffu);
        so[0] = make_float4(o.x, o.y, o.z, t_max);
        so[1] = make_float4(d.x, d.y, d.z, 1.0F);
    }
    return true;
}

// VolumePathTracing::Nee (volume_pathtracing.cpp:228-407) + ShadeMiss with bounce = depth_count + the bookkeeping of TraverseShadowRay
// (volume_pathtracing_impl.h:285-293), one path per lane over the iteration's queue.  The body is device/volume_shade_body.hpp, shared as
// text with k_vol_shade_grid (device/volume_grid.hpp)
#ifndef ATN_VOLUME_GRID_TU
template <int MS>
__global__ void __launch_bounds__(256) k_vol_shade(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, VolArgs va, int32_t it)
{
#define ATN_VOL_SHADE_GRID 0
#include "volume_shade_body.hpp"
#undef ATN_VOL_SHADE_GRID
}
#endif

#ifndef ATN_VOLUME_GRID_TU
// HenyeyGreensteinPhaseFunction::SampleDirection(r1, r2, g, w) and Evaluate(g, w, wo) for n cases (atn_volume_phase_table)
__global__ void __launch_bounds__(256) k_vol_phase_table(float g, uint32_t n, const float* __restrict__ w, const float* __restrict__ r1,
                                                         const float* __restrict__ r2, const float* __restrict__ wo, float* __restrict__ out_dir,
                                                         float* __restrict__ out_eval)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const f3 ww = mk3(w[3u * i], w[3u * i + 1u], w[3u * i + 2u]);
    const f3 d = hg_sample(r1[i], r2[i], g, ww);
    out_dir[3u * i] = d.x; out_dir[3u * i + 1u] = d.y; out_dir[3u * i + 2u] = d.z;
    out_eval[i] = hg_evaluate(g, ww, mk3(wo[3u * i], wo[3u * i + 1u], wo[3u * i + 2u]));
}
#endif  // !ATN_VOLUME_GRID_TU
#endif  // ATN_VOLUME_TU

} // namespace atn
