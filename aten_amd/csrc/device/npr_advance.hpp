// NPR look-through (aten::NprPathTracer::AdvanceNPRPath, src/libaten/renderer/npr/npr.cpp:202-282, with CheckStencil and
// CheckMaterialTranslucentByAlpha, renderer/pathtracing/pathtracing_impl.h:511-678): behind a StencilType::STENCIL surface the path
// looks for a front-facing ALWAYS surface, behind a surface whose alpha is < 1 it goes on with the surface's colour blended in.
// docs/NPR_ADVANCE.md has the rules and the quirks kept.  Opt-in (atn_npr_set_skip_through(1)) and launched only for scenes that
// need it (a STENCIL material, or alpha blending with a material whose alpha may be < 1).
//
// Per bounce b, between k_npr_commit and the shade launch:
//   k_npr_advance (a job over the queue NPR's eval left, through the frame's walk: fetch evaluates the query hit and decides what the
//   path does -- nothing, the stencil lookups, the alpha lookups -- finish applies the rules to the walk's answer and restarts the
//   lane behind the surface, at most 10 walks per check) -> k_npr_adv_commit -> k_shade_ab (shade_body's alpha-blend flavour).
// The reference traces the path's ray once more after a check said true: that walk repeats the last one done inside the check, so the
// job takes the last walk's answer (the tests' CPU twin walks again and holds the shortcut to that, docs/NPR_ADVANCE.md).
//
// State, per path slot:
//   ab        float4: alpha_blend.throughput.xyz, alpha_blend.transmission            (0, 0, 0, 1) per sample (k_npr_adv_init)
//   ab_acc    uint32: is_accumulating_alpha_blending                                  1 per sample
//   ray_o / ray_d  float4: the ray the current check walks (CheckStencil's local ray; the path's ray inside the alpha check)
//   info      uint32: bits 0-1 which check said true (1 stencil, 2 alpha), bits 8-15 walks done           0 per sample
#pragma once
#include "npr.hpp"

namespace atn {

constexpr uint32_t kAdvMaxLookups = 10u;            // MAX_LOOKUPS of both checks
constexpr uint32_t kAdvSlotMask = (1u << 26) - 1u;  // payload: bits 0-25 slot, 26-29 walks done in the current check, 30-31 the check (0 = none)
constexpr uint32_t kAdvWalkShift = 26u, kAdvKindShift = 30u;
constexpr uint32_t kAdvNone = 0u, kAdvStencil = 1u, kAdvAlpha = 2u;
constexpr int kAdvCounters = 2;                     // per bounce: 0 the walk's fetch cursor, 1 paths left for the shade launch

struct NprAdvArgs {
    const uint32_t* queue_in;       // NprArgs::queue: the bounce's paths without those a line ended
    const uint32_t* counters_in;    // NprArgs::counters ([kNprCounters * bounce + 2]: how many)
    uint32_t* queue_out;            // ... without those whose look-through ended in a miss (they go to the next bounce's trace queue)
    uint32_t* counters;             // [kAdvCounters * bounce + i]
    float4* ab; uint32_t* ab_acc;
    float4* ray_o; float4* ray_d;
    uint32_t* info;
    float4* st_adv;                 // stage buffer (atn_npr_capture; null = off), [2 n] per pixel after bounce 0:
                                    //   {check that said true, walks done, the answer: triangle id or -1, is_singular} {throughput.xyz, transmission}
    int32_t max_depth;
};

#ifdef ATN_NPR_ADVANCE_TU

// FillMaterial: a negative id selects the white-diffuse fallback behind the last material
ATN_DEV const DevMaterial& adv_material(const DevScene& sc, int32_t mtrlid) { return sc.materials[mtrlid >= 0 ? mtrlid : sc.n_materials]; }

__global__ void __launch_bounds__(256) k_npr_adv_init(FrameParams fp, NprAdvArgs aa)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= (uint32_t)fp.n_slots) return;
    aa.ab[slot] = make_float4(0.0F, 0.0F, 0.0F, 1.0F);
    aa.ab_acc[slot] = 1u;
    aa.info[slot] = 0u;
}

struct NprAdvanceJob {
    PathBuffers pb;
    DevScene sc;
    NprAdvArgs aa;
    int32_t bounce;
    float t_min;

    // ray(hit_pos, dir, -hit_nml) (ray.h:17-24: the direction is normalised again) into the slot's working ray
    ATN_DEV void restart_behind(uint32_t slot, const f3& p, const f3& n, const f3& dir, f3& o, f3& d) const
    {
        o = ray_offset(p, -n);
        d = normalize(dir);
        aa.ray_o[slot] = make_float4(o.x, o.y, o.z, 0.0F);
        aa.ray_d[slot] = make_float4(d.x, d.y, d.z, 0.0F);
    }
    // one look-through of CheckMaterialTranslucentByAlpha's loop up to its walk (:560-568): the ray behind the pane, the pane's colour
    // into alpha_blend.throughput, its transparency into alpha_blend.transmission, is_singular
    ATN_DEV void through_pane(uint32_t slot, const f3& p, const f3& n, const f3& dir, const float4& base, const float4& texel, float alpha,
                              f3& o, f3& d) const
    {
        restart_behind(slot, p, n, dir, o, d);
        float4 bl = aa.ab[slot];
        // transmission * baseColor * texel * alpha, left to right
        bl.x = bl.x + ((bl.w * base.x) * texel.x) * alpha;
        bl.y = bl.y + ((bl.w * base.y) * texel.y) * alpha;
        bl.z = bl.z + ((bl.w * base.z) * texel.z) * alpha;
        bl.w = bl.w * (1.0F - alpha);
        aa.ab[slot] = bl;
        pb.ray_d[slot].w = __uint_as_float(__float_as_uint(pb.ray_d[slot].w) | F_SINGULAR);
    }
    // AdvanceNPRPath up to the first walk (npr.cpp:209-270) at the slot's query hit.  `after_stencil`: CheckStencil has said false.
    // Returns the check whose ray (o, d) is to be walked, or kAdvNone.
    ATN_DEV uint32_t begin(uint32_t slot, bool after_stencil, f3& o, f3& d) const
    {
        const float4 is4 = pb.isect[slot];
        const int32_t objid = __float_as_int(is4.x);
        if (objid < 0) return kAdvNone;
        const int32_t tri = __float_as_int(is4.w);
        const DevMaterial& m = adv_material(sc, triangle_mtrlid(sc, tri));
        const uint32_t attr = m.attrib;
        const bool stencil = !after_stencil && (attr & kAttrStencilStencil) != 0u;
        // (:524-537) the alpha check does nothing with blending off, once an original hit was opaque, or on a translucent material
        const bool blend = sc.enable_alpha_blending != 0 && !(attr & ATN_MTRL_ATTR_TRANSLUCENT) && aa.ab_acc[slot] != 0u;
        if (!stencil && !blend) return kAdvNone;
        if (!stencil && !(attr & kAttrMaybeAlpha)) {
            // baseColor.a >= 1 and no texel with a < 1 (the upload's flag): alpha >= 1 without looking at the hit (:604-607)
            aa.ab_acc[slot] = 0u;
            return kAdvNone;
        }
        const f3 dir = mk3(pb.ray_d[slot]);
        HitRec rec;
        evaluate_hit(rec, sc, objid, tri, is4.y, is4.z);
        const bool isBackfacing = dot(rec.normal, -dir) < 0.0F;
        // applyNormal FIRST, then the back-face flip (npr.cpp:229-242: the other way round than PathTracing::shade); CarPaint is refused
        f3 n = apply_normal_map(sc, m.normalMap, rec.normal, rec.u, rec.v);
        if (!(attr & ATN_MTRL_ATTR_TRANSLUCENT) && isBackfacing) n = -n;
        if (stencil) {
            restart_behind(slot, rec.p, n, dir, o, d);
            return kAdvStencil;
        }
        const float4 texel = sample_texture(sc, m.albedoMap, rec.u, rec.v, make_float4(1.0F, 1.0F, 1.0F, 1.0F));
        const float alpha = texel.w * m.baseColor.w;
        if (!(alpha < 1.0F)) { aa.ab_acc[slot] = 0u; return kAdvNone; }     // the only thing that stops the accumulation
        through_pane(slot, rec.p, n, dir, m.baseColor, texel, alpha, o, d);
        return kAdvAlpha;
    }

    ATN_DEV void fetch(uint32_t j, float4& a, float4& b, float& stop_t) const
    {
        const uint32_t slot = aa.queue_in[j];
        stop_t = -kInf;
        f3 o, d;
        const uint32_t kind = begin(slot, false, o, d);
        if (kind == kAdvNone) {
            // nothing to do: a ray no box lets in (t_max < t_min; finite slab constants); finish() hands the slot on
            a = make_float4(0.0F, 0.0F, 0.0F, -1.0F);
            b = make_float4(0.57735026F, 0.57735026F, 0.57735026F, __uint_as_float(slot));
            return;
        }
        aa.info[slot] = 0u;     // (the previous bounce's)
        a = make_float4(o.x, o.y, o.z, kInf);
        b = make_float4(d.x, d.y, d.z, __uint_as_float(slot | (kind << kAdvKindShift)));
    }

    // the path stays in the queue the shade launch reads
    ATN_DEV void keep(uint32_t slot) const { aa.queue_out[atomicAdd(&aa.counters[kAdvCounters * bounce + 1], 1u)] = slot; }

    // A check said true and its last walk's answer is the path's intersection (npr.cpp:272-281); `walks`: all walks done for the slot.
    ATN_DEV void answer(uint32_t slot, uint32_t kind, uint32_t walks, const Hit& h, bool isHit) const
    {
        const float4 wo = aa.ray_o[slot], wd = aa.ray_d[slot];
        const float4 ro = pb.ray_o[slot], rd = pb.ray_d[slot];
        uint32_t flags = __float_as_uint(rd.w);
        aa.info[slot] = kind | (walks << 8);
        pb.ray_o[slot] = make_float4(wo.x, wo.y, wo.z, ro.w);
        if (isHit) {
            pb.ray_d[slot] = make_float4(wd.x, wd.y, wd.z, __uint_as_float(flags));
            pb.isect[slot] = make_float4(__int_as_float(h.objid), h.a, h.b, __int_as_float(h.tri));
            keep(slot);
            return;
        }
        // a miss: not shaded at this depth and not terminated -- the path goes to depth + 1 with its new ray, misses again there and
        // takes ShadeMissSampleRay and ShadeMiss of that depth (nothing at depth + 1 == maxDepth)
        flags &= ~F_HIT;
        pb.ray_d[slot] = make_float4(wd.x, wd.y, wd.z, __uint_as_float(flags));
        pb.isect[slot] = make_float4(__int_as_float(-1), 0.0F, 0.0F, __int_as_float(-1));
        if (bounce + 1 < aa.max_depth) {
            uint32_t* qn = ((bounce + 1) & 1) ? pb.queue[1] : pb.queue[0];     // (no dynamic index into the kernel arguments)
            qn[atomicAdd(&pb.q_count[bounce + 1], 1u)] = slot;
        }
    }

    ATN_DEV bool finish(uint32_t payload, const Hit& h, bool isHit, float4& ra, float4& rb, float& rstop) const
    {
        const uint32_t slot = payload & kAdvSlotMask;
        uint32_t kind = payload >> kAdvKindShift;
        if (kind == kAdvNone) { keep(slot); return false; }
        uint32_t walks = ((payload >> kAdvWalkShift) & 15u) + 1u;      // (of this check, this walk included)
        rstop = -kInf;
        f3 o, d;
        if (kind == kAdvStencil) {
            // CheckStencil's loop body, :635-674.  A miss returns false (the reference walks the same ray ten times)
            bool verdict = false;
            if (isHit) {
                const uint32_t hattr = adv_material(sc, triangle_mtrlid(sc, h.tri)).attrib;
                if (hattr & (kAttrStencilAlways | kAttrStencilStencil)) {
                    const f3 dir = mk3(aa.ray_d[slot]);
                    HitRec rec;
                    evaluate_hit(rec, sc, h.objid, h.tri, h.a, h.b);
                    if (hattr & kAttrStencilAlways) verdict = !(dot(rec.normal, -dir) < 0.0F);      // "not apply stencil to back facing"
                    else if (walks < kAdvMaxLookups) {
                        restart_behind(slot, rec.p, rec.normal, dir, o, d);
                        ra = make_float4(o.x, o.y, o.z, kInf);
                        rb = make_float4(d.x, d.y, d.z, __uint_as_float(slot | (walks << kAdvWalkShift) | (kAdvStencil << kAdvKindShift)));
                        return true;
                    }
                }
            }
            if (verdict) { answer(slot, kAdvStencil, walks, h, true); return false; }
            // false: the alpha check runs on the original hit, with the path's ray as it was
            kind = begin(slot, true, o, d);
            if (kind == kAdvNone) { aa.info[slot] = walks << 8; keep(slot); return false; }
            aa.info[slot] = walks << 8;
            ra = make_float4(o.x, o.y, o.z, kInf);
            rb = make_float4(d.x, d.y, d.z, __uint_as_float(slot | (kAdvAlpha << kAdvKindShift)));
            return true;
        }
        // CheckMaterialTranslucentByAlpha's loop behind its walk, :576-600, and the next look-through
        const uint32_t before = aa.info[slot] >> 8;        // (CheckStencil's walks)
        if (isHit) {
            const DevMaterial& hm = adv_material(sc, triangle_mtrlid(sc, h.tri));
            if (hm.attrib & kAttrMaybeAlpha) {
                const f3 dir = mk3(aa.ray_d[slot]);
                HitRec rec;
                evaluate_hit(rec, sc, h.objid, h.tri, h.a, h.b);
                const float4 texel = sample_texture(sc, hm.albedoMap, rec.u, rec.v, make_float4(1.0F, 1.0F, 1.0F, 1.0F));
                const float alpha = texel.w * hm.baseColor.w;
                if (!(alpha >= 1.0F) && walks < kAdvMaxLookups) {
                    // the pane's normal turned against the ray
                    const f3 n = dot(-dir, rec.normal) < 0.0F ? -rec.normal : rec.normal;
                    through_pane(slot, rec.p, n, dir, hm.baseColor, texel, alpha, o, d);
                    ra = make_float4(o.x, o.y, o.z, kInf);
                    rb = make_float4(d.x, d.y, d.z, __uint_as_float(slot | (walks << kAdvWalkShift) | (kAdvAlpha << kAdvKindShift)));
                    return true;
                }
            }
        }
        // a miss, an opaque surface, or the tenth walk ended on a pane: that walk's answer
        answer(slot, kAdvAlpha, before + walks, h, isHit);
        return false;
    }
    ATN_DEV void cost(uint32_t, uint32_t, uint32_t) const {}
};

template <bool REFILL, bool LDSN>
__global__ void ATN_TRACE_ATTR __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_npr_advance(PathBuffers pb, DevScene sc, NprAdvArgs aa, int32_t bounce)
{
    const uint32_t count = aa.counters_in[kNprCounters * bounce + 2];
    const NprAdvanceJob job{ pb, sc, aa, bounce, kEps };
    TravCounters tc{};
    trace_dispatch<false, REFILL, NprAdvanceJob, LDSN>(sc, count, &aa.counters[kAdvCounters * bounce], job, &tc);
}

// what the look-through left in the queue becomes the bounce's count for the shade launch
__global__ void __launch_bounds__(64) k_npr_adv_commit(PathBuffers pb, NprAdvArgs aa, int32_t bounce)
{
    if (threadIdx.x == 0) pb.q_count[bounce] = aa.counters[kAdvCounters * bounce + 1];
}

// the stage buffer after bounce 0's look-through, in front of its shade launch (atn_npr_capture)
__global__ void __launch_bounds__(256) k_npr_adv_capture0(PathBuffers pb, FrameParams fp, NprAdvArgs aa)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= (uint32_t)fp.n_slots) return;
    int32_t x, y;
    if (!slot_to_pixel(fp, slot, x, y)) return;
    const uint32_t idx = (uint32_t)(y * fp.width + x);
    const uint32_t info = aa.info[slot];
    const float4 is4 = pb.isect[slot];
    const float ans = __float_as_int(is4.x) >= 0 ? (float)__float_as_int(is4.w) : -1.0F;
    const bool singular = (__float_as_uint(pb.ray_d[slot].w) & F_SINGULAR) != 0u;
    aa.st_adv[2 * idx] = make_float4((float)(info & 3u), (float)(info >> 8), ans, singular ? 1.0F : 0.0F);
    aa.st_adv[2 * idx + 1] = aa.ab[slot];
}

// shade_body's alpha-blend flavour (kernels.hpp, AB): the albedo and the miss colour through ApplyAlphaBlend with the slot's plane
template <int MS>
__global__ void ATN_SHADE_ATTR __launch_bounds__(256) k_shade_ab(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, int32_t bounce, const float4* ab)
{
    shade_body<false, MS, false, false, false, true>(pb, sc, fp, cam, bounce, SvgfShade{}, RegenOut{}, ab);
}
template <int MS, int WAVES>
__global__ void __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) __launch_bounds__(256) k_shade_ab_wn(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, int32_t bounce,
                                                                                                       const float4* ab)
{
    shade_body<false, MS, false, false, false, true>(pb, sc, fp, cam, bounce, SvgfShade{}, RegenOut{}, ab);
}

#endif  // ATN_NPR_ADVANCE_TU

} // namespace atn
