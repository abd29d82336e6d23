// Launch policy shared by the translation units of libaten_amd.so (build.py: HIP_UNITS, compiled in parallel under their own flags):
// what a pass launches (PassPlan: PathTracing::plan_pass), which kernel instantiation each launch gets, and the launchers regen.hip and
// shade_relaxed.hip export to aten_amd.hip.
#pragma once
#include <type_traits>
#include "kernels.hpp"

namespace atn {

// f(std::bool_constant<flags>{}...): runtime flags -> template arguments, one instantiation per combination
template <class F>
void with_flags(F&& f) { f(); }
template <class F, class... B>
void with_flags(F&& f, bool flag, B... rest)
{
    if (flag) with_flags([&](auto... x) { f(std::true_type{}, x...); }, rest...);
    else with_flags([&](auto... x) { f(std::false_type{}, x...); }, rest...);
}

// f(ShadeFlavour<MS, WAVES>{}) launches the shade instantiation of a material set (BSDFs no uploaded material uses are compiled out):
// the three smaller sets held to `waves` = 4 / 5 waves per SIMD (kernels.hpp, k_shade_wn), CarPaint and Toon unconstrained (WAVES = 0)
template <int MS, int WAVES>
struct ShadeFlavour { static constexpr int ms = MS, waves = WAVES; };
template <class F>
void with_shade_flavour(int material_set, int waves, F&& f)
{
    switch (material_set) {
    case kMsCore: if (waves == 5) f(ShadeFlavour<kMsCore, 5>{}); else f(ShadeFlavour<kMsCore, 4>{}); break;
    case kMsDisney: if (waves == 5) f(ShadeFlavour<kMsDisney, 5>{}); else f(ShadeFlavour<kMsDisney, 4>{}); break;
    case kMsAnalytic: if (waves == 5) f(ShadeFlavour<kMsAnalytic, 5>{}); else f(ShadeFlavour<kMsAnalytic, 4>{}); break;
    case kMsCarPaint: f(ShadeFlavour<kMsCarPaint, 0>{}); break;
    default: f(ShadeFlavour<kMsToon, 0>{}); break;
    }
}

// launch geometry: enough waves to fill 256 CUs several times over; grid-stride loops do the rest
inline uint32_t grid_for(uint32_t n, uint32_t cap_blocks = 256u * 16u)
{
    uint32_t b = (n + 255u) / 256u;
    if (b == 0) b = 1;
    return b < cap_blocks ? b : cap_blocks;
}

enum class PassKind { Serial, Svgf, Regen };

// What one pass over n paths launches: the serial sample loop of a batch, the SVGF path pass of a batch, or a regenerated burst.
struct PassPlan {
    PassKind kind;
    bool refill;                // the persistent lane-refilling walk (deep trees) / the plain walk
    uint32_t lds_bytes;         // the LDS copy of the node image the walk reads (0: the walk reads global memory)
    uint32_t block;             // threads per block of the plain walk's fused launches
    uint32_t trace_grid;        // blocks of an unfused trace launch (n jobs)
    uint32_t fused_grid;        // blocks of a fused trace launch (2n jobs; in 256-thread blocks for the plain walk)
    int shade_items;            // queue entries per thread and chunk of the shade launches (FrameParams::chunk_items)
    uint32_t shade_grid;
    int shade_waves;            // 4 / 5 (with_shade_flavour)
    bool sph = false;           // the uploaded scene has sphere leaves: the pass launches the sphere-aware kernels (spheres.hip)
};

// One fused trace launch of a pass: shadow rays of stage - 1 + closest-hit rays of stage
struct TraceLaunch {
    bool closest;               // k_trace_closest<false, false> instead of k_trace_fused
    bool refill, lds;
    uint32_t grid, block, lds_bytes;
    int prof_kind;              // ATN_K_*
    bool sph = false;           // PassPlan::sph
};

// ---- spheres.hip (device/spheres.hpp): the sphere-aware siblings of the serial loop's launches, for scenes with sphere leaves ----
void sph_launch_trace(bool shadow, bool count, bool refill, uint32_t grid, uint32_t block, hipStream_t st, const PathBuffers& pb, const DevScene& sc, int32_t b);
void sph_launch_trace_fused(const TraceLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, int32_t bs, int32_t bc, int32_t launch);
void sph_launch_batch(bool count, bool refill, uint32_t grid, uint32_t block, hipStream_t st, const DevScene& sc, const atn_ray* rays, uint32_t n,
                      float t_min, float t_max, atn_intersection* out, unsigned long long* stats);
// -1 = the material set has no sphere-aware shade (toon)
int sph_launch_shade(int material_set, int waves, bool la, uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                     const atn_camera_param& cam, int32_t bounce);

inline TraceLaunch trace_launch(const PassPlan& p, int32_t stage)
{
    // the first launch holds only primary rays: coherent, they finish together, and the refill bookkeeping buys nothing (sponza_lod
    // 4.33 -> 4.30 ms, atrium 4K 221 -> 219 ms)
    const bool refill = p.refill && stage != 0;
    // Only closest-hit rays in the first launch of a serial sample (there is no bounce -1 to cast shadows): the closest-hit kernel is
    // the same walk without the shadow job's code in it (every ray's stop_t is a constant there; the fused kernel's plain flavour grew
    // by the any-hit twins' root selection: primary rays 0.168 -> 0.203 ms per frame, back at 0.168 through this launch).  The
    // regenerated pool's stage 0 keeps the fused kernel.
    const bool closest = p.kind != PassKind::Regen && stage == 0 && p.lds_bytes == 0u;
    // (timed under "trace_closest" when it is a different kernel from the other launches: the roofline of k_trace_fused<true, .> is
    // about those)
    return TraceLaunch{ closest, refill, p.lds_bytes != 0u, refill ? p.fused_grid : p.fused_grid * (256u / p.block),
                        refill ? (uint32_t)kTraceBlock : p.block, p.lds_bytes, p.refill && stage == 0 ? ATN_K_TRACE_CLOSEST : ATN_K_TRACE_FUSED, p.sph };
}

// aten_amd.hip instantiates REGEN = false (the serial loop), regen.hip REGEN = true (the regenerated pool)
template <bool REGEN>
void launch_trace_fused(const TraceLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, int32_t bs, int32_t bc, int32_t launch)
{
    const dim3 g(l.grid), t(l.block);
    if constexpr (!REGEN) if (l.sph) { sph_launch_trace_fused(l, st, pb, sc, bs, bc, launch); return; }
    if constexpr (!REGEN) if (l.closest) { hipLaunchKernelGGL((k_trace_closest<false, false>), g, t, l.lds_bytes, st, pb, sc, bc); return; }
    with_flags([&](auto refill, auto alpha, auto lds) {
        hipLaunchKernelGGL((k_trace_fused<decltype(refill)::value, decltype(alpha)::value, decltype(lds)::value, REGEN>), g, t, l.lds_bytes, st, pb, sc, bs, bc, launch);
    }, l.refill, sc.any_alpha != 0, l.lds);
}

// The launches of a renderer that walks a ray list of its own beside the pass (NPR's sample rays, the AO rays, the shadow pre-pass's
// shadow rays, the volume walks): shade-like kernels over the queue, per-slot kernels, and the list's rays through the frame's walk
// (the plan's walk, LDS copy and block).
struct RayLaunch {
    uint32_t grid;              // blocks of 256, grid-stride over the queue (prep / eval / shade)
    uint32_t slot_grid;         // blocks of 256 over all slots (begin, resolve, reduce)
    bool refill;
    uint32_t trace_grid, trace_block, lds_bytes;
};
// `refill_grid`: the refill walk's blocks for the list's n_rays jobs -- PathTracing::trace_grid(n_rays, true), which follows the frames
// in flight; the volume walks (one job per path) take the plan's own trace_grid
inline RayLaunch ray_launch(const PassPlan& p, uint32_t n_slots, uint32_t n_rays, uint32_t refill_grid)
{
    RayLaunch l{};
    l.grid = grid_for(n_slots); l.slot_grid = (n_slots + 255u) / 256u;
    l.refill = p.refill; l.lds_bytes = p.lds_bytes;
    l.trace_block = p.refill ? (uint32_t)kTraceBlock : p.block;
    l.trace_grid = p.refill ? refill_grid : grid_for(n_rays) * (256u / p.block);
    return l;
}

// svgf_pixel's tiles over a frame (8 x 32 pixels per block of 256; x rounded up to a multiple of 8, one strip per XCD): the motion pass
// and the display tail; a ragged frame's last tiles are partly outside it
struct TileLaunch { uint32_t grid_x, grid_y; };
inline TileLaunch tile_launch(int32_t width, int32_t height)
{
    return TileLaunch{ (uint32_t)((((width + 7) / 8) + 7) / 8 * 8), (uint32_t)((height + 31) / 32) };
}

// Node-wide SVGF's two data movers (device/svgf_gather.hpp), one thread per slot in blocks of 256: the pack over a shard's slots, the
// unpack over the slots of every shard but the first (0 blocks with one shard: nothing to launch)
struct GatherLaunch { uint32_t pack_grid, unpack_grid; };
inline GatherLaunch svgf_gather_launch(uint32_t n_slots, int32_t world)
{
    const uint64_t gathered = (uint64_t)(world > 1 ? world - 1 : 0) * n_slots;
    return GatherLaunch{ (n_slots + 255u) / 256u, (uint32_t)((gathered + 255u) / 256u) };
}

// ---- regen.hip (PathTracing::render_regen) ----
void regen_launch_begin(uint32_t grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, const atn_camera_param& cam);
// shadow rays of stage bs (< 0: none) + closest-hit rays of stage bc (< 0: none); `launch` indexes the job-fetch cursor
void regen_launch_trace(const TraceLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, int32_t bs, int32_t bc, int32_t launch);
void regen_launch_shade(int material_set, int waves, uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                        const atn_camera_param& cam, int32_t stage, const RegenOut& ro);
// the stable compaction in front of trace(stage): regions written by shade(stage - 1) (by regen_launch_begin for stage 0) -> dense queues
void regen_launch_compact(uint32_t grid, hipStream_t st, const PathBuffers& pb, int32_t stage, uint32_t chunk_size, uint32_t* group_counts_next, uint32_t n_groups);
// the pending epilogues of retired slots (per slot), in front of regen_launch_end (per pixel)
void regen_launch_flush(uint32_t grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, const RegenOut& ro);
void regen_launch_end(uint32_t grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, const RegenOut& ro);

// ---- shade_relaxed.hip ----
void relaxed_launch_shade(int material_set, int waves, uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                          const atn_camera_param& cam, int32_t bounce);

// ---- restir.hip (device/restir.hpp) ----
struct RestirArgs;
void restir_launch_shade(int material_set, uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                         const atn_camera_param& cam, const RestirArgs& ra);
void restir_launch_vis_prep(uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const RestirArgs& ra);
void restir_launch_temporal(int material_set, bool temporal, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                            const RestirArgs& ra);
void restir_launch_spatial(int material_set, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const RestirArgs& ra);
void restir_launch_color(int material_set, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const RestirArgs& ra);
void restir_launch_motion(hipStream_t st, const FrameParams& fp, const RestirArgs& ra);

// ---- npr.hip (device/npr.hpp) ----
struct NprArgs;
// one bounce's NPR launches: prep and eval over the bounce's queue, the sample rays through the frame's walk (8 rays per path)
void npr_launch_gen(uint32_t grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, const NprArgs& na);
void npr_launch_bounce(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                       const atn_camera_param& cam, const NprArgs& na, int32_t bounce);
void npr_launch_capture0(uint32_t grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, const NprArgs& na);

// ---- npr_advance.hip (device/npr_advance.hpp) ----
struct NprAdvArgs;
// the alpha-blend plane and the look-through's records of a sample, per slot
void npr_adv_launch_init(uint32_t slot_grid, hipStream_t st, const FrameParams& fp, const NprAdvArgs& aa);
// one bounce's look-through between npr_launch_bounce and the shade launch: the job over the queue NPR's eval left, through the frame's walk
void npr_adv_launch_bounce(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const NprAdvArgs& aa, int32_t bounce);
void npr_adv_launch_capture0(uint32_t slot_grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, const NprAdvArgs& aa);
// the shade launch's alpha-blend flavour; -1 = the material set has none (CarPaint)
int npr_adv_launch_shade(int material_set, int waves, uint32_t grid, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                         const atn_camera_param& cam, int32_t bounce, const float4* ab);

// ---- ao.hip (device/ao.hpp) ----
struct AoArgs;
// one AO frame's launches after k_gen_path: the primary rays (the pass's first trace launch, with the AO job), shade over the queue,
// the AO rays through the frame's walk (num_rays rays per path), resolve per slot
void ao_launch_primary(const TraceLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const AoArgs& aa);
void ao_launch_rays(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const AoArgs& aa);
void ao_launch_resolve(const RayLaunch& l, hipStream_t st, const FrameParams& fp, const AoArgs& aa, float4* film, float4* tile_out);

// ---- npr_shadow.hip (device/npr_shadow.hpp) ----
struct NsArgs;
// the shadow pre-pass's launches after k_gen_path: the primary rays (the pass's first trace launch, with a job that keeps t), shade over
// the queue, the shadow rays through the frame's walk (one per path), the row filter over w x h pixels
void ns_launch_primary(const TraceLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const NsArgs& na);
void ns_launch_rays(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp, const NsArgs& na);
void ns_launch_filter(hipStream_t st, const float* lit, const float* depth, float* out, int32_t width, int32_t height);

// ---- npr_hatching.hip (device/npr_hatching.hpp) ----
// the AO rays' answers (ao_launch_primary / ao_launch_rays over `aa`) folded into the pre-pass's source and depth planes, per slot
void nh_launch_resolve(uint32_t slot_grid, hipStream_t st, const FrameParams& fp, const AoArgs& aa, float* src, float* depth);
// the filter of one HatchingShadowDirection (0..5) over w x h pixels; `first` receives the first step's plane of directions 4 / 5
void nh_launch_filter(int32_t direction, hipStream_t st, const float* src, const float* depth, float* first, float* out, int32_t width, int32_t height);

// ---- volume.hip (device/volume.hpp) ----
struct VolArgs;
// one iteration's volume launches: the closest-hit walk and the connection walk through the frame's walk (one job per path), the shade
// over the iteration's queue
void vol_launch_begin(const RayLaunch& l, hipStream_t st, const FrameParams& fp, const VolArgs& va);
void vol_launch_closest(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const VolArgs& va, int32_t it);
void vol_launch_shade(int material_set, const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                      const atn_camera_param& cam, const VolArgs& va, int32_t it);
void vol_launch_transmit(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const VolArgs& va, int32_t it);
void vol_launch_reduce(const RayLaunch& l, hipStream_t st, const FrameParams& fp, const VolArgs& va);
void vol_launch_phase_table(hipStream_t st, float g, uint32_t n, const float* w, const float* r1, const float* r2, const float* wo, float* out_dir, float* out_eval);
// ---- volume_grid.hip (device/volume_grid.hpp): the shade and connection launches of a frame whose media name a grid ----
struct VolGridArgs;
void vol_launch_shade_grid(int material_set, const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const FrameParams& fp,
                           const atn_camera_param& cam, const VolArgs& va, const VolGridArgs& vg, int32_t it);
void vol_launch_transmit_grid(const RayLaunch& l, hipStream_t st, const PathBuffers& pb, const DevScene& sc, const VolArgs& va, const VolGridArgs& vg, int32_t it);

// ---- skinning.hip (device/skinning.hpp) ----
struct SkinVtxArgs;
struct SkinTriArgs;
// one skinning tick's two launches: a block of 256 per 256 vertices / triangles (the triangle pass always has its block 0: it
// finishes the box), the palette in LDS when it fits
struct SkinLaunch {
    uint32_t vtx_grid, tri_grid;
    bool palette_lds;
};
inline SkinLaunch skin_launch(uint32_t n_vtx, uint32_t n_tri, uint32_t n_matrices, uint32_t palette_lds_max)
{
    SkinLaunch l{};
    l.vtx_grid = (n_vtx + 255u) / 256u;
    l.tri_grid = n_tri ? (n_tri + 255u) / 256u : 1u;
    l.palette_lds = n_matrices <= palette_lds_max;
    return l;
}
void skin_launch_vertices(const SkinLaunch& l, hipStream_t st, const SkinVtxArgs& a);
void skin_launch_triangles(const SkinLaunch& l, hipStream_t st, const SkinTriArgs& a);
// k_lbvh_morton with the box in device memory (min xyz, max xyz)
void skin_launch_morton(hipStream_t st, const atn_triangle_param* tris, const float4* vtx, int32_t vtx_offset, uint32_t n, const float* box,
                        uint32_t* codes, uint32_t* indices);

// ---- tlas.hip (device/tlas.hpp) ----
struct TlasArgs;
// a top-layer rebuild over n >= 2 instances: the block path (one launch of one workgroup, a power of two >= n threads) up to
// `block_max` instances unless the general path is forced; the general path's grids are blocks of 256 over the leaves / the nodes
struct TlasLaunch {
    bool block_path;
    uint32_t block;             // threads of the block path's workgroup
    uint32_t leaf_grid, node_grid;
};
inline TlasLaunch tlas_launch(uint32_t n, uint32_t block_max, bool force_general)
{
    TlasLaunch l{};
    l.block_path = n <= block_max && !force_general;
    l.block = 64u;
    while (l.block < n && l.block < block_max) l.block <<= 1;
    l.leaf_grid = (n + 255u) / 256u;
    l.node_grid = (2u * n - 1u + 255u) / 256u;
    return l;
}
void tlas_launch_block(const TlasLaunch& l, hipStream_t st, const TlasArgs& a);
// the general path in front of the sort (leaf boxes, union box, codes) ...
void tlas_launch_codes(const TlasLaunch& l, hipStream_t st, const TlasArgs& a);
// ... and behind k_lbvh_hierarchy (boxes, links and records)
void tlas_launch_emit(const TlasLaunch& l, hipStream_t st, const TlasArgs& a);

// ---- motion.hip (device/motion.hpp) ----
struct MotionArgs;
// the primary hit records of slots [fp.slot_begin, fp.slot_end) -> the ids plane; `grid` blocks of 256 over those slots
void motion_launch_capture(uint32_t grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, float4* ids);
// the motion pass over a frame's tiles
void motion_launch_geometry(const TileLaunch& l, hipStream_t st, const MotionArgs& a);
void motion_launch_copy(hipStream_t st, float4* dst, const float4* src, uint32_t n_quads);

// ---- taa.hip (device/taa.hpp) ----
struct TaaArgs;
// the display tail over a frame's tiles
void taa_launch_resolve(const TileLaunch& l, hipStream_t st, const TaaArgs& a);

} // namespace atn
