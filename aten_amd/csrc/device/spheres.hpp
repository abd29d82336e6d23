// Analytic spheres in the walk (atn_set_sphere_intersection(1), docs/SPHERES.md): the kernels of a scene whose top layer holds sphere
// leaves.  Each is its triangle-only sibling of kernels.hpp with the walk's and the shade body's SPH flag set -- the sphere step rides
// with the leaf step of walk_iteration (traverse.hpp, sphere_test), a hit record with tri < 0 is evaluated as a sphere's
// (shading.hpp, evaluate_sphere_hit) -- and nothing else changed; they are launched only when the uploaded scene has such a leaf.
// The shadow jobs are the ALPHA = false flavour: a sphere's hit has no triangle to read a material from, and frames of a scene whose
// materials a shadow ray may look through are refused while sphere leaves are uploaded.
#pragma once
#include "kernels.hpp"

namespace atn {

template <bool COUNT, bool REFILL>
__global__ void __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_sph_trace_closest(PathBuffers pb, DevScene sc, int32_t bounce)
{
    const uint32_t count = pb.q_count[bounce];
    const ClosestJobT<COUNT> job{ pb, pb.queue[bounce & 1], kEps, pb.doomed_bit, pb.doomed_stop, (uint32_t)(bounce & 1) * pb.isect_odd };
    TravCounters tc{};
    trace_dispatch<COUNT, REFILL, ClosestJobT<COUNT>, false, true>(sc, count, &pb.fetch_closest[bounce], job, &tc);
    if (COUNT) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&pb.stats[0], (unsigned long long)count);
        wave_add_stat(&pb.stats[3], tc.nodes);
        wave_add_stat(&pb.stats[4], tc.tris);
    }
}

template <bool COUNT, bool REFILL>
__global__ void __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_sph_trace_shadow(PathBuffers pb, DevScene sc, int32_t bounce)
{
    const uint32_t count = pb.sh_count[bounce];
    const ShadowJob<false> job{ pb, sc, kEps };
    TravCounters tc{};
    trace_dispatch<COUNT, REFILL, ShadowJob<false>, false, true>(sc, count, &pb.fetch_shadow[bounce], job, &tc);
    if (COUNT) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&pb.stats[1], (unsigned long long)count);
        wave_add_stat(&pb.stats[5], tc.nodes);
        wave_add_stat(&pb.stats[6], tc.tris);
    }
}

template <bool REFILL, bool LDSN>
__global__ void ATN_TRACE_ATTR __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_sph_trace_fused(PathBuffers pb, DevScene sc, int32_t bs, int32_t bc, int32_t launch)
{
    const uint32_t n_shadow = bs >= 0 ? pb.sh_count[bs] : 0u;
    const uint32_t n_closest = bc >= 0 ? pb.q_count[bc] : 0u;
    const FusedJob<false> job{ ShadowJob<false>{ pb, sc, kEps }, ClosestJobT<true>{ pb, pb.queue[(bc >= 0 ? bc : 0) & 1], kEps, pb.doomed_bit, pb.doomed_stop,
                                                                                  (uint32_t)((bc >= 0 ? bc : 0) & 1) * pb.isect_odd }, n_shadow, kEps };
    TravCounters tc{};
    trace_dispatch<false, REFILL, FusedJob<false>, LDSN, true>(sc, n_shadow + n_closest, &pb.fetch_closest[launch], job, &tc);
}

// atn_trace_closest's job (kernels.hpp, BatchJob) where a hit may be a sphere leaf's: sphere.mtrl_id and the leaf's mesh id
struct SphBatchJob {
    DevScene sc;
    const atn_ray* __restrict__ rays;
    atn_intersection* out;
    float t_min, t_max;
    ATN_DEV void fetch(uint32_t j, float4& a, float4& b, float& stop_t) const
    {
        const atn_ray r = rays[j];
        stop_t = -kInf;
        a = make_float4(r.org[0], r.org[1], r.org[2], t_max);
        b = make_float4(r.dir[0], r.dir[1], r.dir[2], __uint_as_float(j));
    }
    ATN_DEV bool finish(uint32_t j, const Hit& h, bool, float4&, float4&, float&) const
    {
        atn_intersection o;
        o.t = h.t; o.objid = h.objid; o.tri_id = h.tri; o.a = h.a; o.b = h.b; o.isVoxel = 0;
        o.mtrlid = -1; o.meshid = -1;
        if (h.objid >= 0 && h.tri < 0) {
            o.mtrlid = sc.objects[h.objid].sphere.mtrl_id;
            o.meshid = h.meshid;
        }
        else if (h.objid >= 0) {
            const atn_triangle_param tp = sc.tris[h.tri];
            o.mtrlid = tp.mtrlid;
            o.meshid = tp.mesh_id < 0 ? h.meshid : tp.mesh_id;     // threaded_bvh_traverser.h:206-209
        }
        out[j] = o;
        return false;
    }
    ATN_DEV void cost(uint32_t, uint32_t, uint32_t) const {}
};

template <bool COUNT, bool REFILL>
__global__ void __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_sph_trace_batch(DevScene sc, const atn_ray* __restrict__ rays, uint32_t n,
                                                                                          float t_min, float t_max, atn_intersection* out,
                                                                                          unsigned long long* stats)
{
    const SphBatchJob job{ sc, rays, out, t_min, t_max };
    TravCounters tc{};
    trace_dispatch<COUNT, REFILL, SphBatchJob, false, true>(sc, n, reinterpret_cast<uint32_t*>(&stats[7]), job, &tc);     // stats[7]: zeroed fetch cursor
    if (COUNT) { wave_add_stat(&stats[3], tc.nodes); wave_add_stat(&stats[4], tc.tris); }
}

template <int MS>
__global__ void ATN_SHADE_ATTR __launch_bounds__(256) k_sph_shade(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, int32_t bounce)
{
    shade_body<false, MS, false, false, false, false, true>(pb, sc, fp, cam, bounce, SvgfShade{});
}
template <int MS, int WAVES, bool LA>
__global__ void __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) __launch_bounds__(256) k_sph_shade_wn(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, int32_t bounce)
{
    shade_body<false, MS, false, LA, false, false, true>(pb, sc, fp, cam, bounce, SvgfShade{});
}

} // namespace atn
